"""The arithmetic of pair_finish_kernel (hysortk_amd/csrc/hsk_pairrank.h: which key bits make the bucket, a pair's rank from its bucket's start,
the smaller keys of the bucket and the equal keys that arrived before it, which element of a run of equal keys carries the sum, the [L, U]
filter on the SUM, and the output slot from the popcounts of the kept-heads mask) on the CPU, under the address and undefined-behaviour
sanitizers: tests/pairfinish_test.cpp runs every bin of up to twelve pairs over three keys (two of them in one bucket), sums that land on and
beside the bounds from partial counts on the other side, 65535 / 65536 / 65537, and random bins of up to 2048 pairs -- uniform keys, one bucket
for the whole bin, long runs of equal keys -- in random arrival orders, and holds each to the sorted, merged, filtered list; every pair is
accounted for exactly once (the ranks are a permutation in key order, the heads' sums add up to the bin's counts)."""
import os
import subprocess

from tests import util


def test_every_bin_is_sorted_merged_filtered_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pairfinish_test")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                           os.path.join(util.ROOT, "tests", "pairfinish_test.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0 and out.startswith("OK"), out
