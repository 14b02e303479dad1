"""The no-HIP parts of the merge of all-bins row lists (hysortk_amd/csrc/hsk_diagmerge.h: dm_before, dm_split, dm_join) on the CPU, under
the address and undefined-behaviour sanitizers: tests/diagmerge_test.cpp holds the merge-path split over two-word keys, for every diagonal
of lists of up to a few hundred rows, to a plain two-pointer merge, and replays the kernel's tile-by-tile merge (ownership by A's copy,
look-behind, look-ahead) against that merge's joined rows -- empty sides, one list below the other, equal keys with interleaved bins, a
shared (key, bin) at every position, keys with bit 63 set, bins at 1 and around 2^33."""
import os
import subprocess

from tests import util


def test_split_and_join_follow_the_two_pointer_merge_under_sanitizers(tmp_path):
    exe = str(tmp_path / "diagmerge_test")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                           os.path.join(util.ROOT, "tests", "diagmerge_test.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0 and out.startswith("OK"), out
