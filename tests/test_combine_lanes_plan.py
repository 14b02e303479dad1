"""The lane assignment of combine_kernel's deduplicating instance (hysortk_amd/csrc/hsk_lanes.h: the packed scan value, the offsets beside the
multiplicities, n = ceil(T / 256), the binary search over the offsets and a piece's walk over item ends) on the CPU, under the address and
undefined-behaviour sanitizers: tests/combine_lanes_test.cpp builds the list as the compaction does -- from every vector of item counts of up to
six slots, every count alone and in pairs, full tables and random ones of up to 1024 items -- and holds the 256 pieces to a brute-force
enumeration: every k-mer of the stream is taken exactly once, in order, with its entry's multiplicity."""
import os
import subprocess

from tests import util


def test_every_kmer_of_the_stream_is_taken_once_under_sanitizers(tmp_path):
    exe = str(tmp_path / "combine_lanes_test")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                           os.path.join(util.ROOT, "tests", "combine_lanes_test.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0 and out.startswith("OK"), out
