"""The gather of hsk_result_strands (hysortk_amd/csrc/hsk_strandbits.h: strand_load, strand_twin, strand_decide) on the CPU, under the
address and undefined-behaviour sanitizers: tests/strandbits_test.cpp loads the K bases at every position of reads whose last k-mer ends
in the last byte of a heap block of exactly the packed reads' size -- K = 3, 4, 21, 31, 33, 51, 63, 65, 77, 95 and a few even K, every bit
offset, every byte phase of the read's start against the aligned words the load reads -- and holds them to k-mers built base by base; the
strand is held to a reverse complement taken on the strings: forward, reverse, palindromes (ACGT repeats, even K) and k-mers that are
neither, which must be reported as a mismatch."""
import os
import subprocess

from tests import util


def test_loads_and_strands_under_sanitizers(tmp_path):
    exe = str(tmp_path / "strandbits_test")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                           os.path.join(util.ROOT, "tests", "strandbits_test.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0 and out.startswith("OK"), out
