"""The windows, the mismatch masks, the x-drop step by runs, the valid columns and the overlap row of hsk_pair_diags_extend
(hysortk_amd/csrc/hsk_xdrop.h: what the kernels, the host and this test share) on the CPU, under the address and undefined-behaviour
sanitizers: tests/xdrop_test.cpp takes windows at every base offset and byte phase of reads that end in the last byte of a heap block of
exactly the packed size, forward and reverse-complemented, against strings; the step against the column-by-column loop of the definition
on random masks -- every start column mod 32, spans around 31/32/33 and 63/64/65, xdrop 0, a drop of exactly xdrop (goes on) and of
xdrop + 1 (stops), mismatch 0, match = mismatch = 2^15 with a 64-bit score --; t_lo and t_hi for both orientations with seeds flush with a
read's start or end; and whole walks and rows (coordinates, mismatches, ends) of overlaps cut from a genome, K = 3, 31, 51, 77."""
import os
import subprocess

from tests import util


def test_windows_steps_and_rows_under_sanitizers(tmp_path):
    exe = str(tmp_path / "xdrop_test")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                           os.path.join(util.ROOT, "tests", "xdrop_test.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0 and out.startswith("OK"), out
