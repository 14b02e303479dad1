"""The base accessors of the four sides, the cell with its packed (score, edits) pair, the best rule, the serial walk and the overlap row of
hsk_pair_diags_extend_gapped (hysortk_amd/csrc/hsk_gapped.h: what the kernel and this test share) on the CPU, under the address and
undefined-behaviour sanitizers: tests/gapped_test.cpp holds them to a plain full-matrix DP written from the definition -- every base of
every side from every offset, reads at every byte phase that end in the last byte of a heap block of exactly the packed size, both
orientations, K = 3, 31, 51, 77, bands 0, 1, 7, 8, 63, every seed offset of short reads, a drop of exactly xdrop (goes on) and of
xdrop + 1 (stops), mismatch 0, gap 0, xdrop 0, and match = mismatch = gap = 255 on reads with la + lb = 2^22 - 1."""
import os
import subprocess

from tests import util


def test_sides_cells_and_rows_under_sanitizers(tmp_path):
    exe = str(tmp_path / "gapped_test")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                           os.path.join(util.ROOT, "tests", "gapped_test.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0 and out.startswith("OK"), out
