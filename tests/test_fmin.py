"""The clamp-and-detect arithmetic behind scan_kernel's window minima (hysortk_amd/csrc/hsk_fmin.h: 64-bit minima as double-precision minima of
hashes whose top word is capped at a sentinel below the NaN range) on the CPU, under the address and undefined-behaviour sanitizers:
tests/fmin_test.cpp holds a chain of such minima, and a lane's eight windows built as the kernel builds them, to a brute-force unsigned minimum
-- every pair and triple of the edge patterns (around the sentinel and 0x7FF00000, zero, all ones, the sign bit, denormals, equal top words
with different low words), and 60000 windows of 8 to 64 hashes with none, some, most and all of their hashes in the sentinel class."""
import os
import subprocess

from tests import util


def test_clamped_double_minima_are_exact_or_say_so_under_sanitizers(tmp_path):
    exe = str(tmp_path / "fmin_test")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                           os.path.join(util.ROOT, "tests", "fmin_test.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0 and out.startswith("OK"), out
