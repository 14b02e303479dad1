"""The no-HIP parts of the merge of row lists (hysortk_amd/csrc/hsk_rowmerge.h: the row shapes PairRow and DiagRow, mp_before, mp_same,
mp_split, mp_join) on the CPU, under the address and undefined-behaviour sanitizers: tests/rowmerge_test.cpp holds the merge-path split,
for every diagonal of lists of up to a few hundred rows, to a plain two-pointer merge, and replays the kernel's tile-by-tile merge
(ownership by A's copy, look-behind, look-ahead) against that merge's joined rows -- empty sides, one list below the other, every row in
both, a shared row at every position, keys with bit 63 set; for both shapes, the six-word rows compared on (key, bin) and the four-word rows
compared on the key; and for the two-word compare also equal keys with interleaved bins, bins at 1 and around 2^33."""
import os
import subprocess

from tests import util


def test_split_and_join_follow_the_two_pointer_merge_under_sanitizers(tmp_path):
    exe = str(tmp_path / "rowmerge_test")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                           os.path.join(util.ROOT, "tests", "rowmerge_test.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0 and out.startswith("OK"), out
