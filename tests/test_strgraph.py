"""The class of a row, the two arcs of a dovetail, the check against the lengths, the duplicate rule, the witness test, the search in the
sorted arc array and the walk of one arc of hsk_overlaps_reduce (hysortk_amd/csrc/hsk_strgraph.h: what the kernels and this test share) on the
CPU, under the address and undefined-behaviour sanitizers: tests/strgraph_test.cpp holds them to a brute-force O(n^3) reduction written from
the definition -- every (o, e) of the 2 x 16, every combination of coordinates and ends bits on short reads, the search on runs of 0, 1 and
2 records and on dead records, whole random graphs with duplicates, exchanged rows, contained reads and self rows, and lengths next to 2^32
where the sums need 64 bits.  And the ctypes mirrors of the call's two structs against the header."""
import ctypes as C
import os
import subprocess

from tests import util


def test_row_rules_search_and_reduction_under_sanitizers(tmp_path):
    exe = str(tmp_path / "strgraph_test")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                           os.path.join(util.ROOT, "tests", "strgraph_test.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0 and out.startswith("OK"), out


def test_struct_sizes_match_header(tmp_path):
    from hysortk_amd import _lib
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "hsk.h"\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(hsk_reduce_opts), sizeof(hsk_reduced), offsetof(hsk_reduced, ms_classify), offsetof(hsk_reduced, priv));return 0;}\n'
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(util.ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = subprocess.check_output([str(tmp_path / "t")]).decode().split()
    assert [int(x) for x in out] == [C.sizeof(_lib.ReduceOpts), C.sizeof(_lib.Reduced), _lib.Reduced.ms_classify.offset, _lib.Reduced.priv.offset]
