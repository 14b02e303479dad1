"""The out-arcs of a vertex over its run of the sorted arc array, the link test, the state of a vertex and the step that doubles it, the cut of
a cycle, the canonical rule and the row packers of hsk_overlaps_unitigs (hysortk_amd/csrc/hsk_unitig.h: what the kernels and this test share)
on the CPU, under the address and undefined-behaviour sanitizers: tests/unitig_test.cpp runs the kernels' steps on them -- the ranking as a
host loop that applies the doubling step round by round on two buffers -- and holds the result to a sequential walk written from the
definition, on lines and rings of 1 to 1025 reads, on random graphs with forks, joins, parallel arcs and contained reads, and on lengths next
to 2^32; the rounds must stay within 2 ceil(log2(2 nreads)) + 4.  And the ctypes mirrors of the call's two structs against the header."""
import ctypes as C
import os
import subprocess

from tests import util


def test_rules_and_doubling_against_a_walk_under_sanitizers(tmp_path):
    exe = str(tmp_path / "unitig_test")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                           os.path.join(util.ROOT, "tests", "unitig_test.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0 and out.startswith("OK"), out


def test_struct_sizes_match_header(tmp_path):
    from hysortk_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "hsk.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(hsk_unitig_opts), sizeof(hsk_unitigs), '
           'offsetof(hsk_unitigs, table), offsetof(hsk_unitigs, singletons), offsetof(hsk_unitigs, rounds), offsetof(hsk_unitigs, ms_arcs), offsetof(hsk_unitigs, priv));return 0;}\n')
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(util.ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = subprocess.check_output([str(tmp_path / "t")]).decode().split()
    U = _lib.Unitigs
    assert [int(x) for x in out] == [C.sizeof(_lib.UnitigOpts), C.sizeof(U), U.table.offset, U.singletons.offset, U.rounds.offset, U.ms_arcs.offset, U.priv.offset]
    assert "hsk_overlaps_unitigs" in _lib.SYMBOLS and "hsk_unitigs_free" in _lib.SYMBOLS
