"""Read pairs by diagonal (hsk_result_pair_diagonals, include/hsk.h) without a GPU: the bin arithmetic of hysortk_amd/csrc/hsk_diagbin.h on
the CPU under the address and undefined-behaviour sanitizers (tests/diagbin_test.cpp), the selection and the host join of PairDiagonals on
rows made by hand, and the C ABI's new surface -- the exports, the layout of hsk_pair_diags against its ctypes mirror, and the refusals that
need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import util

TOP = 1 << 63


def test_bin_arithmetic_is_exact_under_sanitizers(tmp_path):
    exe = str(tmp_path / "diagbin_test")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                           os.path.join(util.ROOT, "tests", "diagbin_test.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0 and out.startswith("OK"), out


def _v(pa, pb):
    return (pa << 32) | pb


def _allbins(rows, **kw):
    """rows: (key, bin, support, first, last) -> an all-bins PairDiagonals"""
    from hysortk_amd import PairDiagonals
    r = np.array([[k, s, b, s, f, l] for k, b, s, f, l in rows], dtype=np.uint64).reshape(-1, 6)
    return PairDiagonals.from_rows(r, diag_bin=kw.pop("diag_bin", 16), all_bins=True, **kw)


K1, K2, K3 = (1 << 32) | 2, (1 << 32) | 3, TOP | (1 << 32) | 2


def test_select_on_hand_made_rows():
    ab = _allbins([
        (K1, 5, 3, _v(1, 1), _v(9, 9)), (K1, 9, 7, _v(20, 2), _v(30, 3)), (K1, 11, 7, _v(40, 4), _v(50, 5)), (K1, 12, 1, _v(60, 6), _v(60, 6)),      # a tie: the smaller bin
        (K2, 4, 1, _v(7, 7), _v(7, 7)),                                                                                                         # a single bin
        (K3, 2, 2, _v(3, 3), _v(4, 4)), (K3, 3, 2, _v(5, 5), _v(6, 6)), (K3, 8, 1, _v(8, 8), _v(8, 8)),                                           # a tie at the front
    ])
    best = ab.select()
    assert not best.all_bins and best.diag_bin == 16 and best.info["keys"] == 3
    assert best.rows().tolist() == [[K1, 18, 9, 7, _v(20, 2), _v(30, 3)], [K2, 1, 4, 1, _v(7, 7), _v(7, 7)], [K3, 5, 2, 2, _v(3, 3), _v(4, 4)]]
    assert best.opposite.tolist() == [False, False, True] and best.rid_a.tolist() == [1, 1, 1] and best.rid_b.tolist() == [2, 3, 2]
    assert (best.first_pos_a.tolist(), best.first_pos_b.tolist(), best.last_pos_a.tolist(), best.last_pos_b.tolist()) == ([20, 7, 3], [2, 7, 3], [30, 7, 4], [3, 7, 4])
    # min_support comes after the selection: a key whose best bin is too small goes, whatever its shared count
    assert best.shared.tolist() == [18, 1, 5]
    assert ab.select(min_support=2).rows().tolist() == [best.rows()[0].tolist(), best.rows()[2].tolist()]
    assert ab.select(min_support=3).rows().tolist() == [best.rows()[0].tolist()]
    assert len(ab.select(min_support=8)) == 0 and ab.select(min_support=8).info["keys"] == 3
    assert len(_allbins([]).select()) == 0
    with pytest.raises(ValueError):
        best.select()


def test_diagonal_ranges():
    ab = _allbins([(K1, ((1 << 32) + 100) // 16, 1, _v(100, 0), _v(100, 0)), (K1, ((1 << 32) - 5) // 16, 1, _v(0, 5), _v(0, 5)), (K3, 219 // 16, 1, _v(100, 119), _v(100, 119))])
    lo, hi = ab.diagonal()
    assert lo.dtype == np.int64 and lo.tolist() == [96, -16, 208] and hi.tolist() == [111, -1, 223]
    from hysortk_amd import PairDiagonals
    with pytest.raises(ValueError):
        PairDiagonals.from_rows(ab.rows(), all_bins=True).diagonal()


def test_combine_on_hand_made_rows():
    from hysortk_amd import PairDiagonals
    a = _allbins([(K1, 5, 3, _v(10, 1), _v(12, 3)), (K1, 9, 4, _v(20, 2), _v(30, 3)), (K3, 2, 2, _v(3, 3), _v(4, 4))], info=dict(records=11, self_records=2))
    b = _allbins([(K1, 5, 2, _v(9, 0), _v(11, 2)), (K1, 9, 1, _v(31, 4), _v(31, 4)), (K2, 4, 1, _v(7, 7), _v(7, 7))], info=dict(records=5, self_records=1))
    c = PairDiagonals.combine([a, b, _allbins([])])
    assert c.all_bins and c.diag_bin == 16 and c.info == dict(records=16, self_records=3, keys=3, bins=4)
    assert c.rows().tolist() == [[K1, 5, 5, 5, _v(9, 0), _v(12, 3)], [K1, 5, 9, 5, _v(20, 2), _v(31, 4)], [K2, 1, 4, 1, _v(7, 7), _v(7, 7)], [K3, 2, 2, 2, _v(3, 3), _v(4, 4)]]
    # a key split over two parts: neither part's best bin decides -- in a bin 9 leads (4 : 3), in b bin 5 (2 : 1); joined they tie at 5 and the smaller bin wins
    assert a.select().rows()[0].tolist() == [K1, 7, 9, 4, _v(20, 2), _v(30, 3)] and b.select().rows()[0].tolist() == [K1, 3, 5, 2, _v(9, 0), _v(11, 2)]
    best = c.select()
    assert best.rows().tolist() == [[K1, 10, 5, 5, _v(9, 0), _v(12, 3)], [K2, 1, 4, 1, _v(7, 7), _v(7, 7)], [K3, 2, 2, 2, _v(3, 3), _v(4, 4)]]
    assert c.select(min_support=2).rows().tolist() == [best.rows()[0].tolist(), best.rows()[2].tolist()]
    assert np.array_equal(PairDiagonals.combine([b, a]).rows(), c.rows())
    assert len(PairDiagonals.combine([])) == 0
    with pytest.raises(ValueError):                       # the best-bin lists themselves do not combine
        PairDiagonals.combine([a.select(), b.select()])
    with pytest.raises(ValueError):
        PairDiagonals.combine([a, _allbins([], diag_bin=7)])


def test_library_exports_the_diagonal_entry_points():
    from hysortk_amd import _lib
    lib = _lib.load()
    for name in ("hsk_result_pair_diagonals", "hsk_pair_diags_free"):
        assert hasattr(lib, name), "libhsk.so does not export " + name
        assert name in _lib.SYMBOLS


def test_pair_diags_struct_size_matches_header(tmp_path):
    from hysortk_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "hsk.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(hsk_pair_diags), offsetof(hsk_pair_diags, bins), '
           'offsetof(hsk_pair_diags, ms_expand), offsetof(hsk_pair_diags, reserved), offsetof(hsk_pair_diags, priv));return 0;}\n')
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(util.ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).decode().split()]
    assert out == [C.sizeof(_lib.PairDiags), _lib.PairDiags.bins.offset, _lib.PairDiags.ms_expand.offset, _lib.PairDiags.reserved.offset, _lib.PairDiags.priv.offset]


def test_bad_arguments_are_refused_without_a_gpu():
    from hysortk_amd import _lib
    lib = _lib.load()
    pd, res, st = _lib.PairDiags(), _lib.Result(), _lib.Strands()
    INVALID = 1                                           # HSK_ERR_INVALID_ARG
    assert lib.hsk_result_pair_diagonals(None, None, None, 0, 0, 16, 1, 0, 0, None) == INVALID
    assert lib.hsk_result_pair_diagonals(None, C.byref(res), C.byref(st), 0, 0, 16, 1, 0, 0, C.byref(pd)) == INVALID
    assert lib.hsk_result_pair_diagonals(None, C.byref(res), C.byref(st), 0, 0, 0, 1, 0, 0, C.byref(pd)) == INVALID          # diag_bin == 0
    assert lib.hsk_result_pair_diagonals(None, C.byref(res), C.byref(st), 0, 0, (1 << 31) + 1, 1, 0, 0, C.byref(pd)) == INVALID
    assert lib.hsk_result_pair_diagonals(None, C.byref(res), C.byref(st), 0, 0, 16, 0, 0, 0, C.byref(pd)) == INVALID         # min_support == 0
    lib.hsk_pair_diags_free(None, None)                   # (nothing to free: no effect)
    lib.hsk_pair_diags_free(None, C.byref(pd))
    assert pd.n == 0 and not pd.priv
