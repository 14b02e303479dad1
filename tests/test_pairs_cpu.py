"""The read-pair stage (hsk_result_pairs, include/hsk.h) without a GPU: the record-index decode of hysortk_amd/csrc/hsk_pairdecode.h on
the CPU under the address and undefined-behaviour sanitizers (tests/pairdecode_test.cpp), and the C ABI's new surface -- the exports,
the layout of hsk_pairs against its ctypes mirror, and the refusal of NULL arguments, which needs no device."""
import ctypes as C
import os
import subprocess

from tests import util


def test_pair_decode_is_exact_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pairdecode_test")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                           os.path.join(util.ROOT, "tests", "pairdecode_test.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0 and out.startswith("OK"), out


def test_library_exports_the_pair_entry_points():
    from hysortk_amd import _lib
    lib = _lib.load()
    for name in ("hsk_result_pairs", "hsk_pairs_free"):
        assert hasattr(lib, name), "libhsk.so does not export " + name
        assert name in _lib.SYMBOLS


def test_pairs_struct_size_matches_header(tmp_path):
    from hysortk_amd import _lib
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "hsk.h"\nint main(){printf("%zu %zu %zu\\n", sizeof(hsk_pairs), offsetof(hsk_pairs, ms_expand), offsetof(hsk_pairs, priv));return 0;}\n'
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(util.ROOT, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).decode().split()]
    assert out == [C.sizeof(_lib.Pairs), _lib.Pairs.ms_expand.offset, _lib.Pairs.priv.offset]


def test_null_arguments_are_refused_without_a_gpu():
    from hysortk_amd import _lib
    lib = _lib.load()
    pr, res = _lib.Pairs(), _lib.Result()
    assert lib.hsk_result_pairs(None, None, 0, 0, 1, 0, None) == 1            # HSK_ERR_INVALID_ARG
    assert lib.hsk_result_pairs(None, C.byref(res), 0, 0, 1, 0, C.byref(pr)) == 1
    lib.hsk_pairs_free(None, None)                                            # (nothing to free: no effect)
    lib.hsk_pairs_free(None, C.byref(pr))
    assert pr.n == 0 and not pr.priv
