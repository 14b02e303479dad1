"""hsk_pairs_merge (include/hsk.h): the several-list contract of the read pairs on the GPU -- the merge kernel of
hysortk_amd/csrc/hsk_rowmerge.h on four-word rows -- against ReadPairs.combine(parts), the host code in numpy, on synthetic row lists.  A list is ascending
by key with every key at most once; the words behind the key are arbitrary 64-bit numbers here (first and last use all 64 bits throughout,
so the minimum and maximum are held to the unsigned order everywhere).  All comparisons are exact: rows, keys, records, self_records."""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# around the tile the kernel has (hsk_rowmerge.h: PairRow::TILE = 1024; 0 + 1024 and 1 + 1023 are one full tile with no look-ahead), around
# every other tile size it may have (2^8 .. 2^12), and many tiles
SIZES = [0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 20011]
BIT63 = np.uint64(1) << np.uint64(63)


@pytest.fixture(scope="module")
def H():
    import hysortk_amd
    return hysortk_amd


@pytest.fixture(scope="module")
def ctx(H):
    with H.Context(K=31, M=17, L=2, U=50) as c:           # (neither EXTENSION nor a resident result)
        yield c


def _u64(rng, n, lo=0, hi=1 << 64):
    return rng.integers(lo, hi, size=n, dtype=np.uint64, endpoint=False) if n else np.zeros(0, np.uint64)


def _distinct(rng, n, lo=0, hi=1 << 64):
    """n distinct keys in [lo, hi), ascending."""
    k = np.unique(_u64(rng, n + n // 8 + 16, lo, hi))
    assert k.size >= n
    return np.sort(rng.choice(k, n, replace=False)) if n else np.zeros(0, np.uint64)


def _part(H, rng, keys, shared_hi=1 << 34, records=None):
    keys = np.asarray(keys, dtype=np.uint64)
    assert np.all(keys[1:] > keys[:-1])
    n = keys.size
    rows = np.stack([keys, _u64(rng, n, 1, shared_hi), _u64(rng, n), _u64(rng, n)], axis=1) if n else np.zeros((0, 4), np.uint64)
    rec = int(rng.integers(0, 1 << 40)) if records is None else records
    return H.ReadPairs.from_rows(rows, info=dict(records=rec, self_records=rec // 3))


def _same(got, want, parts):
    assert len(got) == len(want)
    assert np.array_equal(got.rows(), want.rows())
    assert got.info["keys"] == want.info.get("keys", 0)      # (the host code gives a list of empty parts no info)
    for k in ("records", "self_records"):
        assert got.info[k] == sum(p.info[k] for p in parts), k
        assert got.info[k] == want.info.get(k, got.info[k]), k


def _hold(H, ctx, parts, min_shared=1):
    want = H.ReadPairs.combine(parts, min_shared=min_shared)
    got = H.ReadPairs.combine(parts, min_shared=min_shared, ctx=ctx)
    _same(got, want, parts)
    return want


def _split(rng, keys, na):
    """Distinct keys dealt to two lists at random: na to the first."""
    pick = np.zeros(keys.size, bool)
    pick[rng.choice(keys.size, na, replace=False)] = True
    return keys[pick], keys[~pick]


def test_lists_that_share_no_key_interleave(H, ctx):
    """Every pair of sizes: the diagonal of every tile falls somewhere else in the two lists."""
    rng = np.random.default_rng(1)
    for na, nb in itertools.product(SIZES, SIZES):
        a, b = _split(rng, _distinct(rng, na + nb), na)
        want = _hold(H, ctx, [_part(H, rng, a), _part(H, rng, b)])
        assert len(want) == na + nb


@pytest.mark.parametrize("a_first", [True, False])
def test_one_list_below_the_other(H, ctx, a_first):
    """All of A below all of B, and the reverse: tiles that take rows of one list only, and the one tile that changes over."""
    rng = np.random.default_rng(2)
    for na, nb in itertools.product(SIZES, [0, 1, 257, 2048, 4097, 20011]):
        lo, hi = _distinct(rng, na, 0, 1 << 62), _distinct(rng, nb, 1 << 62, 1 << 63)
        parts = [_part(H, rng, lo), _part(H, rng, hi)]
        _hold(H, ctx, parts if a_first else parts[::-1])


def test_every_key_in_both_lists(H, ctx):
    """The same keys in both lists: every position pair of the merged sequence is one joined row, so A's copy is the last row of a tile's
    share and B's copy the first of the next at every tile boundary, whatever power of two the tile is."""
    rng = np.random.default_rng(3)
    for n in SIZES:
        k = _distinct(rng, n)
        want = _hold(H, ctx, [_part(H, rng, k), _part(H, rng, k)])
        assert len(want) == n and want.info.get("keys", 0) == n


def test_shared_keys_at_multiples_of_256(H, ctx):
    """The keys of both lists are exactly those at A's indices 0, 256, 512, ...; B holds other keys besides."""
    rng = np.random.default_rng(4)
    for na, extra in ((20011, 0), (20011, 5000), (4097, 4096), (4096, 1), (257, 20011)):
        k = _distinct(rng, na + extra)
        a, other = _split(rng, k, na)
        b = np.sort(np.concatenate([a[::256], other]))
        want = _hold(H, ctx, [_part(H, rng, a), _part(H, rng, b)])
        assert len(want) == na + extra
        _hold(H, ctx, [_part(H, rng, b), _part(H, rng, a)])


def test_keys_are_unsigned(H, ctx):
    """Keys with bit 63 set sort behind all others; half of them are in both lists."""
    rng = np.random.default_rng(5)
    k = np.concatenate([_distinct(rng, 3000, 0, 1 << 20), _distinct(rng, 3000, (1 << 63), (1 << 63) + (1 << 20)), np.array([(1 << 64) - 1], np.uint64)])
    a = k[rng.random(k.size) < 0.7]
    b = k[rng.random(k.size) < 0.7]
    want = _hold(H, ctx, [_part(H, rng, a), _part(H, rng, b)])
    assert int((want.key & BIT63 != 0).sum()) > 2000 and np.all(want.key[1:] > want.key[:-1]) and len(want) < a.size + b.size


def test_wide_words(H, ctx):
    """shared sums above 2^32 (64-bit sums), first and last with bit 63 set (unsigned minimum and maximum)."""
    rng = np.random.default_rng(6)
    k = _distinct(rng, 5000)
    pa, pb = _part(H, rng, k, shared_hi=1 << 62), _part(H, rng, k[::2], shared_hi=1 << 62)
    want = _hold(H, ctx, [pa, pb])
    assert int(want.shared.max()) > 1 << 62 and int((want.shared > np.uint64(1 << 32)).sum()) > 4000
    joined = want.first[::2] != pa.first[::2]            # rows whose minimum came from the second list
    assert 500 < int(joined.sum()) < 2000
    assert int(((pa.first[::2] & BIT63 != 0) & (pb.first & BIT63 == 0) & joined).sum()) > 100      # a signed minimum would have kept the first list's word


@pytest.mark.parametrize("nparts", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("min_shared", [1, 3])
def test_several_parts(H, ctx, nparts, min_shared):
    """Parts of unequal sizes over one universe of keys, empty ones among them; min_shared is applied to the joined rows and `keys` counts the
    rows before it."""
    rng = np.random.default_rng(10 * nparts + min_shared)
    universe = _distinct(rng, 9000)
    sizes = [7000, 0, 2049, 1, 4096, 0, 300, 5555][:nparts] if nparts > 1 else [3000]
    parts = [_part(H, rng, np.sort(rng.choice(universe, n, replace=False)), shared_hi=5) for n in sizes]
    want = _hold(H, ctx, parts, min_shared=min_shared)
    assert want.info["keys"] >= len(want) > 0
    if min_shared == 3:
        assert want.info["keys"] > len(want)
    _hold(H, ctx, parts[::-1], min_shared=min_shared)


def test_no_parts_and_empty_parts(H, ctx):
    rng = np.random.default_rng(7)
    for parts in ([], [_part(H, rng, [], records=5)], [_part(H, rng, [], records=5), _part(H, rng, [], records=9)]):
        assert len(H.ReadPairs.combine(parts, min_shared=2)) == 0
        got = H.ReadPairs.combine(parts, min_shared=2, ctx=ctx)
        assert len(got) == 0 and got.rows().shape == (0, 4) and got.info["keys"] == 0
        assert got.info["records"] == sum(p.info["records"] for p in parts) and got.info["self_records"] == sum(p.info["self_records"] for p in parts)
        with H.ReadPairs.combine(parts, ctx=ctx, on_device=True) as d:
            assert d.n == 0 and not d.rows_dev


def test_host_and_device_parts(H, ctx):
    """Parts whose rows are in HBM are read where they are (and stay intact); the result on the device equals the one on the host."""
    rng = np.random.default_rng(8)
    universe = _distinct(rng, 12000)
    host = [_part(H, rng, np.sort(rng.choice(universe, n, replace=False)), shared_hi=4) for n in (4097, 9000, 255)]
    dev = [H.ReadPairs.combine([p], ctx=ctx, on_device=True) for p in host]
    try:
        for d, p in zip(dev, host):
            assert d.n == len(p) and d.rows_dev and d.info["records"] == p.info["records"]
        for ms in (1, 3):
            want = H.ReadPairs.combine(host, min_shared=ms)
            for mix in (dev, [dev[0], host[1], dev[2]], [host[0], dev[1], host[2]], dev[:1], dev[:2]):
                ref = want if len(mix) == 3 else H.ReadPairs.combine(host[:len(mix)], min_shared=ms)
                _same(H.ReadPairs.combine(mix, min_shared=ms, ctx=ctx), ref, host[:len(mix)])
                with H.ReadPairs.combine(mix, min_shared=ms, ctx=ctx, on_device=True) as out:
                    assert out.n == len(ref) and out.info["keys"] == ref.info["keys"]
                    assert out.rows_dev not in [d.rows_dev for d in dev]
                    rows = ctx.d2h(out.rows_dev, out.n * 32).view(np.uint64).reshape(out.n, 4)
                    assert np.array_equal(rows, ref.rows())
        for d, p in zip(dev, host):                      # the parts are left as they were
            assert np.array_equal(ctx.d2h(d.rows_dev, d.n * 32).view(np.uint64).reshape(d.n, 4), p.rows())
    finally:
        for d in dev:
            d.close()


@pytest.mark.parametrize("case", ["joined", "parts"])
def test_no_write_past_a_block(H, case):
    """Red zones behind every device block: the call fails if a merge writes past one."""
    rng = np.random.default_rng(9)
    with H.Context(K=31, M=17, L=2, U=50, tuning={"pool_redzone": 256}) as c:
        if case == "joined":
            k = _distinct(rng, 20011)
            parts = [_part(H, rng, k), _part(H, rng, k)]
        else:
            universe = _distinct(rng, 9000)
            parts = [_part(H, rng, np.sort(rng.choice(universe, n, replace=False)), shared_hi=3) for n in (4097, 0, 2048, 1, 6000)]
        for ms in (1, 3):
            _hold(H, c, parts, min_shared=ms)


def test_refusals(H, ctx):
    from hysortk_amd import _lib
    rng = np.random.default_rng(11)
    good = _part(H, rng, _distinct(rng, 300))
    rows = np.ascontiguousarray(good.rows())
    ok = _lib.Pairs(); ok.n = 300; ok.rows = rows.ctypes.data_as(C.POINTER(C.c_uint64))
    norows = _lib.Pairs(); norows.n = 5
    out = _lib.Pairs()
    P = C.POINTER(_lib.Pairs)
    one = (P * 1)(C.pointer(ok))
    merge = ctx.lib.hsk_pairs_merge
    assert merge(ctx.h, one, 1, 1, 0, None) == 1                                   # no result struct
    assert merge(None, one, 1, 1, 0, C.byref(out)) == 1                            # no context
    assert merge(ctx.h, None, 1, 1, 0, C.byref(out)) == 1                          # parts announced, none given
    assert merge(ctx.h, one, -1, 1, 0, C.byref(out)) == 1
    assert merge(ctx.h, one, 1, 0, 0, C.byref(out)) == 1                           # min_shared == 0
    assert merge(ctx.h, (P * 2)(C.pointer(ok), P()), 2, 1, 0, C.byref(out)) == 1   # a NULL part
    assert merge(ctx.h, (P * 2)(C.pointer(ok), C.pointer(norows)), 2, 1, 0, C.byref(out)) == 1
    assert ctx.lib.hsk_last_error(ctx.h)
    assert out.n == 0 and not out.rows and not out.rows_dev and not out.priv
    with pytest.raises(H.HskError) as e:
        H.ReadPairs.combine([good], min_shared=0, ctx=ctx)
    assert e.value.status == 1
    assert merge(ctx.h, None, 0, 1, 0, C.byref(out)) == 0 and out.n == 0           # no parts: an empty list
    ctx.lib.hsk_pairs_free(ctx.h, C.byref(out))
    assert merge(ctx.h, one, 1, 1, 0, C.byref(out)) == 0 and out.n == 300          # the context works afterwards
    assert np.array_equal(np.ctypeslib.as_array(out.rows, shape=(1200,)).reshape(300, 4), rows)
    ctx.lib.hsk_pairs_free(ctx.h, C.byref(out))
    other = _part(H, rng, _distinct(rng, 5000))
    _hold(H, ctx, [good, other])
