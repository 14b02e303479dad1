"""hsk_pair_diags_merge (include/hsk.h): the several-list contract of the read pairs by diagonal on the GPU -- the merge kernel of
hysortk_amd/csrc/hsk_rowmerge.h on six-word rows and the two-word key (key, bin), and the selection behind it -- against PairDiagonals.combine(parts) and
.select(), the host code in numpy, on synthetic all-bins lists.  A list is ascending by (key, bin) with every (key, bin) at most once;
first and last are arbitrary 64-bit numbers (the minimum and maximum are held to the unsigned order everywhere).  All comparisons are exact:
rows, keys, bins, records, self_records."""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049, 4097, 20011]      # around the tile of the merge (512) and of the selection (1024), and many tiles
BIT63 = np.uint64(1) << np.uint64(63)
MERGE_TILE, SELECT_TILE = 512, 1024                      # hsk_rowmerge.h: DiagRow::TILE; hsk_pairdiag.h: DS_TILE


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


def _distinct(rng, n, nkeys=None, key_lo=0, key_hi=1 << 64, bin_hi=1 << 34):
    """n distinct (key, bin) in ascending order, [n, 2]: the keys from a pool of nkeys (default: about n / 3, several bins per key)."""
    if not n:
        return np.zeros((0, 2), np.uint64)
    pool = np.unique(_u64(rng, (nkeys or max(n // 3, 1)) + 8, key_lo, key_hi))
    kb = np.stack([rng.choice(pool, n + n // 8 + 16), _u64(rng, n + n // 8 + 16, 0, bin_hi)], axis=1)
    kb = np.unique(kb, axis=0)
    assert kb.shape[0] >= n
    return kb[np.sort(rng.choice(kb.shape[0], n, replace=False))]


def _ascending(kb):
    return bool(np.all((kb[1:, 0] > kb[:-1, 0]) | ((kb[1:, 0] == kb[:-1, 0]) & (kb[1:, 1] > kb[:-1, 1]))))


def _part(H, rng, kb, sup_hi=1 << 34, records=None, sup=None):
    kb = np.asarray(kb, dtype=np.uint64).reshape(-1, 2)
    assert _ascending(kb)
    n = kb.shape[0]
    s = _u64(rng, n, 1, sup_hi) if sup is None else np.asarray(sup, np.uint64)
    rows = np.stack([kb[:, 0], s, kb[:, 1], s, _u64(rng, n), _u64(rng, n)], axis=1) if n else np.zeros((0, 6), np.uint64)
    rec = int(rng.integers(0, 1 << 40)) if records is None else records
    return H.PairDiagonals.from_rows(rows, diag_bin=7, all_bins=True, info=dict(records=rec, self_records=rec // 3))


def _want(H, parts, min_support=1, all_bins=True):
    """The host code: the join, then the filter on the joined rows or the selection."""
    joined = H.PairDiagonals.combine(parts)
    if not all_bins:
        return joined.select(min_support=min_support)
    r = joined.rows()
    return H.PairDiagonals.from_rows(r[r[:, 3] >= np.uint64(min_support)], diag_bin=joined.diag_bin, all_bins=True, info=joined.info)


def _same(got, want, parts):
    assert len(got) == len(want) and got.all_bins == want.all_bins
    assert np.array_equal(got.rows(), want.rows())
    assert (got.info["keys"], got.info["bins"]) == (want.info["keys"], want.info["bins"])
    for k in ("records", "self_records"):
        assert got.info[k] == sum(p.info[k] for p in parts) == want.info[k], k


def _hold(H, ctx, parts, min_support=1, modes=(True, False)):
    for all_bins in modes:
        want = _want(H, parts, min_support, all_bins)
        got = H.PairDiagonals.combine(parts, ctx=ctx, all_bins=all_bins, min_support=min_support)
        _same(got, want, parts)
    return _want(H, parts, min_support, True)


def _split(rng, kb, na):
    """Distinct (key, bin) dealt to two lists at random: na to the first."""
    pick = np.zeros(kb.shape[0], bool)
    pick[rng.choice(kb.shape[0], na, replace=False)] = True
    return kb[pick], kb[~pick]


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------------------
def test_lists_that_share_no_row_interleave(H, ctx):
    """Every pair of sizes: the diagonal of every tile falls somewhere else in the two lists."""
    rng = np.random.default_rng(1)
    for na, nb in itertools.product(SIZES, SIZES):
        a, b = _split(rng, _distinct(rng, na + nb), na)
        want = _hold(H, ctx, [_part(H, rng, a), _part(H, rng, b)], modes=(True,))
        assert len(want) == na + nb == want.info["bins"]


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a_first", [True, False])
def test_one_list_below_the_other(H, ctx, a_first):
    """All of A below all of B, and the reverse; once by the key, once inside one key by the bin alone."""
    rng = np.random.default_rng(2)
    for na, nb in itertools.product(SIZES, [0, 1, 257, 512, 1025, 20011]):
        lo, hi = _distinct(rng, na, key_hi=1 << 62), _distinct(rng, nb, key_lo=1 << 62, key_hi=1 << 63)
        parts = [_part(H, rng, lo), _part(H, rng, hi)]
        _hold(H, ctx, parts if a_first else parts[::-1])
    for na, nb in ((513, 700), (1, 20011), (4097, 1)):
        bins = np.sort(rng.choice(1 << 20, na + nb, replace=False)).astype(np.uint64)
        kb = np.stack([np.full(na + nb, 77, np.uint64), bins], axis=1)
        parts = [_part(H, rng, kb[:na]), _part(H, rng, kb[na:])]
        _hold(H, ctx, parts if a_first else parts[::-1])


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------------------
def test_every_row_in_both_lists(H, ctx):
    """The same (key, bin) in both lists: every position pair of the merged sequence is one joined row, so A's copy is the last row of a
    tile's share and B's copy the first of the next at every tile boundary."""
    rng = np.random.default_rng(3)
    for n in SIZES:
        kb = _distinct(rng, n)
        want = _hold(H, ctx, [_part(H, rng, kb), _part(H, rng, kb)])
        assert len(want) == n == want.info["bins"] and want.info["keys"] == np.unique(kb[:, 0]).size


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------------------
def test_same_keys_and_disjoint_bins(H, ctx):
    """Both lists hold every key, and no (key, bin) twice: the order inside a key is decided by word two alone.  A compare on the key alone
    would call every such pair of rows a tie and put all of A's bins of a key in front of B's -- the precondition below is that this
    order is not the ascending one -- and would join rows that do not belong together."""
    rng = np.random.default_rng(4)
    for nkeys, nbins in ((1, 3000), (40, 100), (700, 6), (3000, 2)):
        keys = np.sort(np.unique(_u64(rng, nkeys + 8))[:nkeys])
        bins = np.stack([np.sort(rng.choice(1 << 33, nbins, replace=False)) for _ in range(nkeys)]).astype(np.uint64) + np.uint64((1 << 33) - (1 << 32))
        to_a = rng.random((nkeys, nbins)) < 0.5
        to_a[:, 0], to_a[:, 1] = False, True                # every key in both lists, and B's smallest bin below A's
        kk = np.repeat(keys, nbins).reshape(nkeys, nbins)
        a, b = np.stack([kk[to_a], bins[to_a]], axis=1), np.stack([kk[~to_a], bins[~to_a]], axis=1)
        assert np.array_equal(np.unique(a[:, 0]), keys) and np.array_equal(np.unique(b[:, 0]), keys)
        one_word = np.concatenate([a, b])[np.argsort(np.concatenate([a[:, 0], b[:, 0]]), kind="stable")]      # A's copy of a key first
        assert not _ascending(one_word)
        pa, pb = _part(H, rng, a), _part(H, rng, b)
        want = _hold(H, ctx, [pa, pb])
        assert len(want) == nkeys * nbins and want.info["keys"] == nkeys
        _hold(H, ctx, [pb, pa])


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------------------
def test_shared_rows_at_multiples_of_256(H, ctx):
    """The (key, bin) of both lists are exactly those at A's indices 0, 256, 512, ...; B holds others besides."""
    rng = np.random.default_rng(5)
    for na, extra in ((20011, 0), (20011, 5000), (4097, 4096), (1024, 1), (257, 20011)):
        a, other = _split(rng, _distinct(rng, na + extra), na)
        b = np.unique(np.concatenate([a[::256], other]), axis=0)
        want = _hold(H, ctx, [_part(H, rng, a), _part(H, rng, b)])
        assert len(want) == na + extra
        _hold(H, ctx, [_part(H, rng, b), _part(H, rng, a)])


# ---- 6 -----------------------------------------------------------------------------------------------------------------------------------------
def test_keys_are_unsigned_and_words_are_wide(H, ctx):
    """Keys with bit 63 set sort behind all others; supports whose sums pass 2^32; first and last with bit 63 set."""
    rng = np.random.default_rng(6)
    kb = np.concatenate([_distinct(rng, 3000, key_hi=1 << 20), _distinct(rng, 3000, key_lo=1 << 63, key_hi=(1 << 63) + (1 << 20)),
                         np.array([[(1 << 64) - 1, 0], [(1 << 64) - 1, (1 << 33) - 1]], np.uint64)])
    a, b = kb[rng.random(kb.shape[0]) < 0.7], kb[rng.random(kb.shape[0]) < 0.7]
    pa, pb = _part(H, rng, a, sup_hi=1 << 62), _part(H, rng, b, sup_hi=1 << 62)
    want = _hold(H, ctx, [pa, pb])
    assert int((want.key & BIT63 != 0).sum()) > 2000 and len(want) < a.shape[0] + b.shape[0] and int(want.support.max()) > 1 << 62
    joined = np.flatnonzero(np.isin(want.key, pa.key) & np.isin(want.key, pb.key))
    assert joined.size > 1000


# ---- 7 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nparts", [1, 2, 3, 5, 9])
def test_a_chain_of_parts(H, ctx, nparts):
    """Parts of unequal sizes over one universe of (key, bin), empty ones among them: the binary-counter order of the merges, lists that move
    up unmerged, and the counts of the last merge."""
    rng = np.random.default_rng(70 + nparts)
    universe = _distinct(rng, 9000, nkeys=1500)
    sizes = [7000, 0, 2049, 1, 4096, 0, 300, 5555, 513][:nparts] if nparts > 1 else [3000]
    parts = [_part(H, rng, universe[np.sort(rng.choice(9000, n, replace=False))], sup_hi=5) for n in sizes]
    want = _hold(H, ctx, parts)
    assert want.info["bins"] == len(want) > want.info["keys"] > 0
    _hold(H, ctx, parts[::-1])


# ---- 8 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_support", [2, 5])
@pytest.mark.parametrize("nparts", [1, 3])
def test_min_support_is_applied_after_the_join(H, ctx, min_support, nparts):
    rng = np.random.default_rng(80 + min_support + nparts)
    universe = _distinct(rng, 6000, nkeys=4000)
    parts = [_part(H, rng, universe[np.sort(rng.choice(6000, n, replace=False))], sup_hi=7) for n in (4500, 3000, 1025)[:nparts]]
    for all_bins in (True, False):
        want = _want(H, parts, min_support, all_bins)
        unfiltered = _want(H, parts, 1, all_bins)
        assert 0 < len(want) < len(unfiltered)
        if nparts > 1:                                       # rows that pass only because they were joined first
            alone = np.concatenate([p.rows()[p.support >= np.uint64(min_support)] for p in parts])
            assert len(_want(H, parts, min_support, True)) > np.unique(alone[:, [0, 2]], axis=0).shape[0]
    _hold(H, ctx, parts, min_support=min_support)


# ---- 9 -----------------------------------------------------------------------------------------------------------------------------------------
def test_selection_of_the_joined_list(H, ctx):
    """all_bins=False is the host select() of the host join.  One key has 5000 bin rows -- several tiles of the merge and of the selection --
    and its largest support, 100, is reached three times: by a bin of the first part alone, by a bin of the second part alone, far behind
    it, and between them by a bin that only the join brings there (60 + 40).  The smallest of the three bins wins."""
    rng = np.random.default_rng(9)
    big, nb = np.uint64(1 << 40), 5000
    bins = np.sort(rng.choice(1 << 33, nb, replace=False)).astype(np.uint64)
    to_a = rng.random(nb) < 0.5
    i_a, i_j, i_b = 300, 2600, 4700
    to_a[i_a], to_a[i_b] = True, False
    sup = rng.integers(1, 30, nb).astype(np.uint64)
    sup[i_a] = sup[i_b] = 100
    ka = np.stack([np.full(int(to_a.sum()), big), bins[to_a]], axis=1)
    kb = np.stack([np.full(int((~to_a).sum()), big), bins[~to_a]], axis=1)
    sa, sb = sup[to_a], sup[~to_a]
    # the joined bin: in both parts
    if to_a[i_j]:
        kb = np.concatenate([kb, np.array([[big, bins[i_j]]], np.uint64)]); sb = np.concatenate([sb, np.array([40], np.uint64)]); sa[np.flatnonzero(ka[:, 1] == bins[i_j])] = 60
        o = np.argsort(kb[:, 1]); kb, sb = kb[o], sb[o]
    else:
        ka = np.concatenate([ka, np.array([[big, bins[i_j]]], np.uint64)]); sa = np.concatenate([sa, np.array([60], np.uint64)]); sb[np.flatnonzero(kb[:, 1] == bins[i_j])] = 40
        o = np.argsort(ka[:, 1]); ka, sa = ka[o], sa[o]
    # other keys around it, below and above, shared and not
    other = _distinct(rng, 3000, nkeys=900)
    other = other[other[:, 0] != big]
    oa, ob = other[rng.random(other.shape[0]) < 0.6], other[rng.random(other.shape[0]) < 0.6]

    def whole(own, own_sup, more):
        kk = np.concatenate([own, more]); ss = np.concatenate([own_sup, rng.integers(1, 5, more.shape[0]).astype(np.uint64)])
        o = np.lexsort((kk[:, 1], kk[:, 0]))
        return _part(H, rng, kk[o], sup=ss[o])

    pa, pb = whole(ka, sa, oa), whole(kb, sb, ob)
    joined = H.PairDiagonals.combine([pa, pb])
    at = np.flatnonzero((joined.key == big) & (joined.support == np.uint64(100)))
    run = np.flatnonzero(joined.key == big)
    assert run.size == nb and int(joined.support[run].max()) == 100 and at.size == 3
    assert at[0] // MERGE_TILE != at[1] // MERGE_TILE != at[2] // MERGE_TILE and at[0] // SELECT_TILE != at[2] // SELECT_TILE
    best = joined.select()
    row = best.rows()[best.key == big][0]
    assert int(row[2]) == int(bins[i_a]) and int(row[3]) == 100 and int(row[1]) == int(joined.support[run].sum())
    for ms in (1, 3, 101):
        for parts in ([pa, pb], [pb, pa]):
            _hold(H, ctx, parts, min_support=ms)
    # one list: the device-side select()
    got = joined.select(min_support=3, ctx=ctx)
    assert np.array_equal(got.rows(), joined.select(min_support=3).rows()) and got.info["keys"] == joined.info["keys"] and not got.all_bins


# ---- 10 ----------------------------------------------------------------------------------------------------------------------------------------
def test_host_and_device_parts(H, ctx):
    """Parts whose rows are in HBM are read where they are (and stay intact); the result on the device equals the one on the host."""
    rng = np.random.default_rng(10)
    universe = _distinct(rng, 12000, nkeys=2000)
    host = [_part(H, rng, universe[np.sort(rng.choice(12000, n, replace=False))], sup_hi=4) for n in (4097, 9000, 255)]
    dev = [H.PairDiagonals.combine([p], ctx=ctx, on_device=True) for p in host]
    try:
        for d, p in zip(dev, host):
            assert d.n == len(p) and d.rows_dev and d.rows_dev % 16 == 0 and d.info["records"] == p.info["records"] and d.all_bins
        for ms, all_bins in ((1, True), (3, True), (1, False), (3, False)):
            for mix in (dev, [dev[0], host[1], dev[2]], [host[0], dev[1], host[2]], dev[:1], dev[:2]):
                ref = _want(H, host[:len(mix)], ms, all_bins)
                _same(H.PairDiagonals.combine(mix, ctx=ctx, all_bins=all_bins, min_support=ms), ref, host[:len(mix)])
                with H.PairDiagonals.combine(mix, ctx=ctx, all_bins=all_bins, min_support=ms, on_device=True) as out:
                    assert out.n == len(ref) and out.info["keys"] == ref.info["keys"] and out.info["bins"] == ref.info["bins"]
                    assert out.rows_dev not in [d.rows_dev for d in dev]
                    assert np.array_equal(ctx.d2h(out.rows_dev, out.n * 48).view(np.uint64).reshape(out.n, 6), ref.rows())
        for d, p in zip(dev, host):                      # the parts are left as they were
            assert np.array_equal(ctx.d2h(d.rows_dev, d.n * 48).view(np.uint64).reshape(d.n, 6), p.rows())
    finally:
        for d in dev:
            d.close()


def test_no_parts_and_empty_parts(H, ctx):
    rng = np.random.default_rng(12)
    for parts in ([], [_part(H, rng, [], records=5)], [_part(H, rng, [], records=5), _part(H, rng, [], records=9)]):
        for all_bins in (True, False):
            got = H.PairDiagonals.combine(parts, ctx=ctx, all_bins=all_bins, min_support=2)
            assert len(got) == 0 and got.rows().shape == (0, 6) and got.info["keys"] == 0 and got.info["bins"] == 0
            assert got.info["records"] == sum(p.info["records"] for p in parts) and got.info["self_records"] == sum(p.info["self_records"] for p in parts)
        with H.PairDiagonals.combine(parts, ctx=ctx, on_device=True) as d:
            assert d.n == 0 and not d.rows_dev


# ---- 11 ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["joined", "parts"])
def test_no_write_past_a_block(H, case):
    """Red zones behind every device block: the call fails if a merge or the selection writes past one."""
    rng = np.random.default_rng(11)
    with H.Context(K=31, M=17, L=2, U=50, tuning={"pool_redzone": 256}) as c:
        if case == "joined":
            kb = _distinct(rng, 20011)
            parts = [_part(H, rng, kb, sup_hi=4), _part(H, rng, kb, sup_hi=4)]
        else:
            universe = _distinct(rng, 9000, nkeys=1200)
            parts = [_part(H, rng, universe[np.sort(rng.choice(9000, n, replace=False))], sup_hi=3) for n in (4097, 0, 2048, 1, 6000)]
        for ms in (1, 3):
            _hold(H, c, parts, min_support=ms)


# ---- 12 ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(H, ctx):
    from hysortk_amd import _lib
    rng = np.random.default_rng(13)
    good = _part(H, rng, _distinct(rng, 300))
    rows = np.ascontiguousarray(good.rows())
    ok = _lib.PairDiags(); ok.n = 300; ok.rows = rows.ctypes.data_as(C.POINTER(C.c_uint64))
    norows = _lib.PairDiags(); norows.n = 5
    out = _lib.PairDiags()
    P = C.POINTER(_lib.PairDiags)
    one = (P * 1)(C.pointer(ok))
    merge = ctx.lib.hsk_pair_diags_merge

    def works():
        assert merge(ctx.h, one, 1, 1, 1, 0, C.byref(out)) == 0 and out.n == 300 and out.bins == 300
        assert np.array_equal(np.ctypeslib.as_array(out.rows, shape=(1800,)).reshape(300, 6), rows)
        ctx.lib.hsk_pair_diags_free(ctx.h, C.byref(out))

    assert merge(ctx.h, one, 1, 1, 1, 0, None) == 1                                   # no result struct
    assert merge(None, one, 1, 1, 1, 0, C.byref(out)) == 1                            # no context
    for args in ((None, 1, 1), (one, -1, 1), (one, 1, 0),                             # parts announced and none given; nparts < 0; min_support == 0
                 ((P * 2)(C.pointer(ok), P()), 2, 1), ((P * 2)(C.pointer(ok), C.pointer(norows)), 2, 1)):      # a NULL part; rows announced and none given
        assert merge(ctx.h, args[0], args[1], args[2], 1, 0, C.byref(out)) == 1
        assert ctx.lib.hsk_last_error(ctx.h)
        assert out.n == 0 and not out.rows and not out.rows_dev and not out.priv
        works()
    with H.PairDiagonals.combine([good], ctx=ctx, on_device=True) as d:               # a device list that is not 16-byte aligned
        odd = _lib.PairDiags(); odd.n = 10; odd.rows_dev = d.rows_dev + 8
        assert merge(ctx.h, (P * 1)(C.pointer(odd)), 1, 1, 1, 0, C.byref(out)) == 1 and b"aligned" in ctx.lib.hsk_last_error(ctx.h)
        works()
    with pytest.raises(H.HskError) as e:
        H.PairDiagonals.combine([good], min_support=0, ctx=ctx)
    assert e.value.status == 1
    assert merge(ctx.h, None, 0, 1, 0, 0, C.byref(out)) == 0 and out.n == 0           # no parts: an empty list
    ctx.lib.hsk_pair_diags_free(ctx.h, C.byref(out))
    with pytest.raises(ValueError):                                                   # best-bin lists do not combine, on the device either
        H.PairDiagonals.combine([good.select()], ctx=ctx)
    with pytest.raises(ValueError):
        good.select().select(ctx=ctx)
    _hold(H, ctx, [good, _part(H, rng, _distinct(rng, 5000))])
