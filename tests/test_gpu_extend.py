"""hsk_pair_diags_extend (include/hsk.h): the seed of every diagonal row extended in both directions, ungapped, with an x-drop stop, over the
reads in HBM -- against the definition applied base by base (tests/extend_ref.py, itself held to hand-written overlaps by
tests/test_extend_ref.py).  Everything is integer work and compared word for word.  The rows of most cases are filled in by hand: the call
needs neither EXTENSION nor a resident result.  Every case runs through both device paths (wave_span 1: a wavefront per row;
0xFFFFFFFF: a lane per row; 0: the library's choice) and must give the same rows."""
import ctypes as C

import numpy as np
import pytest

from tests import extend_ref as X
from tests.test_extend_ref import random_case

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def H():
    import hysortk_amd
    return hysortk_amd


def _extend(H, c, rows, dna, rid_base=0, **kw):
    return H.PairDiagonals.from_rows(rows).extend(c, dna, rid_base=rid_base, **kw)


def _both_paths(H, c, rows, dna, want, columns, rid_base=0, **kw):
    """wave_span 1, none and the default: the same rows word for word; wave_rows is n, 0 and anything."""
    n = np.asarray(rows).reshape(-1, 6).shape[0]
    for span in (1, NONE, 0):
        ov = _extend(H, c, rows, dna, rid_base=rid_base, wave_span=span, **kw)
        got = ov.rows()
        print("wave_span %d: %d rows (reference %d), columns %d (%d), wave_rows %d, dropped %d, %.3f ms" % (span, len(ov), want.shape[0], ov.info["columns"], columns, ov.info["wave_rows"], ov.info["dropped"],
                                                                                                           ov.info["ms_extend"]))
        bad = np.flatnonzero((got != want).any(axis=1)) if got.shape == want.shape else None
        assert got.shape == want.shape and bad.size == 0, "wave_span %d: row %s is %s, the reference has %s" % (span, bad[:1], got[bad[:1]].tolist(), want[bad[:1]].tolist())
        assert ov.info["input_rows"] == n and ov.info["dropped"] == n - want.shape[0] and ov.info["columns"] == columns
        assert ov.info["wave_rows"] == (n if span == 1 else 0) or span == 0
    return ov


def _fetch(c, ov):
    """the rows of a list that was left in HBM"""
    return c.d2h(ov.rows_dev, len(ov) * 48).view(np.uint64).reshape(len(ov), 6)


def _mut(s, positions):
    s = list(s)
    for p in positions:
        s[p] = "ACGT"[("ACGT".index(s[p]) + 1) % 4]
    return "".join(s)


# ---- 1. geometry by hand -------------------------------------------------------------------------------------------------------------------
def _hand_cases(K):
    """(reads, rows): every case is two reads cut from one genome -- A = g[sa : sa + la), B = g[sb : sb + lb) or its reverse complement, the
    seed at genome position gs, A with substitutions at the genome positions `mut` -- and one row by hand."""
    rng = np.random.default_rng(100 + K)
    g = "".join(rng.choice(list("ACGT"), 600))
    reads, rows = [], []

    def add(sa, la, sb, lb, gs, o, mut=(), n_at=None, b_is_a=False):
        a = _mut(g[sa:sa + la], [p - sa for p in mut])
        if n_at is not None:
            assert a[n_at - sa] == "A"
            a = a[:n_at - sa] + "N" + a[n_at - sa + 1:]
        bf = a if b_is_a else g[sb:sb + lb]
        b = X.revcomp(bf) if o else bf
        pa, pb = gs - sa, (lb - (gs - sb) - K if o else gs - sb)
        rows.append(X.diag_row(len(reads), len(reads) + 1, o, pa, pb, support=len(rows) + 1))
        reads.extend([a, b])

    for o in (0, 1):
        add(200, K + 50, 150, 199, 200, o)                          # the seed at A's start
        add(200, K + 50, 150, 199, 250, o)                          # ... at A's end
        add(200, K, 150, 199, 200, o)                               # ... both: A is the seed
        add(150, 199, 200, K, 200, o)                               # B is the seed
        add(150, 199, 200, 131, 200, o)                             # the seed at B's forward start (o = 1: pb at B's end)
        add(150, 199, 130, 70 + K, 200, o)                          # the seed at B's forward end (o = 1: pb = 0)
        add(100, 197, 90, 199, 170, o, mut=[169])                   # a mismatch in the column next to the seed, left
        add(100, 197, 90, 199, 170, o, mut=[170 + K])               # ... right
        add(100, 197, 90, 199, 170, o, mut=[169, 170 + K])          # ... both
        for d in (31, 32, 33):                                      # mismatches 31, 32, 33 columns from the seed, either side
            add(100, 198, 110, 193, 170, o, mut=[170 + K + d])
            add(100, 198, 110, 193, 170, o, mut=[169 - d])
        add(100, 198, 110, 193, 170, o, mut=[170 + K + 31, 170 + K + 32, 170 + K + 33, 169 - 31, 169 - 32, 169 - 33])
        add(100, 198, 110, 193, 170, o, mut=[170 + K + 10, 170 + K + 11, 170 + K + 12])                  # a burst of 3: under xdrop 3 it drops exactly xdrop
        add(100, 198, 110, 193, 170, o, mut=[170 + K + 10, 170 + K + 11, 170 + K + 12, 170 + K + 13])    # ... of 4: xdrop + 1
        add(100, 198, 110, 193, 170, o, mut=[160, 161, 162])
        add(100, 198, 110, 193, 170, o, mut=[159, 160, 161, 162])
        n_at = g.index("A", 170 + K + 5)
        add(100, 198, 110, 193, 170, o, n_at=n_at)                  # an N against an A: a match
        add(100, 198, 110, 193, 170, o, n_at=g.index("A", 170))         # ... inside the seed
        add(100, 199, 100, 199, 110, o, b_is_a=True)                # identical reads
        add(100, 31 + K, 100, 31 + K, 100 + 31, o, b_is_a=True, mut=[105])
    lens = sorted({len(r) for r in reads})
    assert lens[0] == K and lens[-1] <= 200 and any(n % 4 for n in lens)
    return reads, np.array(rows, dtype=np.uint64)


@pytest.mark.parametrize("K", [31, 51])
def test_hand_geometry(H, K):
    reads, rows = _hand_cases(K)
    dna = H.DnaBuffer.from_sequences(reads)
    with H.Context(K=K) as c:
        for m, mm, xd in ((1, 1, 7), (1, 1, 3), (1, 1, 2), (2, 3, 0), (4, 0, 0), (1 << 15, 1 << 15, (1 << 31) - 1)):
            want, columns = X.extend_rows(rows, reads, K, match=m, mismatch=mm, xdrop=xd)
            ov = _both_paths(H, c, rows, dna, want, columns, match=m, mismatch=mm, xdrop=xd)
            assert np.array_equal(ov.support, rows[:, 3]) and np.array_equal(ov.key, rows[:, 0])
        # what the construction says, without the reference: under xdrop 3 a burst of 3 is crossed and a burst of 4 ends the side
        ov = _extend(H, c, rows, dna, match=1, mismatch=1, xdrop=3)
        per = rows.shape[0] // 2
        for o in (0, 1):
            b3, b4 = o * per + 16, o * per + 17
            assert ov.a_hi[b3] == 198 and ov.mismatches[b3] == 3 and ov.a_hi[b4] == 70 + K + 10 and ov.mismatches[b4] == 0, (ov.rows()[b3].tolist(), ov.rows()[b4].tolist())
            ident = o * per + 22
            assert ov.a_lo[ident] == 0 and ov.a_hi[ident] == 199 and ov.ends[ident] == 15 and ov.kind()[ident] == H.Overlaps.A_CONTAINED and ov.score[ident] == 199
        assert np.array_equal(ov.opposite, np.repeat([False, True], per))


# ---- 2. the bulk comparison ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bulk():
    rng = np.random.default_rng(2024)
    reads, rows = random_case(rng, 2000, 20000, 31, 31, 400, genome=5000, err=0.03)
    return reads, rows, X.code_matrix(reads)


def test_random_rows(H, bulk):
    reads, rows, mat = bulk
    assert rows.shape[0] == 20000 and len(reads) == 2000
    dna = H.DnaBuffer.from_sequences(reads)
    with H.Context(K=31) as c:
        for m, mm, xd in ((1, 1, 7), (2, 3, 5)):
            want, columns = X.extend_rows_bulk(rows, mat, 31, match=m, mismatch=mm, xdrop=xd)
            ov = _both_paths(H, c, rows, dna, want, columns, match=m, mismatch=mm, xdrop=xd)
        assert int(ov.mismatches.sum()) > 1000 and len(set(ov.kind().tolist())) == 4
        # the filter: the survivors are the reference's, in order
        med = int(np.median(want[:, 1]))
        want, columns = X.extend_rows_bulk(rows, mat, 31, match=2, mismatch=3, xdrop=5, min_score=med, min_length=60)
        assert 1000 < want.shape[0] < 19000
        _both_paths(H, c, rows, dna, want, columns, match=2, mismatch=3, xdrop=5, min_score=med, min_length=60)
        # a filter that drops everything, and an empty list
        ov = _extend(H, c, rows, dna, min_score=1 << 40)
        assert len(ov) == 0 and ov.info["dropped"] == 20000 and ov.rows().shape == (0, 6)
        ov = _extend(H, c, np.zeros((0, 6), np.uint64), dna)
        assert len(ov) == 0 and ov.info == dict(ov.info, input_rows=0, dropped=0, columns=0, wave_rows=0)


# ---- 3. long rows ----------------------------------------------------------------------------------------------------------------------------
def test_long_rows_through_the_wave_path(H):
    """Two reads of 70 000 bases and their reverse complements.  A step of the wave path is 2048 columns: single differences at walk
    positions 2047, 2048 and 2049 of either side, and on the right a burst from position 4090 on that crosses xdrop 7 at 4097, in the first
    window of the third step; the left side runs clean to the read's start.  A pair of identical reads runs clean to both ends."""
    K, L, gs = 31, 70000, 35003
    rng = np.random.default_rng(70)
    r0 = "".join(rng.choice(list("ACGT"), L))
    right = [gs + K + p for p in (2047, 2048, 2049)] + [gs + K + p for p in range(4090, 4101)]
    left = [gs - 1 - p for p in (2047, 2048, 2049)]
    r1 = _mut(r0, right + left)
    reads = [r0, r1, X.revcomp(r0), X.revcomp(r1), r0[:L - 7]]
    rc_pos = L - gs - K
    rows = np.array([X.diag_row(0, 1, 0, gs, gs, support=4), X.diag_row(0, 3, 1, gs, rc_pos), X.diag_row(2, 1, 1, rc_pos, gs), X.diag_row(2, 3, 0, rc_pos, rc_pos),
                     X.diag_row(0, 2, 1, 10, L - 10 - K), X.diag_row(0, 4, 0, L - 7 - K, L - 7 - K), X.diag_row(1, 4, 0, 3, 3)], dtype=np.uint64)
    dna = H.DnaBuffer.from_sequences(reads)
    with H.Context(K=K) as c:
        for xd in (7, 20):
            want, columns = X.extend_rows(rows, reads, K, xdrop=xd)
            if xd == 7:
                assert want[0].tolist() == [rows[0, 0], gs + K + 4090 - 6 - 6, 0 << 32 | gs + K + 4090, 0 << 32 | gs + K + 4090, 6 << 32 | 5, 4]
                assert want[4, 2] == L and want[4, 4] == 15 and want[5, 4] == 0 << 32 | (1 | 4 | 8)
            else:
                assert want[0, 2] == L and int(want[0, 4]) >> 32 == 17
            for span in (1, NONE, 0, 4096):
                ov = _extend(H, c, rows, dna, xdrop=xd, wave_span=span)
                assert np.array_equal(ov.rows(), want), (span, ov.rows().tolist(), want.tolist())
                assert ov.info["columns"] == columns and ov.info["wave_rows"] == {1: 7, NONE: 0, 4096: 7}.get(span, ov.info["wave_rows"])
                if span == 0:
                    assert ov.info["wave_rows"] > 0
        want, _ = X.extend_rows(rows, reads, K, match=1 << 15, mismatch=0, xdrop=0)
        assert int(want[0, 1]) == (L - 17) << 15
        assert np.array_equal(_extend(H, c, rows, dna, match=1 << 15, mismatch=0, xdrop=0, wave_span=1).rows(), want)


# ---- 4. end to end: count -> strands -> pair_diagonals -> extend, rows and reads on the device ---------------------------------------------------
def _pipeline(H, seqs, par, device_reads=None):
    """(context, dna, host PairDiagonals of the reads' best bins, the same list left in HBM)"""
    dna = H.DnaBuffer.from_sequences(seqs)
    c = H.Context(K=par["K"], M=par["M"], L=par["L"], U=par["U"], EXT=1, ntasks=par["ntasks"], keep_device=True)
    with c.count_resident(dna, rid_base=par["rid_base"]) as dev:
        with dev.strands(dna, rid_base=par["rid_base"]) as st:
            pd_dev = dev.pair_diagonals(st, 64, on_device=True)
            pd = dev.pair_diagonals(st, 64)
    return c, dna, pd, pd_dev


def test_end_to_end_on_the_clean_reads(H):
    """The clean reads of tests/test_gpu_strands.py: the genome has no repeated canonical 31-mer and every read is an exact substring of it or
    of its reverse complement, so every shared 31-mer is a true overlap that runs to a read's end."""
    from hysortk_amd import synth
    from tests.test_gpu_strands import _seqs
    seqs, par = _seqs("clean")
    c, dna, pd, pd_dev = _pipeline(H, seqs, par)
    try:
        assert len(pd) == len(pd_dev) > 10000 and pd_dev.rows_dev
        want, columns = X.extend_rows_bulk(pd.rows(), seqs, 31, rid_base=par["rid_base"])
        dp, nb, do, dl = c.synth_reads(20000, 150, 1500, 29)
        ddna = H.DeviceDna(c, dp, nb, do, dl, 1500, par["rid_base"])
        assert np.array_equal(ddna.packed(), dna.arrays()[0])
        with pd_dev.extend(c, ddna, on_device=True) as ov:            # rows and reads in HBM, the result left there
            assert ov.rows_dev and len(ov) == len(pd) and ov.rows().shape == (0, 6)
            got = _fetch(c, ov)
            assert np.array_equal(got, want) and ov.info["columns"] == columns and ov.info["dropped"] == 0
        host = pd.extend(c, dna, rid_base=par["rid_base"])           # host rows, host reads
        assert np.array_equal(host.rows(), want)
        mixed = pd_dev.extend(c, dna, rid_base=par["rid_base"], wave_span=1)
        assert np.array_equal(mixed.rows(), want) and mixed.info["wave_rows"] == len(pd)
        assert np.array_equal(pd.extend(c, ddna, wave_span=NONE).rows(), want)
        ddna.free()
        length = host.a_hi - host.a_lo
        assert not host.mismatches.any() and np.array_equal(host.score, length.astype(np.uint64)) and np.all(host.kind() != H.Overlaps.INTERNAL)
        assert np.array_equal(host.b_hi - host.b_lo, length) and int(length.min()) >= 31 and np.array_equal(host.support, pd.support)
        three = pd.extend(c, dna, rid_base=par["rid_base"], match=3, mismatch=2)
        assert np.array_equal(three.score, 3 * length.astype(np.uint64))
        assert genome_is_repeat_free(synth)
    finally:
        pd_dev.close()
        c.close()


def genome_is_repeat_free(synth):
    """no canonical 31-mer of the clean case's genome occurs twice"""
    g = synth.genome_codes(20000, 29)
    s = "".join("ACGT"[int(x)] for x in g)
    seen = set()
    for i in range(len(s) - 30):
        k = s[i:i + 31]
        k = min(k, X.revcomp(k))
        if k in seen:
            return False
        seen.add(k)
    return True


@pytest.fixture(scope="module")
def noisy(H):
    """The clean reads with 2 % substitutions: (context, dna, seqs, par, host diagonal rows, the same in HBM, the reference rows)."""
    from tests.test_gpu_strands import _seqs
    seqs, par = _seqs("clean")
    rng = np.random.default_rng(31)
    noisy = []
    for s in seqs:
        hit = np.flatnonzero(rng.random(len(s)) < 0.02)
        noisy.append(_mut(s, hit.tolist()))
    c, dna, pd, pd_dev = _pipeline(H, noisy, par)
    want, columns = X.extend_rows_bulk(pd.rows(), noisy, 31, rid_base=par["rid_base"])
    yield c, dna, noisy, par, pd, pd_dev, want, columns
    pd_dev.close()
    c.close()


def test_end_to_end_with_substitutions(H, noisy):
    c, dna, seqs, par, pd, pd_dev, want, columns = noisy
    assert len(pd) > 5000
    for src in (pd, pd_dev):
        for span in (0, 1, NONE):
            ov = src.extend(c, dna, rid_base=par["rid_base"], wave_span=span)
            assert np.array_equal(ov.rows(), want) and ov.info["columns"] == columns and ov.info["wave_rows"] in ((len(pd),) if span == 1 else (0,) if span == NONE else range(len(pd) + 1))
    assert int(ov.mismatches.sum()) > 1000 and (ov.kind() == H.Overlaps.DOVETAIL).any()
    mat = X.code_matrix(seqs)
    kept, _ = X.extend_rows_bulk(pd.rows(), mat, 31, rid_base=par["rid_base"], min_score=50, min_length=80)
    assert 0 < kept.shape[0] < want.shape[0]
    for span in (0, 1, NONE):
        ov = pd_dev.extend(c, dna, rid_base=par["rid_base"], min_score=50, min_length=80, wave_span=span)
        assert np.array_equal(ov.rows(), kept) and ov.info["dropped"] == want.shape[0] - kept.shape[0] and ov.info["columns"] == columns
    with pd.extend(c, dna, rid_base=par["rid_base"], min_score=50, min_length=80, on_device=True) as ov:
        assert np.array_equal(_fetch(c, ov), kept)
    only_len, _ = X.extend_rows_bulk(pd.rows(), mat, 31, rid_base=par["rid_base"], min_length=100)
    assert np.array_equal(pd.extend(c, dna, rid_base=par["rid_base"], min_length=100).rows(), only_len)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals(H, noisy):
    from hysortk_amd import _lib, synth
    c, dna, seqs, par, pd, pd_dev, want, columns = noisy
    base = par["rid_base"]
    packed, off, lens = dna.arrays()
    n = len(pd)

    def works():
        assert np.array_equal(pd_dev.extend(c, dna, rid_base=base).rows(), want)

    def refused(text, fn, *a, **kw):
        with pytest.raises(H.HskError) as e:
            fn(*a, **kw)
        assert e.value.status == 1 and text in str(e.value), str(e.value)
        print(str(e.value))
        works()

    works()
    other = H.DnaBuffer.from_sequences(synth.reads(20000, 150, 1500, 30))
    refused("not the reads", pd.extend, c, other, rid_base=base)                     # the reads of another seed
    refused("outside [", pd.extend, c, (packed, off[:-1], lens[:-1]), rid_base=base)   # one read too few
    refused("outside [", pd_dev.extend, c, dna, rid_base=base + 1)
    moved = pd.rows().copy()
    moved[:, 4] += np.uint64(1 << 32)                                                # every seed moved by one base in A
    refused("not the reads", H.PairDiagonals.from_rows(moved).extend, c, dna, rid_base=base)
    one = pd.rows().copy()
    inside = np.flatnonzero((one[:, 4] >> np.uint64(32)) + np.uint64(32) < 150)[0]
    one[inside, 4] += np.uint64(1 << 32)                                             # ... one seed, which still fits its read
    refused("of the seed of 1 of %d rows do not all match" % n, H.PairDiagonals.from_rows(one).extend, c, dna, rid_base=base)
    fit = pd.rows().copy()
    fit[5, 4] = np.uint64(120 << 32) | (fit[5, 4] & np.uint64(0xFFFFFFFF))           # pa + K = 151 > 150
    refused("does not fit", H.PairDiagonals.from_rows(fit).extend, c, dna, rid_base=base)
    refused("the seed of 1 of %d rows" % n, H.PairDiagonals.from_rows(fit).extend, c, dna, rid_base=base, wave_span=1)
    refused("packed bytes", pd.extend, c, (packed[:-40], off, lens), rid_base=base)   # the last reads lie outside the packed bytes
    refused("xdrop", pd.extend, c, dna, rid_base=base, xdrop=1 << 31)
    refused("match must", pd.extend, c, dna, rid_base=base, match=0)
    refused("match must", pd.extend, c, dna, rid_base=base, match=(1 << 15) + 1)
    refused("mismatch must", pd.extend, c, dna, rid_base=base, mismatch=-1)
    refused("mismatch must", pd.extend, c, dna, rid_base=base, mismatch=(1 << 15) + 1)
    refused("2^31", pd.extend, c, dna, rid_base=2_147_483_000)

    vp = C.c_void_p
    rows = np.ascontiguousarray(pd.rows())
    opts = _lib.ExtendOpts(match=1, mismatch=1, xdrop=7)

    def raw(pdiag, packed_ptr=packed.ctypes.data_as(vp), popts=C.byref(opts), out=None):
        ov = _lib.Overlaps()
        c._check(c.lib.hsk_pair_diags_extend(c.h, pdiag, packed_ptr, packed.size, off.ctypes.data_as(vp), lens.ctypes.data_as(vp), lens.size, base, 0, popts, 0, C.byref(ov) if out is None else out))
        got = np.ctypeslib.as_array(ov.rows, shape=(int(ov.n) * 6,)).reshape(-1, 6).copy() if ov.n else np.zeros((0, 6), np.uint64)
        c.lib.hsk_overlaps_free(c.h, C.byref(ov))
        return got

    good = _lib.PairDiags(n=n, rows=rows.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert np.array_equal(raw(C.byref(good)), want)                                   # a struct filled in by hand, priv NULL
    refused("NULL", raw, C.byref(good), packed_ptr=None)
    refused("NULL", raw, None)
    refused("NULL", raw, C.byref(good), popts=None)
    refused("neither rows nor rows_dev", raw, C.byref(_lib.PairDiags(n=5)))
    refused("16-byte aligned", raw, C.byref(_lib.PairDiags(n=n - 1, rows_dev=pd_dev.rows_dev + 8)))
    assert c.lib.hsk_pair_diags_extend(c.h, C.byref(good), packed.ctypes.data_as(vp), packed.size, off.ctypes.data_as(vp), lens.ctypes.data_as(vp), lens.size, base, 0, C.byref(opts), 0, None) == 1
    works()
    assert raw(C.byref(_lib.PairDiags(n=0))).shape == (0, 6)                          # an empty list is no error
