"""hsk_pair_diags_extend_gapped (include/hsk.h): the seed of every diagonal row extended in both directions inside a band of diagonals, over
the reads in HBM -- against the definition applied base by base (tests/gapped_ref.py, itself held to hand-written rows by
tests/test_gapped_ref.py; its bulk form where the rows are many or long).  Everything is integer work and compared word for word, `columns`
and `cells` included.  Every case runs through every legal group width (0: the library's choice; 8, 16, 32, 64 where band <= width - 1)
and must give the same rows."""
import ctypes as C

import numpy as np
import pytest

from tests import extend_ref as X
from tests import gapped_ref as G
from tests.test_extend_ref import random_case

pytestmark = pytest.mark.gpu

WIDTHS = (8, 16, 32, 64)


@pytest.fixture(scope="module")
def H():
    import hysortk_amd
    return hysortk_amd


def _groups(band):
    return [0] + [w for w in WIDTHS if band <= w - 1]


def _gapped(H, c, rows, dna, rid_base=0, **kw):
    return H.PairDiagonals.from_rows(rows).extend_gapped(c, dna, rid_base=rid_base, **kw)


def _all_groups(H, c, rows, dna, ref, rid_base=0, groups=None, **kw):
    """every legal width: the reference's rows word for word, its columns and its cells"""
    want, columns, cells = ref
    n = np.asarray(rows).reshape(-1, 6).shape[0]
    band = kw.get("band", 15)
    for group in groups or _groups(band):
        ov = _gapped(H, c, rows, dna, rid_base=rid_base, group=group, **kw)
        got = ov.rows()
        print("band %d group %d: %d rows (reference %d), columns %d (%d), cells %d (%d), dropped %d, %.3f ms" % (band, group, len(ov), want.shape[0], ov.info["columns"], columns, ov.info["cells"], cells,
                                                                                                             ov.info["dropped"], ov.info["ms_extend"]))
        bad = np.flatnonzero((got != want).any(axis=1)) if got.shape == want.shape else None
        assert got.shape == want.shape and bad.size == 0, "group %d: row %s is %s, the reference has %s" % (group, bad[:1], got[bad[:1]].tolist(), want[bad[:1]].tolist())
        assert ov.info["input_rows"] == n and ov.info["dropped"] == n - want.shape[0] and ov.info["columns"] == columns and ov.info["cells"] == cells and ov.info["wave_rows"] == 0
        assert ov.edits is ov.mismatches
    return ov


def _fetch(c, ov):
    """the rows of a list that was left in HBM"""
    return c.d2h(ov.rows_dev, len(ov) * 48).view(np.uint64).reshape(len(ov), 6)


def _spans(rows):
    lo = np.uint64(0xFFFFFFFF)
    return ((rows[:, 2] & lo) - (rows[:, 2] >> np.uint64(32))).astype(np.int64), ((rows[:, 3] & lo) - (rows[:, 3] >> np.uint64(32))).astype(np.int64)


# ---- 1. band 0 is the ungapped call ------------------------------------------------------------------------------------------------------------
def test_band_0_equals_the_ungapped_reference(H):
    reads, rows = random_case(np.random.default_rng(2024), 2000, 20000, 31, 31, 400)
    assert rows.shape[0] == 20000 and len(reads) == 2000
    mat = X.code_matrix(reads)
    dna = H.DnaBuffer.from_sequences(reads)
    with H.Context(K=31) as c:
        for m, mm, xd in ((1, 1, 7), (2, 3, 5)):
            want, columns = X.extend_rows_bulk(rows, mat, 31, match=m, mismatch=mm, xdrop=xd)
            gwant, gcolumns, cells = G.extend_rows_bulk(rows, mat, 31, match=m, mismatch=mm, gap=3, xdrop=xd, band=0)
            assert np.array_equal(gwant, want) and gcolumns == columns
            ov = _all_groups(H, c, rows, dna, (want, columns, cells), match=m, mismatch=mm, gap=3, xdrop=xd, band=0)
            assert np.array_equal(ov.rows(), _ungapped(H, c, rows, dna, match=m, mismatch=mm, xdrop=xd))
        assert int(ov.edits.sum()) > 1000 and len(set(ov.kind().tolist())) == 4


def _ungapped(H, c, rows, dna, **kw):
    return H.PairDiagonals.from_rows(rows).extend(c, dna, **kw).rows()


# ---- 2. geometry by hand -------------------------------------------------------------------------------------------------------------------------
def _edited(g, s0, n, edits, rng):
    """g[s0 : s0 + n) with edits (kind, genome position, size): 'ins' puts `size` random bases in front of the position, 'del' drops the
    `size` bases from it on, 'sub' changes the base; and shift(p) = how far the base at genome position p has moved in the read"""
    s = list(g[s0:s0 + n])
    for kind, p, size in sorted(edits, key=lambda e: -e[1]):
        q = p - s0
        assert 0 <= q and q + (size if kind != "ins" else 0) <= len(s)
        if kind == "ins":
            s[q:q] = list(rng.choice(list("ACGT"), size))
        elif kind == "del":
            del s[q:q + size]
        else:
            s[q] = "ACGT"[("ACGT".index(s[q]) + 1) % 4]
    return "".join(s), lambda p: sum((size if kind == "ins" else -size) for kind, q, size in edits if kind != "sub" and q <= p)


def _hand_cases(K):
    """(reads, rows): every case is two reads cut from one genome -- A from g[sa : sa + la), B from g[sb : sb + lb) or its reverse
    complement, each with its own edits, the seed at genome position gs (no edit touches it) -- and one row by hand."""
    rng = np.random.default_rng(300 + K)
    g = "".join(rng.choice(list("ACGT"), 700))
    reads, rows = [], []

    def add(sa, la, sb, lb, gs, o, ea=(), eb=(), n_at=None, same=False):
        a, shift_a = _edited(g, sa, la, ea, rng)
        if n_at is not None:
            q = n_at - sa + shift_a(n_at)
            assert a[q] == "A"
            a = a[:q] + "N" + a[q + 1:]
        bf, shift_b = (a, shift_a) if same else _edited(g, sb, lb, eb, rng)
        pa, pf = gs - sa + shift_a(gs), gs - (sa if same else sb) + shift_b(gs)
        assert a[pa:pa + K].replace("N", "A") == g[gs:gs + K] == bf[pf:pf + K].replace("N", "A") and len(a) <= 200 and len(bf) <= 200
        b = X.revcomp(bf) if o else bf
        rows.append(X.diag_row(len(reads), len(reads) + 1, o, pa, len(bf) - pf - K if o else pf, support=len(rows) + 1))
        reads.extend([a, b])

    for o in (0, 1):
        near, far = 105, 260 - K                                      # a seed near the reads' start (room on the right) and near their end
        for size in (1, 3):                                           # indels of 1 and 3 bases in A and in B, either side of the seed
            for kind in ("ins", "del"):
                add(100, 190, 95, 190, near, o, ea=[(kind, near + K + 20, size)])
                add(100, 190, 95, 190, near, o, eb=[(kind, near + K + 20, size)])
                add(100, 190, 95, 190, far, o, ea=[(kind, far - 20, size)])
                add(100, 190, 95, 190, far, o, eb=[(kind, far - 20, size)])
        for d in (0, 1, 31, 32, 33, 63, 64, 65):                      # an indel behind walk position d of either side: next to the seed, and where the windows are loaded again
            add(100, 190, 95, 190, near, o, ea=[("del", near + K + d, 1)])
            add(100, 190, 95, 190, near, o, eb=[("ins", near + K + d, 2)])
            add(100, 190, 95, 190, far, o, ea=[("ins", far - d, 1)])
            add(100, 190, 95, 190, far, o, eb=[("del", far - d - 2, 2)])
        add(100, 195, 90, 190, 170, o, ea=[("del", 150, 2), ("sub", 160, 1), ("ins", 170 + K + 9, 3), ("sub", 170 + K + 30, 1)], eb=[("ins", 140, 1), ("del", 170 + K + 40, 1)])
        add(200, K + 50, 150, 190, 200, o, eb=[("del", 200 + K + 10, 1)])       # the seed at A's start
        add(200, K + 50, 150, 190, 250, o, eb=[("ins", 240, 1)])                # ... at A's end
        add(200, K, 150, 190, 200, o)                                           # A is the seed
        add(150, 190, 200, K, 200, o)                                           # B is the seed
        add(150, 190, 200, 131, 200, o, ea=[("del", 200 + K + 5, 3)])           # the seed at B's forward start
        add(150, 190, 130, 70 + K, 200, o, ea=[("ins", 190, 3)])                # ... at B's forward end
        add(100, 197, 90, 190, 170, o, ea=[("del", 170 + K + 50, 1)], n_at=g.index("A", 170 + K + 5))      # an N against an A: a match
        add(100, 199, 100, 199, 110, o, same=True)                              # identical reads
        add(100, 190, 100, 190, 150, o, ea=[("del", 150 + K + 30, 8)])          # a gap of 8: bands 7 and 8
        add(100, 180, 100, 180, 120, o, eb=[("ins", 120 + K + 25, 16)])         # ... of 16: bands 15 and 16
    return reads, np.array(rows, dtype=np.uint64)


BANDS = (0, 1, 2, 3, 7, 8, 15, 16, 31, 32, 63)


@pytest.mark.parametrize("K", [31, 51])
def test_hand_geometry(H, K):
    reads, rows = _hand_cases(K)
    mat = X.code_matrix(reads)
    dna = H.DnaBuffer.from_sequences(reads)
    assert any(len(r) % 4 for r in reads) and rows.shape[0] > 100
    with H.Context(K=K) as c:
        for m, mm, gp, xd in ((1, 1, 1, 7), (1, 1, 1, 0), (2, 3, 2, 5), (1, 0, 0, 3), (255, 255, 255, (1 << 31) - 1)):
            for band in BANDS:
                ref = G.extend_rows_bulk(rows, mat, K, match=m, mismatch=mm, gap=gp, xdrop=xd, band=band)
                if band == 3 and xd == 7:
                    slow = G.extend_rows(rows, reads, K, match=m, mismatch=mm, gap=gp, xdrop=xd, band=band)       # the row form, base by base
                    assert np.array_equal(slow[0], ref[0]) and slow[1:] == ref[1:]
                ov = _all_groups(H, c, rows, dna, ref, match=m, mismatch=mm, gap=gp, xdrop=xd, band=band)
                assert np.array_equal(ov.support, rows[:, 3]) and np.array_equal(ov.key, rows[:, 0])
        # what the construction says, without the reference: a single indel of `size` bases is crossed by a band of `size`, and the overlap
        # then runs to a read's end on either side with `size` edits; a band of size - 1 cannot hold it and stops inside the reads
        per = rows.shape[0] // 2
        for o in (0, 1):
            for t, size in ((0, 1), (8, 3)):                          # the first case of each size: an insertion in A on the right
                i = o * per + t
                wide, narrow = _gapped(H, c, rows, dna, band=size), _gapped(H, c, rows, dna, band=size - 1)
                assert wide.kind()[i] != H.Overlaps.INTERNAL and wide.edits[i] == size and wide.a_hi[i] - wide.a_lo[i] == wide.b_hi[i] - wide.b_lo[i] + size, wide.rows()[i].tolist()
                assert narrow.kind()[i] == H.Overlaps.INTERNAL and narrow.score[i] < wide.score[i], narrow.rows()[i].tolist()
            ident = o * per + per - 3
            assert wide.a_lo[ident] == 0 and wide.a_hi[ident] == 199 and wide.ends[ident] == 15 and wide.kind()[ident] == H.Overlaps.A_CONTAINED and wide.score[ident] == 199 and wide.edits[ident] == 0


# ---- 3. the bulk comparison ----------------------------------------------------------------------------------------------------------------------
def _bulk_case():
    """3000 rows on reads of about 31-400 bases with 2 % substitutions and 1 % indels outside the protected seeds; a row's reads share at
    least seven tenths of the longer one, so that most overlaps are long enough to meet an indel, and a read is in two rows on average, so that the protected seeds leave most of it open"""
    return G.indel_case(np.random.default_rng(4242), 3000, 3000, 31, 31, 400, genome=20000, sub=0.02, indel=0.01, near=30, share=0.7)


@pytest.fixture(scope="module")
def bulk():
    reads, rows = _bulk_case()
    return reads, rows, X.code_matrix(reads)


def test_random_rows_with_indels(H, bulk):
    reads, rows, mat = bulk
    assert rows.shape[0] == 3000
    dna = H.DnaBuffer.from_sequences(reads)
    ungapped, _ = X.extend_rows_bulk(rows, mat, 31)
    with H.Context(K=31) as c:
        for band in (7, 15):
            ref = G.extend_rows_bulk(rows, mat, 31, band=band)
            # the case exercises gaps: most overlaps are longer than the ungapped ones, and most cross a gap
            (ga, gb), (ua, _) = _spans(ref[0]), _spans(ungapped)
            print("band %d: %.1f %% of the rows longer than the ungapped overlap, %.1f %% with spans that differ" % (band, 100 * (ga > ua).mean(), 100 * (ga != gb).mean()))
            assert (ga > ua).mean() >= 0.5 and (ga != gb).mean() >= 0.5
            ov = _all_groups(H, c, rows, dna, ref, band=band)
        assert len(set(ov.kind().tolist())) >= 3
        # the filter: the survivors are the reference's, in order
        med = int(np.median(ref[0][:, 1]))
        keep = (ref[0][:, 1] >= np.uint64(med)) & (_spans(ref[0])[0] >= 60)
        kept = (ref[0][keep],) + ref[1:]
        assert 300 < kept[0].shape[0] < 2700
        _all_groups(H, c, rows, dna, kept, band=15, min_score=med, min_length=60)
        # a filter that drops everything, and an empty list
        ov = _gapped(H, c, rows, dna, min_score=1 << 40)
        assert len(ov) == 0 and ov.info["dropped"] == 3000 and ov.rows().shape == (0, 6) and ov.info["cells"] == ref[2]
        ov = _gapped(H, c, np.zeros((0, 6), np.uint64), dna)
        assert len(ov) == 0 and ov.info == dict(ov.info, input_rows=0, dropped=0, columns=0, cells=0, wave_rows=0)


# ---- 4. long rows --------------------------------------------------------------------------------------------------------------------------------
def _long_case():
    """Two reads of about 20 000 bases of one genome: the second with 40 scattered indels of one base and 200 substitutions outside the seed in
    the middle; and their reverse complements."""
    K, L, gs = 31, 20000, 10007
    rng = np.random.default_rng(77)
    g = rng.integers(0, 4, L)
    protect = np.zeros(L, bool)
    protect[gs:gs + K] = True
    sub = rng.choice(np.flatnonzero(~protect), 240, replace=False)
    edits = [("sub", int(p), 1) for p in sub[:200]] + [("ins" if t % 2 else "del", int(p), 1) for t, p in enumerate(sub[200:])]
    edits = [e for e in edits if not (e[0] != "sub" and gs - 1 <= e[1] <= gs + K)]
    gstr = "".join("ACGT"[x] for x in g)
    r1, shift = _edited(gstr, 0, L, edits, rng)
    p1 = gs + shift(gs)
    assert r1[p1:p1 + K] == gstr[gs:gs + K] and sum(e[0] != "sub" for e in edits) >= 38
    reads = [gstr, r1, X.revcomp(gstr), X.revcomp(r1)]
    rc0, rc1 = L - gs - K, len(r1) - p1 - K
    rows = np.array([X.diag_row(0, 1, 0, gs, p1, support=4), X.diag_row(0, 3, 1, gs, rc1), X.diag_row(2, 1, 1, rc0, p1), X.diag_row(2, 3, 0, rc0, rc1)], dtype=np.uint64)
    return reads, rows


def test_long_rows(H):
    reads, rows = _long_case()
    mat = X.code_matrix(reads)
    dna = H.DnaBuffer.from_sequences(reads)
    with H.Context(K=31) as c:
        for band, groups in ((31, (32, 64)), (63, (64,))):
            ref = G.extend_rows_bulk(rows, mat, 31, band=band)
            ga, gb = _spans(ref[0])
            assert (ga > 19000).all() and (ref[0][:, 4] >> np.uint64(32) > 230).all(), ref[0].tolist()       # the overlaps cross all the indels
            _all_groups(H, c, rows, dna, ref, groups=groups, band=band)


# ---- 5. end to end: count -> strands -> pair_diagonals -> extend_gapped, rows and reads on the device ----------------------------------------------
@pytest.fixture(scope="module")
def chain(H):
    """The clean reads of tests/test_gpu_strands.py with 1 % substitutions and 0.5 % indels: (context, dna, seqs, par, host diagonal rows,
    the same in HBM, the reference for the defaults)."""
    from tests.test_gpu_strands import _seqs
    from tests.test_gpu_extend import _pipeline
    seqs, par = _seqs("clean")
    rng = np.random.default_rng(131)
    noisy = []
    for s in seqs:
        f, _ = G.mutate(np.array(X.codes(s)), np.zeros(len(s), bool), rng, 0.01, 0.005)
        noisy.append("".join("ACGT"[x] for x in f))
    assert len(noisy) == 1500 and len({len(s) for s in noisy}) > 3
    c, dna, pd, pd_dev = _pipeline(H, noisy, par)
    mat = X.code_matrix(noisy)
    ref = G.extend_rows_bulk(pd.rows(), mat, 31, rid_base=par["rid_base"])
    yield c, dna, noisy, par, pd, pd_dev, ref, mat
    pd_dev.close()
    c.close()


def test_end_to_end_with_indels(H, chain, tmp_path):
    c, dna, seqs, par, pd, pd_dev, ref, mat = chain
    want, columns, cells = ref
    base = par["rid_base"]
    assert len(pd) == len(pd_dev) > 5000 and pd_dev.rows_dev
    ga, gb = _spans(want)
    assert (ga != gb).mean() > 0.2 and int((want[:, 4] >> np.uint64(32)).sum()) > 5000
    packed, off, lens = dna.arrays()
    fa = tmp_path / "noisy.fa"                                        # the reads into HBM: packed on the GPU from a FASTA file
    with open(fa, "wb") as f, open(str(fa) + ".fai", "w") as fai:
        for i, s in enumerate(seqs):
            f.write(b">r%d\n" % i)
            fai.write("r%d\t%d\t%d\t%d\t%d\n" % (i, len(s), f.tell(), len(s), len(s) + 1))
            f.write(s.encode() + b"\n")
    ddna = H.read_dna_buffer_device(c, str(fa))
    ddna.first_read_id = base
    assert ddna.nreads == lens.size and ddna.packed().tobytes() == packed.tobytes()
    with pd_dev.extend_gapped(c, ddna, on_device=True) as ov:         # rows and reads in HBM, the result left there
        assert ov.rows_dev and len(ov) == len(pd) and ov.rows().shape == (0, 6)
        assert np.array_equal(_fetch(c, ov), want) and ov.info["columns"] == columns and ov.info["cells"] == cells and ov.info["dropped"] == 0
    for src in (pd, pd_dev):                                          # host rows and rows in HBM, host reads, every width
        for group in _groups(15):
            ov = src.extend_gapped(c, dna, rid_base=base, group=group)
            assert np.array_equal(ov.rows(), want) and ov.info["columns"] == columns and ov.info["cells"] == cells
    assert np.array_equal(pd.extend_gapped(c, ddna).rows(), want)     # host rows, reads in HBM
    ddna.free()
    assert np.array_equal(ov.support, pd.support) and (ov.kind() == H.Overlaps.DOVETAIL).any()
    kept = G.extend_rows_bulk(pd.rows(), mat, 31, rid_base=base, band=7, min_score=50, min_length=80)
    assert 0 < kept[0].shape[0] < want.shape[0]
    ov = pd_dev.extend_gapped(c, dna, rid_base=base, band=7, min_score=50, min_length=80)
    assert np.array_equal(ov.rows(), kept[0]) and ov.info["dropped"] == want.shape[0] - kept[0].shape[0] and ov.info["columns"] == kept[1] and ov.info["cells"] == kept[2]
    with pd.extend_gapped(c, dna, rid_base=base, band=7, min_score=50, min_length=80, on_device=True) as ov:
        assert np.array_equal(_fetch(c, ov), kept[0])


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(H, chain):
    from hysortk_amd import _lib, synth
    c, dna, seqs, par, pd, pd_dev, ref, mat = chain
    want = ref[0]
    base = par["rid_base"]
    packed, off, lens = dna.arrays()
    n = len(pd)

    def works():
        assert np.array_equal(pd_dev.extend_gapped(c, dna, rid_base=base).rows(), want)

    def refused(text, fn, *a, **kw):
        with pytest.raises(H.HskError) as e:
            fn(*a, **kw)
        assert e.value.status == 1 and text in str(e.value) and "hsk_pair_diags_extend_gapped" in str(e.value), str(e.value)
        print(str(e.value))
        works()

    works()
    # every refusal of the ungapped call
    other = H.DnaBuffer.from_sequences(synth.reads(20000, 150, 1500, 30))
    refused("not the reads", pd.extend_gapped, c, other, rid_base=base)
    refused("outside [", pd.extend_gapped, c, (packed, off[:-1], lens[:-1]), rid_base=base)
    refused("outside [", pd_dev.extend_gapped, c, dna, rid_base=base + 1)
    moved = pd.rows().copy()
    moved[:, 4] += np.uint64(1 << 32)
    refused("not the reads", H.PairDiagonals.from_rows(moved).extend_gapped, c, dna, rid_base=base)
    one = pd.rows().copy()
    la = lens[((one[:, 0] >> np.uint64(32)) & np.uint64(0x7FFFFFFF)).astype(np.int64) - base]
    inside = np.flatnonzero((one[:, 4] >> np.uint64(32)) + np.uint64(32) < la)[0]
    one[inside, 4] += np.uint64(1 << 32)
    refused("of the seed of 1 of %d rows do not all match" % n, H.PairDiagonals.from_rows(one).extend_gapped, c, dna, rid_base=base)
    fit = pd.rows().copy()
    fit[5, 4] = np.uint64(190 << 32) | (fit[5, 4] & np.uint64(0xFFFFFFFF))
    refused("does not fit", H.PairDiagonals.from_rows(fit).extend_gapped, c, dna, rid_base=base)
    refused("the seed of 1 of %d rows" % n, H.PairDiagonals.from_rows(fit).extend_gapped, c, dna, rid_base=base, group=64)
    refused("packed bytes", pd.extend_gapped, c, (packed[:-40], off, lens), rid_base=base)
    refused("xdrop", pd.extend_gapped, c, dna, rid_base=base, xdrop=1 << 31)
    refused("match must", pd.extend_gapped, c, dna, rid_base=base, match=0)
    refused("match must", pd.extend_gapped, c, dna, rid_base=base, match=256)
    refused("mismatch must", pd.extend_gapped, c, dna, rid_base=base, mismatch=-1)
    refused("mismatch must", pd.extend_gapped, c, dna, rid_base=base, mismatch=256)
    refused("2^31", pd.extend_gapped, c, dna, rid_base=2_147_483_000)
    # the gapped call's own
    refused("gap must be 0 .. 255 (256 given, %d rows)" % n, pd.extend_gapped, c, dna, rid_base=base, gap=256)
    refused("gap must", pd.extend_gapped, c, dna, rid_base=base, gap=-1)
    refused("band must be 0 .. 63 (64 given, %d rows)" % n, pd.extend_gapped, c, dna, rid_base=base, band=64)
    refused("a group of 8 lanes holds bands up to 7 (band 8 given, %d rows)" % n, pd.extend_gapped, c, dna, rid_base=base, band=8, group=8)
    refused("group must be 0, 8, 16, 32 or 64 (12 given, %d rows)" % n, pd.extend_gapped, c, dna, rid_base=base, group=12)
    refused("a group of 32 lanes", pd_dev.extend_gapped, c, dna, rid_base=base, band=32, group=32)
    # two reads with la + lb = 2^22: refused before any walk (the reads are equal, the seed is one)
    big = "".join(np.random.default_rng(3).choice(list("ACGT"), 1 << 21))
    bigdna = H.DnaBuffer.from_sequences([big, big, big[:-1]])
    refused("2^22 bases or more together", H.PairDiagonals.from_rows([X.diag_row(0, 1, 0, 5, 5), X.diag_row(0, 2, 0, 5, 5)]).extend_gapped, c, bigdna, xdrop=0)
    refused("of 1 of 2 rows", H.PairDiagonals.from_rows([X.diag_row(0, 1, 0, 5, 5), X.diag_row(0, 2, 0, 5, 5)]).extend_gapped, c, bigdna, xdrop=0)

    vp = C.c_void_p
    rows = np.ascontiguousarray(pd.rows())
    opts = _lib.GappedOpts(match=1, mismatch=1, gap=1, xdrop=7, band=15)

    def raw(pdiag, packed_ptr=packed.ctypes.data_as(vp), popts=C.byref(opts), out=None):
        ov = _lib.Overlaps()
        c._check(c.lib.hsk_pair_diags_extend_gapped(c.h, pdiag, packed_ptr, packed.size, off.ctypes.data_as(vp), lens.ctypes.data_as(vp), lens.size, base, 0, popts, 0, C.byref(ov) if out is None else out))
        got = np.ctypeslib.as_array(ov.rows, shape=(int(ov.n) * 6,)).reshape(-1, 6).copy() if ov.n else np.zeros((0, 6), np.uint64)
        assert ov.cells == (ref[2] if ov.n else 0)
        c.lib.hsk_overlaps_free(c.h, C.byref(ov))
        return got

    good = _lib.PairDiags(n=n, rows=rows.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert np.array_equal(raw(C.byref(good)), want)                                   # a struct filled in by hand, priv NULL
    refused("NULL", raw, C.byref(good), packed_ptr=None)
    refused("NULL", raw, None)
    refused("NULL", raw, C.byref(good), popts=None)
    refused("neither rows nor rows_dev", raw, C.byref(_lib.PairDiags(n=5)))
    refused("16-byte aligned", raw, C.byref(_lib.PairDiags(n=n - 1, rows_dev=pd_dev.rows_dev + 8)))
    assert c.lib.hsk_pair_diags_extend_gapped(c.h, C.byref(good), packed.ctypes.data_as(vp), packed.size, off.ctypes.data_as(vp), lens.ctypes.data_as(vp), lens.size, base, 0, C.byref(opts), 0, None) == 1
    works()
    assert raw(C.byref(_lib.PairDiags(n=0))).shape == (0, 6)                          # an empty list is no error
    assert c.lib.hsk_abi_version() == 4
