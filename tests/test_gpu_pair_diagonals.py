"""hsk_result_pair_diagonals (include/hsk.h): the oriented read pairs binned by diagonal, and the best-supported bin of each -- against the
definition applied in numpy to the CPU oracle's EXTENSION result of the same reads (tests/diagonal_ref.py), against a geometry built by hand,
and against the calls that exist (the oriented pair list, the selection and the join on the host).  Everything is integer work and compared
exactly.  The inputs are those of tests/test_gpu_strands.py, and one of its own (`shuffled`)."""
import ctypes as C

import numpy as np
import pytest

from tests import diagonal_ref as D
from tests import oriented_ref as R
from tests.test_gpu_pairs import sort_passes_of
from tests.test_gpu_strands import _case, _open, _revcomp, _seqs

pytestmark = pytest.mark.gpu

TOP = np.uint64(1) << np.uint64(63)
L2_TILE = 1024                                            # bin rows per workgroup of the selection (hsk_pairdiag.h: DS_TILE)


@pytest.fixture(scope="module")
def O():
    from oracle import hsk_oracle
    return hsk_oracle


@pytest.fixture(scope="module")
def H():
    import hysortk_amd
    return hysortk_amd


_OWN = {}


def _own_case(H, O, name, seqs, par):
    """A case of this file, in the form of test_gpu_strands._case."""
    if name not in _OWN:
        dna = H.DnaBuffer.from_sequences(seqs)
        packed, off, lens = dna.arrays()
        o = O.count(packed, off, lens, k=par["K"], m=par["M"], L=par["L"], U=par["U"], ext=1, ntasks=par["ntasks"], rid_base=par["rid_base"])
        _OWN[name] = dict(seqs=seqs, par=par, dna=dna, o=o, strand=R.payload_strands(o, seqs, par["K"], par["rid_base"])[0], ref={})
    return _OWN[name]


def _shuffled(H, O):
    """Read A: 300 000 random bases; read B: 5000 segments A[s : s + 40] in a shuffled order; read C: B's reverse complement.  Pair (A, B) has
    thousands of diagonals (one key's bin rows over several tiles of the selection), (A, C) is its opposite-strand mirror, (B, C) one
    anti-diagonal of about 2 * 10^5 records (one bin run over many tiles of the first reducer)."""
    if "shuffled" not in _OWN:
        rng = np.random.default_rng(13)
        A = "".join(rng.choice(list("ACGT"), 300000))
        perm, jit = rng.permutation(5000), rng.integers(0, 20, 5000)
        B = "".join(A[int(p) * 60 + int(j):int(p) * 60 + int(j) + 40] for p, j in zip(perm, jit))
        _own_case(H, O, "shuffled", [A, B, _revcomp(B)], dict(K=31, M=17, L=2, U=50, ntasks=4, rid_base=0))
    return _OWN["shuffled"]


def _ref(case, W, task_lo=0, task_hi=None, min_support=1):
    """The reference of a case, computed once per (width, task range, min_support); the records once per task range."""
    cache, rng = case.setdefault("dref", {}), ("records", task_lo, task_hi)
    key = (W, task_lo, task_hi, min_support)
    if key not in cache:
        if rng not in cache:
            cache[rng] = D.records(case["o"], case["strand"], task_lo, task_hi)
        cache[key] = D.diagonal_reference(case["o"], case["strand"], W, task_lo, task_hi, min_support, recs=cache[rng])
    return cache[key]


def _check(pd, ref, all_bins):
    want = ref["all_bins"] if all_bins else ref["best"]
    print("diagonals (%s): records %d (reference %d), self %d (%d), keys %d (%d), bins %d (%d), rows %d (%d), sort passes %d" % (
        "all bins" if all_bins else "best bin", pd.info["records"], ref["records"], pd.info["self_records"], ref["self_records"], pd.info["keys"], ref["keys"],
        pd.info["bins"], ref["bins"], len(pd), want.shape[0], pd.info["sort_passes"]))
    assert (pd.info["records"], pd.info["self_records"], pd.info["keys"], pd.info["bins"]) == (ref["records"], ref["self_records"], ref["keys"], ref["bins"])
    assert pd.all_bins == all_bins and len(pd) == want.shape[0]
    assert np.array_equal(pd.rows(), want)
    if all_bins:
        assert np.array_equal(pd.shared, pd.support)
    else:
        assert np.all(pd.shared >= pd.support) and np.all(pd.key[1:] > pd.key[:-1])
    assert np.all(pd.rid_a < pd.rid_b) and np.array_equal(pd.opposite, (pd.key & TOP) != 0)


class _Resident:
    """A case counted once and left on the device, with its strands."""

    def __init__(self, H, case, tuning=None):
        par = case["par"]
        self.case, self.c = case, _open(H, par, tuning=tuning)
        self.dev = self.c.count_resident(case["dna"], rid_base=par["rid_base"])
        self.st = self.dev.strands(case["dna"], rid_base=par["rid_base"])

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.st.close(); self.dev.close(); self.c.close()


@pytest.fixture(scope="module")
def clean(H, O):
    with _Resident(H, _case(H, O, "clean")) as r:
        yield r


# ---- 1. rows against the reference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["clean", "same_read", "wide_entry", "long_run", "clean_k51"])
def test_rows_equal_the_reference(H, O, name):
    case = _case(H, O, name)
    with _Resident(H, case) as r:
        for W in (1, 7, 64):
            best, allb = r.dev.pair_diagonals(r.st, W), r.dev.pair_diagonals(r.st, W, all_bins=True)
            _check(best, _ref(case, W), False)
            _check(allb, _ref(case, W), True)
        ori = r.dev.pairs(strands=r.st)
    assert best.info["records"] == ori.info["records"] and best.info["keys"] == ori.info["keys"] and len(best) == len(ori)
    if name == "same_read":                               # the repeats: pairs inside one read, and read pairs with several diagonals
        assert best.info["self_records"] > 0 and allb.info["bins"] > allb.info["keys"]
    if name.startswith("clean"):
        assert 0 < int(best.opposite.sum()) < len(best)
    if name == "long_run":                                # two copies of one read: every record on the main diagonal, one run over ten tiles of the first reducer
        assert allb.rows().tolist() == [[1, 19970, (1 << 32) // 64, 19970, 0, (19969 << 32) | 19969]]


def test_clean_under_red_zones(H, O):
    case = _case(H, O, "clean")
    with _Resident(H, case, tuning={"pool_redzone": 256}) as r:
        _check(r.dev.pair_diagonals(r.st, 7), _ref(case, 7), False)
        _check(r.dev.pair_diagonals(r.st, 7, all_bins=True), _ref(case, 7), True)


# ---- 2. one key's bin rows over several tiles of the selection, with a tie across tiles ---------------------------------------------------------
def test_shuffled(H, O):
    case = _shuffled(H, O)
    W = 7
    ref = _ref(case, W)
    allb = ref["all_bins"]
    # the preconditions, on the reference: a key with at least 4096 bin rows whose largest support is reached by two bins in different tiles
    keys, first, nb = np.unique(allb[:, 0], return_index=True, return_counts=True)
    big = int(np.argmax(nb))
    rows = allb[first[big]:first[big] + nb[big]]
    at = first[big] + np.flatnonzero(rows[:, 3] == rows[:, 3].max())
    print("shuffled: keys %s, bin rows %s; key %#x: largest support %d at rows %s" % (keys.tolist(), nb.tolist(), int(keys[big]), int(rows[:, 3].max()), at.tolist()))
    assert nb[big] >= 4096 and at.size >= 2 and at[0] // L2_TILE != at[-1] // L2_TILE
    assert ref["records"] > 250000 and int(allb[:, 3].max()) > 100000      # (B, C): one anti-diagonal
    with _Resident(H, case) as r:
        _check(r.dev.pair_diagonals(r.st, W), ref, False)
        _check(r.dev.pair_diagonals(r.st, W, all_bins=True), ref, True)
        _check(r.dev.pair_diagonals(r.st, 1), _ref(case, 1), False)
        _check(r.dev.pair_diagonals(r.st, W, min_support=3), _ref(case, W, min_support=3), False)


# ---- 3. a constructed geometry ------------------------------------------------------------------------------------------------------------------
def test_constructed_geometry(H, O):
    """Read 0 = g[1000:1300], read 1 = g[1100:1250] and read 2 = its reverse complement (test_gpu_strands' geometry): reads 0 and 1 share 120 records
    with pos_a - pos_b = 100, reads 0 and 2 share 120 records with pos_a + pos_b = 219; what the rows must be follows from the construction alone."""
    seqs, par = _seqs("geometry")
    dna = H.DnaBuffer.from_sequences(seqs)
    W = 16
    with _open(H, par) as c:
        with c.count_resident(dna, rid_base=0) as dev:
            with dev.strands(dna, rid_base=0) as st:
                pd = dev.pair_diagonals(st, W)
                allb = dev.pair_diagonals(st, W, all_bins=True)
    lo, hi = pd.diagonal()
    rows = {(int(o), int(a), int(b)): (int(s), int(n), int(p), int(f), int(l), int(x), int(y))
            for o, a, b, s, n, p, f, l, x, y in zip(pd.opposite, pd.rid_a, pd.rid_b, pd.shared, pd.bin, pd.support, pd.first, pd.last, lo, hi)}
    print({k: v for k, v in rows.items() if k[2] <= 2})
    assert rows[(0, 0, 1)] == (120, ((1 << 32) + 100) // W, 120, (100 << 32) | 0, (219 << 32) | 119, 96, 111) and (1, 0, 1) not in rows
    assert rows[(1, 0, 2)] == (120, 219 // W, 120, (100 << 32) | 119, (219 << 32) | 0, 208, 223) and (0, 0, 2) not in rows
    # reads 1 and 2 are each other's reverse complement: pos_a + pos_b = 150 - 31
    assert rows[(1, 1, 2)][:3] == (120, 119 // W, 120) and rows[(1, 1, 2)][5:] == (112, 127)
    assert int((allb.rid_b <= 2).sum()) == 3              # one bin each


# ---- 4. ties to the existing path ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["clean", "same_read"])
def test_ties_to_the_existing_path(H, O, name):
    case = _case(H, O, name)
    with _Resident(H, case) as r:
        ori = r.dev.pairs(strands=r.st)
        for W in (7, 64):
            allb, best = r.dev.pair_diagonals(r.st, W, all_bins=True), r.dev.pair_diagonals(r.st, W)
            sel = allb.select()
            assert len(best) > 100 and np.array_equal(sel.rows(), best.rows()) and sel.info["keys"] == best.info["keys"]
            k = allb.rows()
            start = np.flatnonzero(np.concatenate([[True], k[1:, 0] != k[:-1, 0]]))
            folded = np.stack([k[start, 0], np.add.reduceat(k[:, 3], start), np.minimum.reduceat(k[:, 4], start), np.maximum.reduceat(k[:, 5], start)], axis=1)
            assert np.array_equal(folded, ori.rows())
            assert np.array_equal(best.key, ori.key) and np.array_equal(best.shared, ori.shared)


# ---- 5. task ranges ------------------------------------------------------------------------------------------------------------------------------------
def test_task_ranges_join(H, O, clean):
    r, case, W = clean, clean.case, 7
    whole = _ref(case, W)
    a, b = r.dev.pair_diagonals(r.st, W, 0, 8, all_bins=True), r.dev.pair_diagonals(r.st, W, 8, 16, all_bins=True)
    _check(a, _ref(case, W, task_lo=0, task_hi=8), True)
    _check(b, _ref(case, W, task_lo=8, task_hi=16), True)
    assert len(a) > 100 and len(b) > 100
    comb = H.PairDiagonals.combine([a, b])
    assert np.array_equal(comb.rows(), whole["all_bins"])
    assert (comb.info["records"], comb.info["self_records"], comb.info["keys"], comb.info["bins"]) == (whole["records"], whole["self_records"], whole["keys"], whole["bins"])
    assert np.array_equal(comb.select().rows(), whole["best"])
    assert np.array_equal(comb.select().rows(), r.dev.pair_diagonals(r.st, W).rows())
    _check(r.dev.pair_diagonals(r.st, W, 3, 3), _ref(case, W, task_lo=3, task_hi=3), False)      # an empty range: no rows, no error
    with pytest.raises(ValueError):
        H.PairDiagonals.combine([r.dev.pair_diagonals(r.st, W, 0, 8), r.dev.pair_diagonals(r.st, W, 8, 16)])


# ---- 6. min_support ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ms", [2, 5])
def test_min_support(H, O, clean, ms):
    r, case, W = clean, clean.case, 7
    ref = _ref(case, W, min_support=ms)
    assert 0 < ref["best"].shape[0] < _ref(case, W)["best"].shape[0] and 0 < ref["all_bins"].shape[0] < _ref(case, W)["all_bins"].shape[0]
    best = r.dev.pair_diagonals(r.st, W, min_support=ms)
    _check(best, ref, False)
    _check(r.dev.pair_diagonals(r.st, W, min_support=ms, all_bins=True), ref, True)
    assert np.array_equal(r.dev.pair_diagonals(r.st, W, all_bins=True).select(min_support=ms).rows(), best.rows())


# ---- 7. rows left on the device, ownership ------------------------------------------------------------------------------------------------------------------
def test_on_device_and_ownership(H, O):
    """Rows left in HBM equal the host rows; PairDiagonals, Strands, DeviceResult and Context closed in the order of test_gpu_strands' test_ownership,
    with red zones behind every device block (a call fails if a kernel wrote past one).  What the pool holds is not part of the ABI: as in that
    test, closing launches and copies nothing, and the pool serves the next calls with its red zones checked."""
    case = _case(H, O, "clean")
    par, W = case["par"], 7
    c = _open(H, par, tuning={"pool_redzone": 256})
    dev = c.count_resident(case["dna"], rid_base=par["rid_base"])
    st = dev.strands(case["dna"], rid_base=par["rid_base"])
    host, hosta = dev.pair_diagonals(st, W), dev.pair_diagonals(st, W, all_bins=True)
    _check(host, _ref(case, W), False)
    d, da = dev.pair_diagonals(st, W, on_device=True), dev.pair_diagonals(st, W, all_bins=True, on_device=True)
    for got, want in ((d, host), (da, hosta)):
        assert got.n == len(want) and got.rows_dev and got.rows_dev % 16 == 0 and got.info["records"] == want.info["records"] and got.info["bins"] == want.info["bins"]
        assert np.array_equal(c.d2h(got.rows_dev, got.n * 48).view(np.uint64).reshape(got.n, 6), want.rows())
    with da:
        pass
    assert da.rows_dev is None
    before = c.stats(reset=False)
    st.close()
    d.close()
    dev.close()
    after = c.stats(reset=False)
    assert after["host_syncs"] == before["host_syncs"] and after["d2h_bytes"] == before["d2h_bytes"]      # closing launches and copies nothing
    with c.count_resident(case["dna"], rid_base=par["rid_base"]) as dev3:                                  # ... and the pool serves the next calls (its red zones checked)
        with dev3.strands(case["dna"], rid_base=par["rid_base"]) as st3:
            _check(dev3.pair_diagonals(st3, W), _ref(case, W), False)
    c.close()
    st.close(); d.close(); da.close()                     # closing twice, and after the context, is harmless


# ---- 8. high read ids -------------------------------------------------------------------------------------------------------------------------------------------
def test_high_read_ids(H, O):
    """rid_base = 2^31 - nreads: bits 32 .. 62 of the key are all in use, bit 63 is still the orientation."""
    seqs, par = _seqs("few")
    par = dict(par, rid_base=(1 << 31) - len(seqs))
    case = _own_case(H, O, "few_high", seqs, par)
    with _Resident(H, case) as r:
        for W in (7, 64):
            best = r.dev.pair_diagonals(r.st, W)
            _check(best, _ref(case, W), False)
            _check(r.dev.pair_diagonals(r.st, W, all_bins=True), _ref(case, W), True)
    assert len(best) > 100 and int(best.rid_b.max()) == (1 << 31) - 1 and int(best.rid_a.min()) >= par["rid_base"] and 0 < int(best.opposite.sum()) < len(best)


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(H, O, clean):
    from hysortk_amd import _lib
    r, case, W = clean, clean.case, 7
    c, dev, st, par = r.c, r.dev, r.st, case["par"]

    def works():
        _check(dev.pair_diagonals(st, W), _ref(case, W), False)

    def refused(text, *a, **kw):
        with pytest.raises(H.HskError) as e:
            dev.pair_diagonals(*a, **kw)
        assert e.value.status == 1 and text in str(e.value), str(e.value)
        works()

    refused("diag_bin", st, 0)
    refused("diag_bin", st, (1 << 31) + 1)
    refused("min_support", st, W, min_support=0)
    refused("task range", st, W, 0, 17)
    refused("task range", st, W, 5, 4)
    refused("task range", st, W, -1, 4)
    refused("strands is NULL", None, W)
    few = _case(H, O, "few")
    with c.count_resident(few["dna"], rid_base=par["rid_base"]) as dev2:
        with dev2.strands(few["dna"], rid_base=par["rid_base"]) as st2:
            refused("do not belong", st2, W)
    _check(dev.pair_diagonals(st, 1 << 31), _ref(case, 1 << 31), False)      # the largest width is accepted
    pd = _lib.PairDiags()
    assert c.lib.hsk_result_pair_diagonals(c.h, None, C.byref(st.st), 0, 16, W, 1, 0, 0, C.byref(pd)) == 1
    assert c.lib.hsk_result_pair_diagonals(c.h, C.byref(dev.res), C.byref(st.st), 0, 16, W, 1, 0, 0, None) == 1
    works()
    # a resident result without EXTENSION; an EXTENSION result that was not left on the device
    packed, off, lens = case["dna"].arrays()
    kw = dict(K=par["K"], M=par["M"], L=par["L"], U=par["U"], ntasks=par["ntasks"])
    for ctx_kw in (dict(EXT=0, keep_device=True), dict(EXT=1)):
        with H.Context(**kw, **ctx_kw) as c2:
            res, pd = _lib.Result(), _lib.PairDiags()
            c2._check(c2.lib.hsk_count(c2.h, packed.ctypes.data_as(C.c_void_p), packed.size, off.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), lens.size, par["rid_base"], C.byref(res)))
            assert c2.lib.hsk_result_pair_diagonals(c2.h, C.byref(res), C.byref(st.st), 0, 1, W, 1, 0, 0, C.byref(pd)) == 1 and c2.lib.hsk_last_error(c2.h)
            c2.lib.hsk_result_free(c2.h, C.byref(res))
    works()


# ---- 10. sort passes -------------------------------------------------------------------------------------------------------------------------------------------------
def test_sort_passes(H, O, clean):
    """Positions are below 256 (150-base reads), so with diag_bin = 16 the sorted bin word has fewer than 64 values: one digit on top of the oriented
    call's passes over the pair key.  The second digit of the margin is slack for a different base of the word."""
    r = clean
    ori = r.dev.pairs(strands=r.st)
    pd = r.dev.pair_diagonals(r.st, 16)
    print("sort passes: oriented %d, diagonals %d" % (ori.info["sort_passes"], pd.info["sort_passes"]))
    assert ori.info["sort_passes"] >= 0 and pd.info["sort_passes"] >= 0
    assert pd.info["sort_passes"] <= ori.info["sort_passes"] + 2
    # The two-word record keys by their definition (hsk_diagbin.h): word 1 the pair key, word 0 the bin less the smallest bin a record of that
    # orientation can have under the largest position among the payload slots of the entries that have records; a pair inside one read is { 0, 0 }.
    o, ref = r.case["o"], _ref(r.case, 16)
    ent = np.flatnonzero(o.cnt >= 2)
    maxpos = max(int(o.pos[int(p):int(p) + int(n)].max()) for p, n in zip(o.payoff[ent], o.cnt[ent]))
    key, bins = ref["all_bins"][:, 0], ref["all_bins"][:, 2]
    word0 = bins - np.where((key & TOP) != 0, 0, ((1 << 32) - maxpos) // 16).astype(np.uint64)
    words = np.stack([word0, key], axis=1)
    if ref["self_records"]:
        words = np.concatenate([np.zeros((1, 2), np.uint64), words])
    assert pd.info["sort_passes"] == sort_passes_of(words)
