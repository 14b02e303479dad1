"""hsk_result_pair_diagonals_sliced (include/hsk.h): the read pairs by diagonal of a resident EXTENSION result from at most max_records
records expanded at a time -- the slice planner, the window arguments of the expansion with the two-word key, one bound of the positions
for all slices, and the merges of the slices' all-bins lists on (key, bin) (hsk_rowmerge.h) with the selection behind them -- against
the definition applied in numpy to the CPU oracle's result (tests/diagonal_ref.py).  Everything is integer work and compared exactly,
whatever the budget.  The inputs are those of tests/test_gpu_pair_diagonals.py."""
import ctypes as C

import numpy as np
import pytest

from tests import diagonal_ref as D
from tests.test_gpu_pairs import U32, _triu, sort_passes_of
from tests.test_gpu_pairs_sliced import _prime_near, slice_plan
from tests.test_gpu_pair_diagonals import TOP, _Resident, _check, _own_case, _ref, _shuffled
from tests.test_gpu_strands import _case, _seqs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def O():
    from oracle import hsk_oracle
    return hsk_oracle


@pytest.fixture(scope="module")
def H():
    import hysortk_amd
    return hysortk_amd


def _get(H, O, name):
    return _shuffled(H, O) if name == "shuffled" else _case(H, O, name)


def entry_records(case):
    """The records of the whole range in the order of the expansion, entry by entry, computed once per case: (keys, values, off) -- a
    pair inside one read is key 0 and value 0; off: the record offset of every entry that has records, the total last."""
    if "entry_records" not in case:
        o, sb = case["o"], case["strand"].astype(np.uint64)
        rid = o.rid.astype(np.int64).astype(np.uint64) & U32
        pos = o.pos.astype(np.uint64)
        ks, vs, off = [np.zeros(0, np.uint64)], [np.zeros(0, np.uint64)], [0]
        for e in np.flatnonzero(o.cnt >= 2):
            i, j = _triu(int(o.cnt[e]))
            si, sj = int(o.payoff[e]) + i, int(o.payoff[e]) + j
            sw = rid[si] > rid[sj]
            ra, rb, pa, pb = np.where(sw, rid[sj], rid[si]), np.where(sw, rid[si], rid[sj]), np.where(sw, pos[sj], pos[si]), np.where(sw, pos[si], pos[sj])
            k = ((sb[si] ^ sb[sj]) << np.uint64(63)) | (ra << np.uint64(32)) | rb
            self_ = ra == rb
            ks.append(np.where(self_, np.uint64(0), k)); vs.append(np.where(self_, np.uint64(0), (pa << np.uint64(32)) | pb)); off.append(off[-1] + i.size)
        case["entry_records"] = (np.concatenate(ks), np.concatenate(vs), np.array(off, np.int64))
    return case["entry_records"]


def sort_words(case, W):
    """([records, 2] the two-word sort keys of the records in the order of the expansion, off): the keys test_gpu_pair_diagonals'
    test_sort_passes defines -- word 1 the pair key, word 0 the bin less the smallest bin a record of that orientation can have under the
    largest position among the payload slots of the entries that have records; a pair inside one read is { 0, 0 }."""
    o = case["o"]
    k, v, off = entry_records(case)
    ent = np.flatnonzero(o.cnt >= 2)
    maxpos = max(int(o.pos[int(p):int(p) + int(n)].max()) for p, n in zip(o.payoff[ent], o.cnt[ent]))
    real = k != 0
    word0 = np.zeros(k.size, np.uint64)
    word0[real] = D.bins_of(k[real], v[real], W) - np.where((k[real] & TOP) != 0, 0, ((1 << 32) - maxpos) // W).astype(np.uint64)
    return np.stack([word0, k], axis=1), off


def slice_cuts(off, budget):
    """The record offsets at which the planner cuts (hsk_pairplan.h, as tests/test_gpu_pairs_sliced.py's slice_plan walks them)."""
    cuts, a = [0], 0
    while a + 1 < off.size:
        a = max(int(np.searchsorted(off, off[a] + budget, side="right")) - 1, a + 1)
        cuts.append(int(off[a]))
    return cuts


def _largest_entry(o):
    c = int(o.cnt.max()) if o.cnt.size else 0
    return c * (c - 1) // 2


def _check_sliced(pd, ref, all_bins, m, largest, plan=None):
    """plan: (sort words, off) of the range, where slices and sort_passes are held to the planner's rule."""
    _check(pd, ref, all_bins)                             # rows, records, self_records, keys, bins
    records, info = ref["records"], pd.info
    budget = m if m >= 1 else (records if info["slices"] == 1 else None)      # (m = 0: the library's choice, known only where it took everything)
    if plan is not None and budget is not None:
        assert (info["slices"], info["sort_passes"]) == slice_plan(plan, budget), (m, info)
    if m >= 1:
        assert (info["slices"] == 1) == (m >= records), (m, info)
        assert info["peak_records"] <= max(m, largest), (m, info)
    assert 1 <= info["slices"] and info["peak_records"] <= records
    assert (info["merges"] == 0) == (info["slices"] == 1), info
    if info["slices"] == 1:
        assert info["merged_rows"] == 0 and info["peak_records"] == records
    else:
        assert info["merged_rows"] >= ref["bins"]


def _both(r, W, m, **kw):
    return ((all_bins, r.dev.pair_diagonals(r.st, W, all_bins=all_bins, max_records=m, **kw)) for all_bins in (False, True))


# ---- 1. every budget ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["clean", "same_read", "wide_entry", "long_run", "clean_k51", "shuffled"])
def test_every_budget_gives_the_lists(H, O, name):
    """A prime budget near records / 7, one record short of everything, everything, ten times everything and the library's choice; both
    lists, two widths.  wide_entry: the same keys in every slice, entries of 44 850 records each; long_run: every slice is one row with
    the same (key, bin); shuffled: one key's bin rows over several tiles of the merge, one bin's records over several slices."""
    case = _get(H, O, name)
    largest = _largest_entry(case["o"])
    with _Resident(H, case) as r:
        for W in (7, 64):
            ref, plan = _ref(case, W), sort_words(case, W)
            records = ref["records"]
            assert records > 1000 and largest < records and plan[0].shape[0] == records == plan[1][-1]
            for m in (_prime_near(records / 7), records - 1, records, 10 * records, 0):
                for all_bins, pd in _both(r, W, m):
                    _check_sliced(pd, ref, all_bins, m, largest, plan)
                    if m == records - 1:
                        assert pd.info["slices"] == 2
        if name == "wide_entry":                         # budgets below one entry: every entry is a slice of its own
            ref, plan = _ref(case, 7), sort_words(case, 7)
            for m in (1, 44849, 44850):
                for all_bins, pd in _both(r, 7, m):
                    _check_sliced(pd, ref, all_bins, m, largest, plan)
                    assert pd.info["slices"] == 30 and pd.info["peak_records"] == 44850
            for all_bins, pd in _both(r, 7, 2 * 44850):  # two entries per slice: 15 lists that all hold the same keys, 14 merges
                _check_sliced(pd, ref, all_bins, 2 * 44850, largest, plan)
                assert pd.info["slices"] == 15 and pd.info["peak_records"] == 2 * 44850 and pd.info["merges"] == 14


def test_one_record_at_a_time_few_reads(H, O):
    """The first reads of the clean case, a few hundred records: max_records = 1 -- as many slices as there are entries with records, every
    cut, every window offset and a deep merge tree."""
    from hysortk_amd import synth
    par = dict(K=31, M=17, L=2, U=50, ntasks=16, rid_base=7)
    case = _own_case(H, O, "few_reads_48", synth.reads(20000, 150, 1500, 29)[:48], par)
    ref, plan = _ref(case, 7), sort_words(case, 7)
    assert 100 <= ref["records"] <= 3000 and ref["best"].shape[0] >= 3
    with _Resident(H, case) as r:
        for all_bins, pd in _both(r, 7, 1):
            _check_sliced(pd, ref, all_bins, 1, _largest_entry(case["o"]), plan)
            assert pd.info["slices"] == int((case["o"].cnt >= 2).sum())


# ---- 2. best-bin lists are never merged ---------------------------------------------------------------------------------------------------------
def test_the_best_bin_of_a_slice_is_not_the_best_bin_of_the_range(H, O):
    """shuffled, W = 7, a budget near records / 7 (same_read under the same budget has no such key).  The precondition, on the reference:
    there is a key whose best bin among the records of the first slice that holds it differs from its best bin over the whole range -- a
    call that selected per slice and merged the selections could not give the reference's rows."""
    case, W = _get(H, O, "shuffled"), 7
    ref = _ref(case, W)
    m = _prime_near(ref["records"] / 7)
    k, v, off = entry_records(case)
    cuts = slice_cuts(off, m)
    whole = {int(row[0]): int(row[2]) for row in ref["best"]}
    seen, differ = set(), []
    for a, b in zip(cuts[:-1], cuts[1:]):
        ks, vs = k[a:b], v[a:b]
        keep = ks != 0
        ks, vs = ks[keep], vs[keep]
        kb, sup = np.unique(np.stack([ks, D.bins_of(ks, vs, W)], axis=1), axis=0, return_counts=True)
        sup = sup.astype(np.uint64)
        rows = np.stack([kb[:, 0], sup, kb[:, 1], sup, sup, sup], axis=1)
        for row in D.select(rows):
            key = int(row[0])
            if key not in seen and int(row[2]) != whole[key]:
                differ.append((key, int(row[2]), whole[key]))
            seen.add(key)
    print("slices %d; keys whose first slice has another best bin than the range: %d, e.g. %s" % (len(cuts) - 1, len(differ), differ[:3]))
    assert len(cuts) - 1 >= 7 and len(differ) >= 1
    with _Resident(H, case) as r:
        pd = r.dev.pair_diagonals(r.st, W, max_records=m)
        _check_sliced(pd, ref, False, m, _largest_entry(case["o"]))
        assert pd.info["slices"] == len(cuts) - 1
        got = {int(row[0]): int(row[2]) for row in pd.rows()}
        assert all(got[key] == best for key, _, best in differ)


# ---- 3. the clean case: task ranges, min_support, rows on the device, refusals -------------------------------------------------------------------
@pytest.fixture(scope="module")
def clean(H, O):
    with _Resident(H, _case(H, O, "clean")) as r:
        yield r


def test_sliced_task_ranges_join_on_the_device(H, O, clean):
    r, case, W = clean, clean.case, 7
    whole = _ref(case, W)
    ra, rb = _ref(case, W, task_lo=0, task_hi=8), _ref(case, W, task_lo=8, task_hi=16)
    a = r.dev.pair_diagonals(r.st, W, 0, 8, all_bins=True, max_records=_prime_near(ra["records"] / 5))
    b = r.dev.pair_diagonals(r.st, W, 8, 16, all_bins=True, max_records=_prime_near(rb["records"] / 3), on_device=True)
    with b:
        _check(a, ra, True)
        assert a.info["slices"] > 1 and b.info["slices"] > 1 and b.n == rb["all_bins"].shape[0] and b.rows_dev
        for all_bins in (True, False):
            comb = H.PairDiagonals.combine([a, b], ctx=r.c, all_bins=all_bins)
            _check(comb, whole, all_bins)
        _check(H.PairDiagonals.combine([a, b], ctx=r.c, all_bins=False, min_support=3), _ref(case, W, min_support=3), False)
    e = r.dev.pair_diagonals(r.st, W, 3, 3, max_records=5)                        # an empty range: no rows, no error
    _check(e, _ref(case, W, task_lo=3, task_hi=3), False)
    assert e.info["slices"] == 1 and e.info["merges"] == 0


@pytest.mark.parametrize("ms", [2, 5])
def test_min_support_is_applied_to_the_joined_rows(H, O, clean, ms):
    r, case, W = clean, clean.case, 7
    ref = _ref(case, W, min_support=ms)
    assert 0 < ref["best"].shape[0] < _ref(case, W)["best"].shape[0] and 0 < ref["all_bins"].shape[0] < _ref(case, W)["all_bins"].shape[0]
    for m in (_prime_near(ref["records"] / 7), _prime_near(ref["records"] / 64)):
        for all_bins, pd in _both(r, W, m, min_support=ms):
            _check_sliced(pd, ref, all_bins, m, _largest_entry(case["o"]))
            assert pd.info["slices"] > 1


def test_rows_left_on_the_device(H, O, clean):
    r, case, W = clean, clean.case, 7
    ref = _ref(case, W)
    m = _prime_near(ref["records"] / 7)
    for all_bins, host in _both(r, W, m):
        with r.dev.pair_diagonals(r.st, W, all_bins=all_bins, on_device=True, max_records=m) as d:
            assert d.n == len(host) and d.rows_dev and d.rows_dev % 16 == 0 and d.info["slices"] == host.info["slices"] > 1
            assert (d.info["records"], d.info["keys"], d.info["bins"]) == (host.info["records"], host.info["keys"], host.info["bins"])
            assert np.array_equal(r.c.d2h(d.rows_dev, d.n * 48).view(np.uint64).reshape(d.n, 6), host.rows())


def test_refusals(H, O, clean):
    """Everything hsk_result_pair_diagonals refuses, with the context usable after each."""
    from hysortk_amd import _lib
    r, case, W = clean, clean.case, 7
    c, dev, st, par = r.c, r.dev, r.st, case["par"]
    m = _prime_near(_ref(case, W)["records"] / 7)

    def works():
        _check_sliced(dev.pair_diagonals(st, W, max_records=m), _ref(case, W), False, m, _largest_entry(case["o"]))

    def refused(text, *a, **kw):
        with pytest.raises(H.HskError) as e:
            dev.pair_diagonals(*a, max_records=m, **kw)
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
    pd, sl = _lib.PairDiags(), _lib.PairsSlices()
    call = c.lib.hsk_result_pair_diagonals_sliced
    assert call(c.h, None, C.byref(st.st), 0, 16, W, 1, 0, 0, m, C.byref(pd), C.byref(sl)) == 1
    assert call(c.h, C.byref(dev.res), C.byref(st.st), 0, 16, W, 1, 0, 0, m, None, C.byref(sl)) == 1
    assert call(c.h, C.byref(dev.res), C.byref(st.st), 0, 17, W, 1, 0, 0, m, C.byref(pd), C.byref(sl)) == 1 and pd.n == 0 and sl.slices == 0
    assert call(c.h, C.byref(dev.res), C.byref(st.st), 0, 16, W, 1, 0, 0, m, C.byref(pd), None) == 0 and pd.n == _ref(case, W)["best"].shape[0]      # info may be NULL
    c.lib.hsk_pair_diags_free(c.h, C.byref(pd))
    # a resident result without EXTENSION; an EXTENSION result that was not left on the device
    packed, off, lens = case["dna"].arrays()
    kw = dict(K=par["K"], M=par["M"], L=par["L"], U=par["U"], ntasks=par["ntasks"])
    for ctx_kw in (dict(EXT=0, keep_device=True), dict(EXT=1)):
        with H.Context(**kw, **ctx_kw) as c2:
            res, pd = _lib.Result(), _lib.PairDiags()
            c2._check(c2.lib.hsk_count(c2.h, packed.ctypes.data_as(C.c_void_p), packed.size, off.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), lens.size, par["rid_base"], C.byref(res)))
            assert c2.lib.hsk_result_pair_diagonals_sliced(c2.h, C.byref(res), C.byref(st.st), 0, 1, W, 1, 0, 0, m, C.byref(pd), None) == 1 and c2.lib.hsk_last_error(c2.h)
            c2.lib.hsk_result_free(c2.h, C.byref(res))
    works()
    _check(dev.pair_diagonals(st, W), _ref(case, W), False)                        # ... and so does the unsliced call


# ---- 4. red zones, high read ids -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["clean", "same_read"])
def test_no_write_past_a_block(H, O, name):
    """Red zones behind every device block: the call fails if the expansion of a window, the plan, a merge or the selection writes past one."""
    case, W = _get(H, O, name), 7
    ref = _ref(case, W)
    with _Resident(H, case, tuning={"pool_redzone": 256}) as r:
        for m in (_prime_near(ref["records"] / 7), _prime_near(ref["records"] / 29)):
            for all_bins, pd in _both(r, W, m):
                _check_sliced(pd, ref, all_bins, m, _largest_entry(case["o"]))
                assert pd.info["slices"] > 1


def test_high_read_ids(H, O):
    """rid_base = 2^31 - nreads: bits 32 .. 62 of the key are all in use, bit 63 is still the orientation."""
    seqs, par = _seqs("few")
    par = dict(par, rid_base=(1 << 31) - len(seqs))
    case = _own_case(H, O, "few_high", seqs, par)
    with _Resident(H, case) as r:
        for W in (7, 64):
            ref = _ref(case, W)
            m = _prime_near(ref["records"] / 7)
            for all_bins, pd in _both(r, W, m):
                _check_sliced(pd, ref, all_bins, m, _largest_entry(case["o"]), sort_words(case, W))
                assert pd.info["slices"] > 1
    assert int(pd.rid_b.max()) == (1 << 31) - 1 and 0 < int(pd.opposite.sum()) < len(pd)
