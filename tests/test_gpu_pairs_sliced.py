"""hsk_result_pairs_sliced (include/hsk.h): the read pairs of a resident EXTENSION result from at most max_records records expanded at a
time -- the slice planner (hsk_pairplan.h), the window arguments of the expansion and the merges of the slices' row lists
(hsk_rowmerge.h) -- against the definition applied in numpy to the CPU oracle's result (tests/test_gpu_pairs.py: reference).  Everything
is integer work and compared exactly, whatever the budget."""
import numpy as np
import pytest

from tests.test_gpu_pairs import U32, _case, _check, _triu, reference, sort_passes_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def O():
    from oracle import hsk_oracle
    return hsk_oracle


@pytest.fixture(scope="module")
def H():
    import hysortk_amd
    return hysortk_amd


_REF = {}


def _ref(o, name, **kw):
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _REF:
        _REF[key] = reference(o, **kw)
    return _REF[key]


def _prime_near(n):
    n = max(int(n), 2)
    while any(n % d == 0 for d in range(2, int(n ** 0.5) + 1)):
        n += 1
    return n


def _largest_entry(o):
    c = int(o.cnt.max()) if o.cnt.size else 0
    return c * (c - 1) // 2


def _open(H, par, tuning=None):
    return H.Context(K=par["K"], M=par["M"], L=par["L"], U=par["U"], EXT=1, ntasks=par["ntasks"], keep_device=True, tuning=tuning)


def entry_records(o, strand=None):
    """The record keys of the whole range in the order of the expansion, entry by entry (a pair inside one read is the key 0; with the strand of
    every payload slot, bit 63 is the relative strand), and the record offset of every entry that has records, the total last."""
    rid = o.rid.astype(np.int64).astype(np.uint64) & U32
    sb = None if strand is None else strand.astype(np.uint64)
    ks, off = [np.zeros(0, np.uint64)], [0]
    for e in np.flatnonzero(o.cnt >= 2):
        i, j = _triu(int(o.cnt[e]))
        si, sj = int(o.payoff[e]) + i, int(o.payoff[e]) + j
        ra, rb = np.minimum(rid[si], rid[sj]), np.maximum(rid[si], rid[sj])
        k = (ra << np.uint64(32)) | rb
        if sb is not None:
            k |= (sb[si] ^ sb[sj]) << np.uint64(63)
        ks.append(np.where(ra == rb, np.uint64(0), k)); off.append(off[-1] + i.size)
    return np.concatenate(ks), np.array(off, np.int64)


def slice_plan(recs, budget):
    """(slices that hold records, the most scatter passes any slice's sort takes) under the planner's rule (hsk_pairplan.h): a slice takes
    entries while its records stay within the budget, and an entry above the budget is a slice of its own.  Entries without records join
    a neighbour and change no record set."""
    keys, off = recs
    slices, passes, a = 0, 0, 0
    while a + 1 < off.size:
        b = max(int(np.searchsorted(off, off[a] + budget, side="right")) - 1, a + 1)
        slices += 1; passes = max(passes, sort_passes_of(keys[off[a]:off[b]]))
        a = b
    return slices, passes


def _check_sliced(rp, ref, m, largest, recs=None):
    """recs: entry_records() of the range.  sort_passes is the most over the slices' sorts, each over the records of its cut."""
    _check(rp, ref)                                       # rows, n, records, self_records, keys
    records, info = ref[1], rp.info
    budget = m if m >= 1 else (records if info["slices"] == 1 else None)      # (m = 0: the library's choice, known only where it took everything)
    if recs is not None and budget is not None:
        assert (info["slices"], info["sort_passes"]) == slice_plan(recs, budget), (m, info)
    if m >= 1:
        assert (info["slices"] == 1) == (m >= records), (m, info)
        assert info["peak_records"] <= max(m, largest), (m, info)
    assert 1 <= info["slices"] and info["peak_records"] <= records
    if info["slices"] == 1:
        assert info["merges"] == 0 and info["merged_rows"] == 0 and info["peak_records"] == records
    else:
        assert info["merges"] >= 1 and info["merged_rows"] >= len(rp)


@pytest.mark.parametrize("name", ["clean", "same_read", "k51", "sparse", "wide_entry", "long_run"])
def test_every_budget_gives_the_list(H, O, name):
    """A prime budget near records / 7, one record short of everything, everything, ten times everything and the library's choice.
    wide_entry: the same 44 850 keys in every slice, entries of 44 850 records each; long_run: every slice is one row with the same key;
    sparse: the cuts fall into long runs of entries without records."""
    dna, par, o = _case(H, O, name)
    ref = _ref(o, name)
    records, largest, recs = ref[1], _largest_entry(o), entry_records(o)
    assert records > 1000 and largest < records
    with _open(H, par) as c:
        with c.count_resident(dna, rid_base=par["rid_base"]) as dev:
            for m in (_prime_near(records / 7), records - 1, records, 10 * records, 0):
                rp = dev.pairs(max_records=m)
                _check_sliced(rp, ref, m, largest, recs)
                if m == records - 1:
                    assert rp.info["slices"] == 2
            if name == "wide_entry":                     # budgets below one entry: every entry is a slice of its own
                for m in (1, 44849, 44850, 2 * 44850 - 1):
                    rp = dev.pairs(max_records=m)
                    _check_sliced(rp, ref, m, largest, recs)
                    assert rp.info["slices"] == 30 and rp.info["peak_records"] == 44850
                # two entries per slice: 15 lists of the same 44 850 keys, 14 merges of two such lists each
                rp = dev.pairs(max_records=2 * 44850)
                _check_sliced(rp, ref, 2 * 44850, largest, recs)
                assert rp.info["slices"] == 15 and rp.info["peak_records"] == 2 * 44850
                assert rp.info["merges"] == 14 and rp.info["merged_rows"] == 14 * 2 * 44850


def test_one_record_at_a_time_short_reads(H, O):
    """max_records = 1: as many slices as there are entries with records -- every cut, every window offset and a deep merge tree."""
    dna, par, o = _case(H, O, "short")
    ref = _ref(o, "short")
    with _open(H, par) as c:
        with c.count_resident(dna, rid_base=par["rid_base"]) as dev:
            rp = dev.pairs(max_records=1)
            _check_sliced(rp, ref, 1, _largest_entry(o), entry_records(o))
            assert rp.info["slices"] == int((o.cnt >= 2).sum())


def test_one_record_at_a_time_few_reads(H, O):
    """The first reads of the clean case, a few hundred records: max_records = 1, 2 and 3."""
    from hysortk_amd import synth
    par = dict(K=31, M=17, L=2, U=50, ntasks=16, rid_base=7)
    dna = H.DnaBuffer.from_sequences(synth.reads(20000, 150, 1500, 29)[:48])
    packed, off, lens = dna.arrays()
    o = O.count(packed, off, lens, k=par["K"], m=par["M"], L=par["L"], U=par["U"], ext=1, ntasks=par["ntasks"], rid_base=par["rid_base"])
    ref = reference(o)
    assert 100 <= ref[1] <= 3000 and ref[0].shape[0] >= 3
    with _open(H, par) as c:
        with c.count_resident(dna, rid_base=par["rid_base"]) as dev:
            for m in (1, 2, 3):
                rp = dev.pairs(max_records=m)
                _check_sliced(rp, ref, m, _largest_entry(o), entry_records(o))
            assert dev.pairs(max_records=1).info["slices"] == int((o.cnt >= 2).sum())


@pytest.fixture(scope="module")
def clean(H, O):
    dna, par, o = _case(H, O, "clean")
    c = _open(H, par)
    dev = c.count_resident(dna, rid_base=par["rid_base"])
    yield c, dev, o
    dev.close()
    c.close()


@pytest.mark.parametrize("min_shared", [2, 50])
def test_min_shared_is_applied_to_the_joined_rows(H, O, clean, min_shared):
    c, dev, o = clean
    ref = _ref(o, "clean", min_shared=min_shared)
    assert 0 < ref[0].shape[0] < ref[3]
    for m in (_prime_near(ref[1] / 7), _prime_near(ref[1] / 64)):
        rp = dev.pairs(min_shared=min_shared, max_records=m)
        _check_sliced(rp, ref, m, _largest_entry(o))
        assert rp.info["slices"] > 1


def test_task_sub_range(H, O, clean):
    c, dev, o = clean
    ref = _ref(o, "clean", task_lo=5, task_hi=16)
    largest = _largest_entry(o)                          # (of all tasks: no smaller than the sub-range's)
    for m in (_prime_near(ref[1] / 7), ref[1] - 1, ref[1], 0):
        rp = dev.pairs(5, 16, max_records=m)
        _check_sliced(rp, ref, m, largest)
    e = dev.pairs(3, 3, max_records=5)
    assert len(e) == 0 and e.info["records"] == 0 and e.info["keys"] == 0 and e.info["slices"] == 1


def test_rows_left_on_the_device(H, O, clean):
    c, dev, o = clean
    ref = _ref(o, "clean")
    m = _prime_near(ref[1] / 7)
    host = dev.pairs(max_records=m)
    _check(host, ref)
    with dev.pairs(on_device=True, max_records=m) as d:
        assert d.n == len(host) and d.rows_dev and d.info["records"] == host.info["records"] and d.info["slices"] == host.info["slices"] > 1
        rows = c.d2h(d.rows_dev, d.n * 32).view(np.uint64).reshape(d.n, 4)
        assert np.array_equal(rows, host.rows())


@pytest.mark.parametrize("name", ["clean", "same_read"])
def test_no_write_past_a_block(H, O, name):
    """Red zones behind every device block: the call fails if the expansion of a window, the plan or a merge writes past one."""
    dna, par, o = _case(H, O, name)
    ref = _ref(o, name)
    with _open(H, par, tuning={"pool_redzone": 256}) as c:
        with c.count_resident(dna, rid_base=par["rid_base"]) as dev:
            for m in (_prime_near(ref[1] / 7), _prime_near(ref[1] / 29)):
                rp = dev.pairs(max_records=m)
                _check_sliced(rp, ref, m, _largest_entry(o))


def test_refusals(H, O, clean):
    c, dev, o = clean
    ref = _ref(o, "clean")
    for bad in (dict(min_shared=0), dict(task_hi=17), dict(task_lo=-1), dict(task_lo=4, task_hi=3)):
        with pytest.raises(H.HskError) as e:
            dev.pairs(max_records=1000, **bad)
        assert e.value.status == 1
    m = _prime_near(ref[1] / 7)
    _check_sliced(dev.pairs(max_records=m), ref, m, _largest_entry(o))        # the context works afterwards
    _check(dev.pairs(), ref)                                                   # ... and so does the unsliced call
