"""hsk_result_pairs (include/hsk.h): the read pairs that share k-mers, computed on the GPU from a resident EXTENSION result, against the
definition applied in numpy to the CPU oracle's EXTENSION result of the same reads (same K, M, L, U, ntasks, rid_base).  Everything is
integer work: rows, n, records, self_records and keys are compared exactly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U32 = np.uint64(0xFFFFFFFF)


@pytest.fixture(scope="module")
def O():
    from oracle import hsk_oracle
    return hsk_oracle


@pytest.fixture(scope="module")
def H():
    import hysortk_amd
    return hysortk_amd


_TRIU = {}


def _triu(c):
    if c not in _TRIU:
        _TRIU[c] = np.triu_indices(c, 1)
    return _TRIU[c]


def reference(o, task_lo=0, task_hi=None, min_shared=1):
    """The definition, on an oracle EXTENSION result: (rows [n, 4] uint64, records, self_records, keys)."""
    nt = len(o.task_off) - 1
    a, b = int(o.task_off[task_lo]), int(o.task_off[nt if task_hi is None else task_hi])
    cnt = o.cnt[a:b].astype(np.int64)
    rid = o.rid.astype(np.int64).astype(np.uint64) & U32           # read ids as unsigned 32-bit numbers
    pos = o.pos.astype(np.uint64)
    ks, vs, records = [], [], 0
    for e in a + np.flatnonzero(cnt >= 2):
        c, p0 = int(o.cnt[e]), int(o.payoff[e])
        i, j = _triu(c)
        ra, rb, pa, pb = rid[p0 + i], rid[p0 + j], pos[p0 + i], pos[p0 + j]
        sw = ra > rb
        ra, rb, pa, pb = np.where(sw, rb, ra), np.where(sw, ra, rb), np.where(sw, pb, pa), np.where(sw, pa, pb)
        keep = ra != rb
        records += i.size
        ks.append(((ra << np.uint64(32)) | rb)[keep]); vs.append(((pa << np.uint64(32)) | pb)[keep])
    k = np.concatenate(ks) if ks else np.zeros(0, np.uint64)
    v = np.concatenate(vs) if vs else np.zeros(0, np.uint64)
    order = np.lexsort((v, k))
    k, v = k[order], v[order]
    uk, start, shared = np.unique(k, return_index=True, return_counts=True)
    rows = np.stack([uk, shared.astype(np.uint64), v[start], v[start + shared - 1]], axis=1) if uk.size else np.zeros((0, 4), np.uint64)
    return rows[rows[:, 1] >= np.uint64(min_shared)], records, records - int(k.size), int(uk.size)


def distinct_keys(ref):
    """The distinct record keys of a reference computed with min_shared = 1; a pair inside one read is a record with the key 0."""
    rows, records, self_records, keys = ref
    assert rows.shape[0] == keys
    return np.concatenate([np.zeros(1 if self_records else 0, np.uint64), rows[:, 0]])


def sort_passes_of(words, radix_bits=8):
    """The scatter passes of the key sort, from the distinct record keys ([n] or [n, NW] uint64, word 0 first): the digits of
    make_pass_plan(32 NW, NW, radix_bits) (hsk_passplan.h: every word from bit 0 up in digits of radix_bits bits, the last digit of a word
    the narrower one) in which the records do not all hold the same value.  No record or one key: 0."""
    w = np.asarray(words, np.uint64)
    w = w.reshape(w.shape[0], -1)
    passes = 0
    for col in w.T:
        lo = 0
        while lo < 64:
            bits = min(radix_bits, 64 - lo)
            d = (col >> np.uint64(lo)) & np.uint64((1 << bits) - 1)
            passes += int(d.size > 0 and bool(np.any(d != d[0])))
            lo += bits
    return passes


def _check(rp, ref):
    rows, records, self_records, keys = ref
    assert rp.info["records"] == records and rp.info["self_records"] == self_records and rp.info["keys"] == keys
    assert len(rp) == rows.shape[0]
    assert np.array_equal(rp.rows(), rows)


_CASES = {}


def _case(H, O, name):
    """(reads, parameters, oracle result) of a named input, built once."""
    if name in _CASES:
        return _CASES[name]
    from hysortk_amd import synth
    par = dict(K=31, M=17, L=2, U=50, ntasks=16, rid_base=7)
    if name == "clean":
        seqs = synth.reads(20000, 150, 1500, 29)
    elif name == "same_read":
        rng = np.random.default_rng(5)
        unit = "".join(rng.choice(list("ACGT"), 37))
        seqs = synth.reads(20000, 150, 1500, 29) + [(unit * 6)[:200]] * 3 + ["".join(rng.choice(list("ACGT"), 40)) + unit * 4 for _ in range(2)]
    elif name == "k51":
        seqs = synth.reads(20000, 150, 1500, 31); par.update(K=51)
    elif name == "k77":
        seqs = synth.reads(20000, 200, 1200, 33); par.update(K=77)
    elif name == "short":
        seqs = synth.reads(3000, 60, 400, 3) + ["ACGT" * 3, "A" * 20, ""]; par.update(K=21, M=9, U=40, ntasks=5)
    elif name == "sparse":
        seqs = synth.reads(2_000_000, 150, 1500, 1); par.update(L=1)
    elif name == "wide_entry":
        rng = np.random.default_rng(7)
        seqs = ["".join(rng.choice(list("ACGT"), 60))] * 300; par.update(U=1000, ntasks=4, rid_base=0)
    elif name == "long_run":
        rng = np.random.default_rng(9)
        seqs = ["".join(rng.choice(list("ACGT"), 20000))] * 2; par.update(ntasks=4, rid_base=0)
    elif name == "high_rid":
        seqs = synth.reads(20000, 150, 1500, 29); par.update(rid_base=2_000_000_000)
    else:
        raise KeyError(name)
    dna = H.DnaBuffer.from_sequences(seqs)
    packed, off, lens = dna.arrays()
    o = O.count(packed, off, lens, k=par["K"], m=par["M"], L=par["L"], U=par["U"], ext=1, ntasks=par["ntasks"], rid_base=par["rid_base"])
    _CASES[name] = (dna, par, o)
    return _CASES[name]


def _pairs(H, dna, par, tuning=None, **kw):
    with H.Context(K=par["K"], M=par["M"], L=par["L"], U=par["U"], EXT=1, ntasks=par["ntasks"], keep_device=True, tuning=tuning) as c:
        with c.count_resident(dna, rid_base=par["rid_base"]) as dev:
            return dev.pairs(**kw)


@pytest.fixture(scope="module")
def clean(H, O):
    """The clean case counted once and left on the device: (context, DeviceResult, oracle result)."""
    dna, par, o = _case(H, O, "clean")
    c = H.Context(K=par["K"], M=par["M"], L=par["L"], U=par["U"], EXT=1, ntasks=par["ntasks"], keep_device=True)
    dev = c.count_resident(dna, rid_base=par["rid_base"])
    yield c, dev, o
    dev.close()
    c.close()


def test_clean_reads(H, O, clean):
    """Every task non-empty, no pair inside one read."""
    c, dev, o = clean
    ref = reference(o)
    assert ref[1] > 100000 and ref[0].shape[0] > 1000 and int(ref[0][:, 1].max()) > 50 and ref[2] == 0
    rp = dev.pairs()
    _check(rp, ref)
    assert 1 <= rp.info["sort_passes"] <= 8 and rp.info["ms_total"] > 0
    assert rp.info["sort_passes"] == sort_passes_of(distinct_keys(ref))
    assert np.array_equal(rp.rid_a.astype(np.uint64) << np.uint64(32) | rp.rid_b.astype(np.uint64), rp.key) and np.all(rp.rid_a < rp.rid_b)
    assert np.array_equal(rp.first_pos_a.astype(np.uint64) << np.uint64(32) | rp.first_pos_b.astype(np.uint64), rp.first)
    assert np.array_equal(rp.last_pos_a.astype(np.uint64) << np.uint64(32) | rp.last_pos_b.astype(np.uint64), rp.last)


def test_kmers_twice_in_one_read(H, O):
    """Reads made of a repeated unit: occurrence pairs inside one read are counted and dropped; runs of several hundred records."""
    dna, par, o = _case(H, O, "same_read")
    ref = reference(o)
    assert ref[2] > 100 and int(ref[0][:, 1].max()) > 300
    _check(_pairs(H, dna, par), ref)


@pytest.mark.parametrize("name", ["k51", "k77"])
def test_key_widths(H, O, name):
    """Entries of two and three key words: the stage reads (nw + 1)-word records."""
    dna, par, o = _case(H, O, name)
    ref = reference(o)
    assert ref[0].shape[0] > 100
    _check(_pairs(H, dna, par), ref)


def test_short_and_odd_reads(H, O):
    """Reads shorter than K and an empty read."""
    dna, par, o = _case(H, O, "short")
    ref = reference(o)
    assert ref[0].shape[0] > 0
    _check(_pairs(H, dna, par), ref)


def test_mostly_entries_without_records(H, O):
    """Coverage 0.1 with L = 1: nearly every entry has cnt == 1 and no record -- long runs of equal offsets in the expansion's searches."""
    dna, par, o = _case(H, O, "sparse")
    ref = reference(o)
    assert int((o.cnt == 1).sum()) > 0.9 * o.cnt.size and o.cnt.size > 100000
    assert 1 <= ref[0].shape[0] <= 500
    _check(_pairs(H, dna, par), ref)


def test_one_entry_over_many_tiles(H, O):
    """300 copies of one read: 30 entries of 300 occurrences, 44 850 records each -- an entry far larger than a tile, the decode at three-digit j."""
    dna, par, o = _case(H, O, "wide_entry")
    ref = reference(o)
    rows = ref[0]
    assert o.cnt.size == 30 and np.all(o.cnt == 300) and ref[1] == 30 * 44850 and ref[2] == 0
    assert rows.shape[0] == 44850 and np.all(rows[:, 1] == 30) and np.all(rows[:, 2] == 0) and np.all(rows[:, 3] == (np.uint64(29) << np.uint64(32) | np.uint64(29)))
    _check(_pairs(H, dna, par), ref)


def test_one_run_over_many_tiles(H, O):
    """Two copies of one long read: a single row whose run of equal keys crosses the reducer's tiles."""
    dna, par, o = _case(H, O, "long_run")
    ref = reference(o)
    assert ref[0].tolist() == [[1, 19970, 0, (19969 << 32) | 19969]]
    _check(_pairs(H, dna, par), ref)


def test_high_read_ids(H, O):
    """rid_base = 2 * 10^9: read ids that use 31 bits, so the upper digits of both key halves are no longer trivial and the sort takes more
    passes.  (The ids stay below 2^31: ids that are negative as int32 are not covered here.)"""
    dna, par, o = _case(H, O, "high_rid")
    ref = reference(o)
    assert int(ref[0][0, 0] >> np.uint64(32)) >= 2_000_000_000
    rp = _pairs(H, dna, par)
    _check(rp, ref)
    assert int(rp.rid_a.min()) >= 2_000_000_000
    assert rp.info["sort_passes"] == sort_passes_of(distinct_keys(ref))


def test_task_ranges_combine(H, O, clean):
    """Disjoint task ranges: each equals the definition on its tasks, an empty range is an empty list, and ReadPairs.combine of the parts is
    the list of the whole (the multi-rank contract)."""
    c, dev, o = clean
    a, b = dev.pairs(0, 5), dev.pairs(5, 16)
    _check(a, reference(o, 0, 5))
    _check(b, reference(o, 5, 16))
    e = dev.pairs(3, 3)
    assert len(e) == 0 and e.info["records"] == 0 and e.info["keys"] == 0
    whole = reference(o)
    for ms in (1, 3):
        comb = H.ReadPairs.combine([a, b, e], min_shared=ms)
        assert np.array_equal(comb.rows(), whole[0][whole[0][:, 1] >= np.uint64(ms)])
    assert comb.info["records"] == whole[1] and comb.info["keys"] == whole[3]


@pytest.mark.parametrize("min_shared", [2, 50])
def test_min_shared(H, O, clean, min_shared):
    c, dev, o = clean
    ref = reference(o, min_shared=min_shared)
    assert 0 < ref[0].shape[0] < ref[3]
    _check(dev.pairs(min_shared=min_shared), ref)


def test_rows_left_on_the_device(H, O, clean):
    c, dev, o = clean
    host = dev.pairs()
    with dev.pairs(on_device=True) as d:
        assert d.n == len(host) and d.rows_dev and d.info["records"] == host.info["records"]
        rows = c.d2h(d.rows_dev, d.n * 32).view(np.uint64).reshape(d.n, 4)
        assert np.array_equal(rows, host.rows())


@pytest.mark.parametrize("name", ["clean", "same_read"])
def test_no_write_past_a_block(H, O, name):
    """Red zones behind every device block: the call fails if a kernel of the stage writes past one."""
    dna, par, o = _case(H, O, name)
    _check(_pairs(H, dna, par, tuning={"pool_redzone": 256}), reference(o))


def test_refusals(H, O):
    dna, par, o = _case(H, O, "clean")
    kw = dict(K=par["K"], M=par["M"], L=par["L"], U=par["U"], ntasks=par["ntasks"])
    from hysortk_amd import _lib
    import ctypes as C
    packed, off, lens = dna.arrays()

    def raw_count(c):
        res = _lib.Result()
        c._check(c.lib.hsk_count(c.h, packed.ctypes.data_as(C.c_void_p), packed.size, off.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), lens.size, par["rid_base"], C.byref(res)))
        return res

    # a host result (EXTENSION, not left on the device); a resident result without EXTENSION
    for ctx_kw in (dict(EXT=1), dict(EXT=0, keep_device=True)):
        with H.Context(**kw, **ctx_kw) as c:
            res, pr = raw_count(c), _lib.Pairs()
            assert c.lib.hsk_result_pairs(c.h, C.byref(res), 0, par["ntasks"], 1, 0, C.byref(pr)) == 1
            assert c.lib.hsk_last_error(c.h)
            c.lib.hsk_result_free(c.h, C.byref(res))
    with H.Context(**kw, EXT=1, keep_device=True) as c:
        with c.count_resident(dna, rid_base=par["rid_base"]) as dev:
            for bad in (dict(task_hi=par["ntasks"] + 1), dict(task_lo=-1), dict(task_lo=4, task_hi=3), dict(min_shared=0)):
                with pytest.raises(H.HskError) as e:
                    dev.pairs(**bad)
                assert e.value.status == 1
            _check(dev.pairs(), reference(o))                 # the context works afterwards
        with c.count_resident(dna, rid_base=par["rid_base"]) as dev:
            _check(dev.pairs(min_shared=2), reference(o, min_shared=2))
