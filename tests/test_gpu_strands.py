"""hsk_result_strands and hsk_result_pairs_oriented (include/hsk.h): the strand of every k-mer occurrence of a resident EXTENSION result,
recovered from the reads, and the read pairs split by the relative strand of the two occurrences -- against the definitions applied in
numpy to the CPU oracle's EXTENSION result of the same reads (tests/oriented_ref.py), and against a geometry built by hand.  Everything is
integer work and compared exactly.  The inputs are those of tests/test_gpu_pairs.py (1500 reads of 150 bases from a 20 000-base genome,
L = 2, U = 50, 16 tasks, rid_base = 7, unless a case says otherwise)."""
import ctypes as C

import numpy as np
import pytest

from tests import oriented_ref as R
from tests.test_gpu_pairs import distinct_keys, sort_passes_of
from tests.test_gpu_pairs_sliced import entry_records, slice_plan

pytestmark = pytest.mark.gpu

TOP = np.uint64(1) << np.uint64(63)


@pytest.fixture(scope="module")
def O():
    from oracle import hsk_oracle
    return hsk_oracle


@pytest.fixture(scope="module")
def H():
    import hysortk_amd
    return hysortk_amd


_CASES = {}


def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _seqs(name):
    """The reads and parameters of a named input (clean, same_read, wide_entry, long_run: the constructions of tests/test_gpu_pairs.py)."""
    from hysortk_amd import synth
    par = dict(K=31, M=17, L=2, U=50, ntasks=16, rid_base=7)
    if name == "clean":
        seqs = synth.reads(20000, 150, 1500, 29)
    elif name == "clean_k51":
        seqs = synth.reads(20000, 150, 1500, 29); par.update(K=51)
    elif name == "k77":
        seqs = synth.reads(20000, 200, 1200, 33); par.update(K=77)
    elif name == "gaps":                                  # the clean reads under L = 15, U = 40: filtered entries leave gaps in the payload
        seqs = synth.reads(20000, 150, 1500, 29); par.update(L=15, U=40)
    elif name == "same_read":
        rng = np.random.default_rng(5)
        unit = "".join(rng.choice(list("ACGT"), 37))
        seqs = synth.reads(20000, 150, 1500, 29) + [(unit * 6)[:200]] * 3 + ["".join(rng.choice(list("ACGT"), 40)) + unit * 4 for _ in range(2)]
    elif name == "wide_entry":
        rng = np.random.default_rng(7)
        seqs = ["".join(rng.choice(list("ACGT"), 60))] * 300; par.update(U=1000, ntasks=4, rid_base=0)
    elif name == "long_run":
        rng = np.random.default_rng(9)
        seqs = ["".join(rng.choice(list("ACGT"), 20000))] * 2; par.update(ntasks=4, rid_base=0)
    elif name == "even_k":                                # K = 22: k-mers that are their own reverse complement, reads shorter than K, an empty read
        seqs = synth.reads(3000, 60, 400, 3) + ["ACGT" * 15] * 4 + ["A" * 20, ""]; par.update(K=22, M=9, U=40, ntasks=5)
    elif name == "few":                                   # the first 200 reads of the clean case
        seqs = synth.reads(20000, 150, 1500, 29)[:200]
    elif name == "geometry":
        rng = np.random.default_rng(11)
        g = "".join(rng.choice(list("ACGT"), 5000))
        seqs = [g[1000:1300], g[1100:1250], _revcomp(g[1100:1250])] + synth.reads(20000, 150, 50, 77); par.update(rid_base=0)
    else:
        raise KeyError(name)
    return seqs, par


def _case(H, O, name):
    """A named input, built once: reads, parameters, the oracle's result, the strand of every oracle payload and the lookup by (rid, pos)."""
    if name not in _CASES:
        seqs, par = _seqs(name)
        dna = H.DnaBuffer.from_sequences(seqs)
        packed, off, lens = dna.arrays()
        o = O.count(packed, off, lens, k=par["K"], m=par["M"], L=par["L"], U=par["U"], ext=1, ntasks=par["ntasks"], rid_base=par["rid_base"])
        strand = R.payload_strands(o, seqs, par["K"], par["rid_base"])[0]
        _CASES[name] = dict(seqs=seqs, par=par, dna=dna, o=o, strand=strand, lookup=R.strand_lookup(o, seqs, par["K"], par["rid_base"]), ref={})
    return _CASES[name]


def _ref(case, **kw):
    key = tuple(sorted(kw.items()))
    if key not in case["ref"]:
        case["ref"][key] = R.oriented_reference(case["o"], case["strand"], **kw)
    return case["ref"][key]


def _open(H, par, tuning=None, **kw):
    return H.Context(K=par["K"], M=par["M"], L=par["L"], U=par["U"], EXT=1, ntasks=par["ntasks"], keep_device=True, tuning=tuning, **kw)


def _check_bits(dev, st, case):
    """Every task's bits against the definition; payloads, reverse and palindromes exact.  Returns the number of gap slots."""
    key, s, payloads, reverse, palindromes = case["lookup"]
    assert st.info["ntasks"] == dev.ntasks
    print("strands: payloads %d (reference %d), reverse %d (%d), palindromes %d (%d)" % (st.info["payloads"], payloads, st.info["reverse"], reverse, st.info["palindromes"], palindromes))
    assert (st.info["payloads"], st.info["reverse"], st.info["palindromes"]) == (payloads, reverse, palindromes)
    gaps = 0
    for t in range(dev.ntasks):
        f = dev.fetch(t)
        want, g = R.task_bits(f, case["lookup"]) if f["npay"] else (np.zeros(0, bool), 0)
        got = st.task_bits(t)
        assert got.shape == want.shape and np.array_equal(got, want), "task %d" % t
        gaps += g
    return gaps


def _check_rows(rp, ref):
    rows, records, self_records, keys = ref
    print("oriented: records %d (reference %d), self %d (%d), keys %d (%d), rows %d (%d)" % (rp.info["records"], records, rp.info["self_records"], self_records, rp.info["keys"], keys, len(rp), rows.shape[0]))
    assert rp.info["records"] == records and rp.info["self_records"] == self_records and rp.info["keys"] == keys
    assert rp.oriented and len(rp) == rows.shape[0]
    assert np.array_equal(rp.rows(), rows)
    opp = (rp.key & TOP) != 0
    assert np.array_equal(rp.opposite, opp) and np.all(rp.rid_a < rp.rid_b)
    for half in (rp.key[~opp], rp.key[opp]):              # same-strand rows first, each half strictly ascending
        assert np.all(half[1:] > half[:-1])
    assert np.all(~opp[:int((~opp).sum())])


@pytest.fixture(scope="module")
def clean(H, O):
    """The clean case counted once and left on the device, with its strands: (context, DeviceResult, Strands, case)."""
    case = _case(H, O, "clean")
    c = _open(H, case["par"])
    dev = c.count_resident(case["dna"], rid_base=case["par"]["rid_base"])
    st = dev.strands(case["dna"], rid_base=case["par"]["rid_base"])
    yield c, dev, st, case
    st.close()
    dev.close()
    c.close()


# ---- 1. strand bits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["clean", "clean_k51", "k77", "gaps"])
def test_strand_bits_equal_the_reference(H, O, name):
    """Keys of one, two and three words; under L = 15, U = 40 the filtered entries leave gap slots, whose bit is 0."""
    case = _case(H, O, name)
    par = case["par"]
    with _open(H, par) as c:
        with c.count_resident(case["dna"], rid_base=par["rid_base"]) as dev:
            with dev.strands(case["dna"], rid_base=par["rid_base"]) as st:
                gaps = _check_bits(dev, st, case)
                assert st.info["payloads"] > 10000 and 0.3 < st.info["reverse"] / st.info["payloads"] < 0.7      # the synthetic reads are 50/50 by strand
                assert st.info["palindromes"] == 0 and st.info["ms_total"] > 0
                if name == "gaps":
                    assert gaps >= 1
                    assert sum(int(dev.task(t)["npay"]) for t in range(dev.ntasks)) == st.info["payloads"] + gaps


# ---- 2. even K ---------------------------------------------------------------------------------------------------------------------------
def test_even_k_with_palindromes(H, O):
    case = _case(H, O, "even_k")
    par = case["par"]
    with _open(H, par) as c:
        with c.count_resident(case["dna"], rid_base=par["rid_base"]) as dev:
            with dev.strands(case["dna"], rid_base=par["rid_base"]) as st:
                _check_bits(dev, st, case)
                assert st.info["palindromes"] > 0


# ---- 3. reads in HBM and on the host -------------------------------------------------------------------------------------------------------
def test_reads_in_hbm_and_on_the_host_give_the_same_bits(H, O):
    """The clean reads as hsk_synth_reads leaves them in HBM (a DeviceDna) and as a DnaBuffer whose packed array has exactly the reads' bytes:
    the last read's last k-mer ends in the buffer's last byte."""
    from hysortk_amd import synth
    case = _case(H, O, "clean")
    par, o = case["par"], case["o"]
    packed, off, lens = case["dna"].arrays()
    assert packed.size == int(off[-1]) + (int(lens[-1]) + 3) // 4 == sum((len(s) + 3) // 4 for s in case["seqs"])
    last = par["rid_base"] + len(case["seqs"]) - 1
    owned = R.payload_strands(o, case["seqs"], par["K"], par["rid_base"])[1]
    assert np.any(owned & (o.rid == last) & (o.pos == len(case["seqs"][-1]) - par["K"])), "the last read's last k-mer is not retained"
    with _open(H, par) as c:
        dp, nb, do, dl = c.synth_reads(20000, 150, 1500, 29)
        ddna = H.DeviceDna(c, dp, nb, do, dl, 1500, par["rid_base"])
        assert np.array_equal(ddna.packed(), packed) and case["seqs"] == synth.reads(20000, 150, 1500, 29)
        with ddna.count_resident_device() as dev:
            with dev.strands(ddna) as sd, dev.strands(case["dna"], rid_base=par["rid_base"]) as sh:
                _check_bits(dev, sd, case)
                for t in range(dev.ntasks):
                    assert np.array_equal(sd.task_bits(t), sh.task_bits(t))
                assert sd.info["reverse"] == sh.info["reverse"] and sd.info["payloads"] == sh.info["payloads"]
        ddna.free()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(H, O, clean):
    from hysortk_amd import _lib, synth
    c, dev, st, case = clean
    par = case["par"]
    packed, off, lens = case["dna"].arrays()

    def works():
        with dev.strands(case["dna"], rid_base=par["rid_base"]) as s:
            _check_bits(dev, s, case)

    other = H.DnaBuffer.from_sequences(synth.reads(20000, 150, 1500, 30))
    with pytest.raises(H.HskError) as e:
        dev.strands(other, rid_base=par["rid_base"])
    assert e.value.status == 1 and "not the reads" in str(e.value)
    works()
    with pytest.raises(H.HskError) as e:                  # one read short: the last read's payloads name a read that was not given
        dev.strands((packed, off[:-1], lens[:-1]), rid_base=par["rid_base"])
    assert e.value.status == 1 and "outside" in str(e.value)
    works()
    with pytest.raises(H.HskError) as e:
        dev.strands(case["dna"], rid_base=2_147_483_000)
    assert e.value.status == 1 and "2^31" in str(e.value)
    works()
    with pytest.raises(H.HskError) as e:                  # a NULL pointer
        c._check(c.lib.hsk_result_strands(c.h, C.byref(dev.res), None, packed.size, off.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), lens.size, par["rid_base"], 0, C.byref(_lib.Strands())))
    assert e.value.status == 1 and "NULL" in str(e.value)
    works()
    # a resident result without EXTENSION; an EXTENSION result that was not left on the device
    kw = dict(K=par["K"], M=par["M"], L=par["L"], U=par["U"], ntasks=par["ntasks"])
    for ctx_kw in (dict(EXT=0, keep_device=True), dict(EXT=1)):
        with H.Context(**kw, **ctx_kw) as c2:
            res, s2 = _lib.Result(), _lib.Strands()
            c2._check(c2.lib.hsk_count(c2.h, packed.ctypes.data_as(C.c_void_p), packed.size, off.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), lens.size, par["rid_base"], C.byref(res)))
            rc = c2.lib.hsk_result_strands(c2.h, C.byref(res), packed.ctypes.data_as(C.c_void_p), packed.size, off.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), lens.size, par["rid_base"], 0, C.byref(s2))
            assert rc == 1 and c2.lib.hsk_last_error(c2.h)
            c2.lib.hsk_result_free(c2.h, C.byref(res))
    works()


# ---- 5. oriented rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["clean", "same_read", "wide_entry", "long_run", "clean_k51"])
def test_oriented_rows_equal_the_reference(H, O, name):
    case = _case(H, O, name)
    par = case["par"]
    ref = _ref(case)
    with _open(H, par) as c:
        with c.count_resident(case["dna"], rid_base=par["rid_base"]) as dev:
            with dev.strands(case["dna"], rid_base=par["rid_base"]) as st:
                rp = dev.pairs(strands=st)
                _check_rows(rp, ref)
                assert rp.info["slices"] == 1
    if name == "same_read":
        assert rp.info["self_records"] > 0
    if name.startswith("clean"):
        assert 0 < int(rp.opposite.sum()) < len(rp)
    if name == "wide_entry":                              # 300 copies of one read: every pair on the same strand
        assert len(rp) == 44850 and not rp.opposite.any()
    if name == "long_run":
        assert rp.rows().tolist() == [[1, 19970, 0, (19969 << 32) | 19969]]


# ---- 6. a constructed geometry ------------------------------------------------------------------------------------------------------------------
def test_constructed_geometry(H, O):
    """Read A = g[1000:1300], read C = g[1100:1250] and read B = its reverse complement, among 50 reads of another genome: what the rows must be
    follows from the construction alone."""
    seqs, par = _seqs("geometry")
    dna = H.DnaBuffer.from_sequences(seqs)
    with _open(H, par) as c:
        with c.count_resident(dna, rid_base=0) as dev:
            with dev.strands(dna, rid_base=0) as st:
                rp = dev.pairs(strands=st)
    rows = {(int(o), int(a), int(b)): (int(s), int(f), int(l)) for o, a, b, s, f, l in zip(rp.opposite, rp.rid_a, rp.rid_b, rp.shared, rp.first, rp.last)}
    print({k: v for k, v in rows.items() if k[2] <= 2})
    assert rows[(0, 0, 1)] == (120, (100 << 32) | 0, (219 << 32) | 119) and (1, 0, 1) not in rows
    s, f, l = rows[(1, 0, 2)]
    assert s == 120 and (0, 0, 2) not in rows
    for v in (f, l):
        assert (v >> 32) + (v & 0xFFFFFFFF) == 100 + 150 - 31
    assert (f >> 32, l >> 32) == (100, 219)
    assert rows[(1, 1, 2)][0] == 120 and (0, 1, 2) not in rows


# ---- 7. folding -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["clean", "same_read"])
def test_folding_gives_the_unoriented_list(H, O, name):
    case = _case(H, O, name)
    par = case["par"]
    with _open(H, par) as c:
        with c.count_resident(case["dna"], rid_base=par["rid_base"]) as dev:
            with dev.strands(case["dna"], rid_base=par["rid_base"]) as st:
                rp = dev.pairs(strands=st)
                for ms in (1, 3):
                    plain, folded = dev.pairs(min_shared=ms), rp.fold(min_shared=ms)
                    assert not folded.oriented and len(plain) > 100 and np.array_equal(folded.rows(), plain.rows())
                    assert folded.info["records"] == plain.info["records"] and folded.info["self_records"] == plain.info["self_records"]
                assert len(rp) > len(plain)


# ---- 8. sliced equals unsliced ----------------------------------------------------------------------------------------------------------------------
def test_sliced_equals_unsliced(H, O):
    case = _case(H, O, "few")
    par = case["par"]
    ref = _ref(case)
    with _open(H, par) as c:
        with c.count_resident(case["dna"], rid_base=par["rid_base"]) as dev:
            with dev.strands(case["dna"], rid_base=par["rid_base"]) as st:
                one = dev.pairs(strands=st)
                _check_rows(one, ref)
                assert one.info["slices"] == 1 and one.info["records"] > 1000
                assert one.info["sort_passes"] == sort_passes_of(distinct_keys(ref))
                recs = entry_records(case["o"], case["strand"])
                for m in (one.info["records"] // 7, 1):
                    rp = dev.pairs(strands=st, max_records=m)
                    _check_rows(rp, ref)
                    assert (rp.info["slices"], rp.info["sort_passes"]) == slice_plan(recs, m)
                    assert rp.info["slices"] > 1 and np.array_equal(rp.rows(), one.rows())


# ---- 9. several lists -------------------------------------------------------------------------------------------------------------------------------
def test_several_lists_combine(H, O, clean):
    c, dev, st, case = clean
    whole = _ref(case)
    a, b = dev.pairs(0, 5, strands=st), dev.pairs(5, 16, strands=st)
    _check_rows(a, _ref(case, task_lo=0, task_hi=5))
    _check_rows(b, _ref(case, task_lo=5, task_hi=16))
    for comb in (H.ReadPairs.combine([a, b], ctx=c), H.ReadPairs.combine([a, b])):
        assert comb.oriented and np.array_equal(comb.rows(), whole[0])
        assert comb.info["records"] == whole[1] and comb.info["keys"] == whole[3]
    with pytest.raises(ValueError):
        H.ReadPairs.combine([a, dev.pairs(5, 16)])
    with pytest.raises(ValueError):
        H.ReadPairs.combine([a, dev.pairs(5, 16)], ctx=c)


# ---- 10. ownership ------------------------------------------------------------------------------------------------------------------------------------
def test_ownership(H, O):
    """Rows left in HBM; strands of another result are refused; Strands, ReadPairs, DeviceResult and Context closed in that order, with red zones
    behind every device block (the check of tests/test_gpu_pairs.py: a call fails if a kernel wrote past one)."""
    case, few = _case(H, O, "clean"), _case(H, O, "few")
    par = case["par"]
    c = _open(H, par, tuning={"pool_redzone": 256})
    dev = c.count_resident(case["dna"], rid_base=par["rid_base"])
    st = dev.strands(case["dna"], rid_base=par["rid_base"])
    _check_bits(dev, st, case)
    host = dev.pairs(strands=st)
    _check_rows(host, _ref(case))
    d = dev.pairs(strands=st, on_device=True)
    assert d.oriented and d.n == len(host) and d.rows_dev and d.info["records"] == host.info["records"]
    rows = c.d2h(d.rows_dev, d.n * 32).view(np.uint64).reshape(d.n, 4)
    assert np.array_equal(rows, host.rows())
    with c.count_resident(few["dna"], rid_base=par["rid_base"]) as dev2:
        with dev2.strands(few["dna"], rid_base=par["rid_base"]) as st2:
            with pytest.raises(H.HskError) as e:
                dev.pairs(strands=st2)
            assert e.value.status == 1 and "do not belong" in str(e.value)
            _check_rows(dev2.pairs(strands=st2), _ref(few))
    _check_rows(dev.pairs(strands=st), _ref(case))        # the context works afterwards
    before = c.stats(reset=False)
    st.close()
    d.close()
    dev.close()
    after = c.stats(reset=False)
    assert after["host_syncs"] == before["host_syncs"] and after["d2h_bytes"] == before["d2h_bytes"]      # closing launches and copies nothing
    with c.count_resident(case["dna"], rid_base=par["rid_base"]) as dev3:                                  # ... and the pool serves the next call (its red zones checked)
        with dev3.strands(case["dna"], rid_base=par["rid_base"]) as st3:
            _check_bits(dev3, st3, case)
    c.close()
    st.close(); d.close()                                 # closing twice, and after the context, is harmless
