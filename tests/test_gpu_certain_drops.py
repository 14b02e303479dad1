"""The certain drops against the CPU oracle, k-mer by k-mer (tests/ragged_inputs.py: homopolymer_runs, homopolymer_edge; what these inputs hold is
checked in tests/test_ragged_inputs.py).  The sketch of a call counts the all-A and the all-C k-mer exactly inside its sample (est_homopolymer);
more than max(U, 2^16) copies set a bit of the call's mask (certain_drop_mask), and the scan and the general parse kernels clear the positions
of such k-mers from their valid masks (homopolymer_positions).  The oracle knows nothing of this and applies [L, U]: a k-mer that is dropped has
more than U copies and is in no list, so EVERY list here is the oracle's -- a position dropped wrongly (a run of K - 1 bases, a C run under an
A / T mask, a run counted twice by the sketch) loses a k-mer that belongs in it.  That positions are dropped at all shows only in
hsk_stats::dropped_kmers: every case asserts it equals the count of ragged_inputs.expected_drops() for exactly the expected mask, and asserts
from the statistics that the path it names ran.  tuning plan_min_input=1 lets the sketch run on inputs of ~1 Mbp; below 4 MB of packed reads
its sample is every read but the last, which holds no run in any of these inputs."""
import collections

import numpy as np
import pytest

from tests.ext_compare import assert_list_equals, entry_triples, oracle_want
from tests import ragged_inputs as R

pytestmark = pytest.mark.gpu

RID_BASE = 1000
FILTERS = ((1, 65535), (2, 40))
_INPUT = {}
_ORACLE = collections.OrderedDict()
_ORACLE_KEPT = 16                                # lists kept at a time (the cases come grouped by input; one with payloads takes up to ~50 MB)


def _input(name, K):
    """(reads, (packed, read_off, read_len)) of an input at K, built once.  name: (which, uniform) of homopolymer_runs or
    ("edge", copies, base, single_run) of homopolymer_edge"""
    if (name, K) not in _INPUT:
        if name[0] == "edge":
            seqs = R.homopolymer_edge(K, R.SEED, name[1], name[2], single_run=name[3])
        else:
            seqs = R.homopolymer_runs(K, R.SEED, name[0], uniform=name[1])
        _INPUT[name, K] = (seqs, R.pack(seqs))
    return _INPUT[name, K]


def _oracle(name, K, M, L, U, ntasks, ext):
    """the oracle's list of an input (with payloads: ext_compare.Want): computed once, shared by every case on it, never written to"""
    from oracle import hsk_oracle as O
    key = (name, K, M, L, U, ntasks, ext)
    if key not in _ORACLE:
        packed, off, lens = _input(name, K)[1]
        ores = O.count(packed, off, lens, k=K, m=M, L=L, U=U, ext=ext, ntasks=ntasks, rid_base=RID_BASE if ext else 0, fast=True)
        _ORACLE[key] = oracle_want(ores) if ext else ores
        while len(_ORACLE) > _ORACLE_KEPT:
            _ORACLE.popitem(last=False)
    return _ORACLE[key]


def _assert_equals_oracle(res, name, K, M, L, U, ntasks, ext, tag=None):
    import hysortk_amd as H
    from oracle import hsk_oracle as O
    want = _oracle(name, K, M, L, U, ntasks, ext)
    if ext:
        assert res.info["total_kmers"] == want.total_kmers, tag
        assert_list_equals(res, want, tag)
        return
    assert res.info["total_kmers"] == want.stats["total_kmers"], tag
    assert np.array_equal(res.task_off, want.task_off), tag
    assert np.array_equal(res.kmers, want.keys), tag
    assert np.array_equal(res.cnt, want.cnt), tag
    assert H.histogram_text(res.histo) == O.histogram_text(want.cnt), tag


def _tuning(extra):
    return "plan_min_input=1" + ("," + extra if extra else "")


def _scanned(st):
    return st["scan_launches"] > 0 and st["parse_fallbacks"] == 0


def _check(name, K, M, L, U, ntasks=8, ext=0, extra=None, drops=True, ran=_scanned, count=None):
    """one call on the input against the oracle; dropped_kmers is what expected_drops() says of the reads (drops=False: nothing may be dropped)"""
    import hysortk_amd as H
    seqs, dna = _input(name, K)
    tag = (name, K, M, L, U, ntasks, ext, extra)
    with H.Context(K=K, M=M, L=L, U=U, EXT=ext, ntasks=ntasks, profile=True, tuning=_tuning(extra)) as c:
        res = count(c, dna) if count else c.count(dna, rid_base=RID_BASE if ext else 0)
        st = c.stats()
    mask, dropped = R.expected_drops(seqs, K, U) if drops else (0, 0)
    print(tag, "mask", mask, "dropped_kmers", int(st["dropped_kmers"]), "expected", dropped,
          {k: int(st[k]) for k in ("scan_launches", "parse_fallbacks", "combine_launches", "hist_launches", "combine_kmers")})
    assert int(st["dropped_kmers"]) == dropped, (tag, mask, int(st["dropped_kmers"]), dropped)
    assert ran(st), (tag, st)
    _assert_equals_oracle(res, name, K, M, L, U, ntasks, ext, tag)
    return res, st, mask


# ---- a. masks and K ---------------------------------------------------------------------------------------------------------------------------
def _mask_grid():
    for K, M in R.HOMO_GRID:
        for which in R.HOMO_WHICH if K not in R.HOMO_REFUSED_K else ():
            for ntasks in ((8, 1, 16) if (K, M) == (31, 17) else (8,)):
                for L, U in FILTERS:
                    yield K, M, which, False, ntasks, L, U
    for K, M in R.HOMO_UNIFORM_GRID:
        for which in R.HOMO_WHICH:
            for L, U in FILTERS:
                yield K, M, which, True, 8, L, U


@pytest.mark.parametrize("K,M,which,uniform,ntasks,L,U", list(_mask_grid()))
def test_certain_drops_of_runs_inside_reads_vs_oracle(K, M, which, uniform, ntasks, L, U):
    """A / T runs, C / G runs, both, or A / T beyond the threshold beside C / G runs below it: the mask is exactly what the sample holds, the runs
    of its bases go -- whole reads, at a read's start and end, inside it, K bases and more -- and everything else stays, the k-mers of K - 1
    equal bases beside every hole and (AT_over, U = 65535) the all-C k-mer with its exact count included"""
    from oracle import hsk_oracle as O
    res, st, mask = _check((which, uniform), K, M, L, U, ntasks)
    assert mask == {"AT": 1, "CG": 2, "both": 3, "AT_over": 1}[which]
    if which == "AT_over" and U == 65535:
        want = _oracle((which, uniform), K, M, L, U, ntasks, 0)
        key = O.string_to_words("C" * K)
        got = res.cnt[(res.kmers == key).all(axis=1)]
        assert got.size == 1 and 1000 <= int(got[0]) <= 60000 and got.tolist() == want.cnt[(want.keys == key).all(axis=1)].tolist()


def test_a_k_of_32_is_refused_before_any_mask_could_matter():
    """K = 32 would be the last K of the one-word arm of homopolymer_positions (shift 64 - 2 K = 0) and of the sketch (kmask = ~0): hsk_init
    refuses every K that is a multiple of 32, as the reference leaves them undefined, so that arm ends at K = 31"""
    import hysortk_amd as H
    for K in R.HOMO_REFUSED_K:
        with pytest.raises(H.HskError, match="invalid argument"):
            H.Context(K=K, M=17, L=1, U=65535, ntasks=8, tuning=_tuning(None))


# ---- b. must not drop -------------------------------------------------------------------------------------------------------------------------
NO_DROPS = [
    (58, 17, None, lambda st: st["scan_launches"] > 0),                              # the mask serves K <= 57
    (31, 26, None, lambda st: st["scan_launches"] == 0),                             # M = SCAN_MAX_M + 1: the general parse kernels from the start
    (31, 17, "parse_fast=0", lambda st: st["scan_launches"] == 0),
    (31, 17, "drop_certain=0", _scanned),
    (51, 17, "drop_certain=0", _scanned),
]


@pytest.mark.parametrize("L,U", FILTERS)
@pytest.mark.parametrize("K,M,extra,ran", NO_DROPS, ids=["K58", "M26", "parse_fast=0", "drop_certain=0", "drop_certain=0-K51"])
def test_nothing_is_dropped_where_the_mask_does_not_reach(K, M, extra, ran, L, U):
    seqs = _input(("both", False), K)[0]
    assert R.expected_drops(seqs, K, U)[0] == 3                      # (the sample holds enough of both k-mers: only the setting keeps them)
    _check(("both", False), K, M, L, U, extra=extra, drops=False, ran=ran)


# ---- c. payloads ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,U", FILTERS)
@pytest.mark.parametrize("which", ["both", "AT_over"])
@pytest.mark.parametrize("K,M", [(31, 17), (51, 17), (33, 17), (5, 3)])
def test_certain_drops_with_payloads_vs_oracle(K, M, which, L, U):
    """EXTENSION: every (entry, rid, pos) -- a supermer that starts behind a hole in the middle of a read has a pos that is not the read's start,
    in the 100 kbp record beyond 2^16"""
    res, st, mask = _check((which, False), K, M, L, U, ext=1)
    assert mask == (3 if which == "both" else 1)
    if U == 65535:
        assert int(res.pos.max()) > 1 << 16


def test_certain_drops_in_a_resident_result():
    """count_resident + fetch(t): the CSR of every task, read back from HBM, is the host result's (itself held to the oracle)"""
    import hysortk_amd as H
    K, M, L, U, ntasks = 31, 17, 1, 65535, 8
    seqs, dna = _input(("both", False), K)
    host = _check(("both", False), K, M, L, U, ntasks, ext=1)[0]
    with H.Context(K=K, M=M, L=L, U=U, EXT=1, ntasks=ntasks, keep_device=True, profile=True, tuning=_tuning(None)) as c:
        with c.count_resident(dna, rid_base=RID_BASE) as dev:
            assert int(c.stats()["dropped_kmers"]) == R.expected_drops(seqs, K, U)[1]
            assert dev.n == len(host) and np.array_equal(dev.task_off, host.task_off)
            for t in range(dev.ntasks):
                a, b = int(host.task_off[t]), int(host.task_off[t + 1])
                d = dev.fetch(t)
                assert d["n"] == b - a
                if not d["n"]:
                    continue
                assert np.array_equal(d["kmers"], host.kmers[a:b]) and np.array_equal(d["cnt"], host.cnt[a:b])
                assert np.array_equal(d["payload_off"], host.payload_off[a:b])
                local = d["payload_off"].astype(np.int64) - d["payload_base"]
                assert (local >= 0).all() and (local + d["cnt"].astype(np.int64) <= d["npay"]).all()
                got = entry_triples(d["cnt"], local, d["rid"], d["pos"])
                want = entry_triples(host.cnt[a:b], host.payload_off[a:b], host.rid, host.pos)
                assert all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want)), t


# ---- d. forced paths --------------------------------------------------------------------------------------------------------------------------
# (switch, EXTENSION settings it runs with, what hsk_stats must say of the run).  parse_rec_cap: a capacity below the supermers of a tile -- ~230 per
# 2048 positions at K = 31, ~110 at K = 51 (tests/test_gpu_host_path.py) -- makes the scan's store run over: the general parse kernels honour the mask
# combine_ratio=1: with a sketch the call's own estimate decides whether the combining extraction pays (264 000 distinct k-mers in 1 M: it does not);
# a ratio of 1 takes it whatever the estimate says
FORCED = [
    ("parse_rec_cap=%(cap)d", (0, 1), lambda st: st["parse_fallbacks"] > 0),
    ("scan_generic=1", (0, 1), _scanned),
    ("combine_min_bytes=0,combine_ratio=1", (0,), lambda st: _scanned(st) and st["combine_launches"] > 0),
    ("combine=0", (0, 1), lambda st: _scanned(st) and st["combine_launches"] == 0),
    ("pool_redzone=4096", (0, 1), _scanned),
]
REC_CAP = {31: 200, 51: 80}


@pytest.mark.parametrize("K,M", [(31, 17), (51, 17)])
@pytest.mark.parametrize("extra,ext,ran", [(e, x, r) for e, xs, r in FORCED for x in xs], ids=["%s-ext%d" % (e.split("=")[0], x) for e, xs, _ in FORCED for x in xs])
def test_certain_drops_forced_paths_vs_oracle(K, M, extra, ext, ran):
    res, st, mask = _check(("both", False), K, M, 1, 65535, ext=ext, extra=extra % dict(cap=REC_CAP[K]), ran=ran)
    assert mask == 3
    if extra.startswith("combine_min_bytes"):                       # (a call that started again on the instance path reports that attempt: no launch at all)
        assert st["combine_kmers"] == res.info["total_kmers"] - st["dropped_kmers"], st      # the combining kernel saw every k-mer the scan kept, and no other


@pytest.mark.parametrize("ext", [0, 1])
@pytest.mark.parametrize("K,M", [(31, 17), (51, 17)])
def test_certain_drops_of_device_resident_reads_vs_oracle(K, M, ext, tmp_path):
    """hsk_count_device: the sketch and the scan read the caller's buffers where they lie in HBM (packed there from FASTA text, hsk_pack_fasta:
    the same bytes as the host packer's)"""
    import hysortk_amd as H
    seqs, dna = _input(("both", False), K)
    fa = str(tmp_path / "runs.fa")
    with open(fa, "wb") as f, open(fa + ".fai", "w") as fai:
        for i, s in enumerate(seqs):
            f.write(b">r%d\n" % i)
            fai.write("r%d\t%d\t%d\t%d\t%d\n" % (i, len(s), f.tell(), len(s), len(s) + 1))
            f.write(s.encode() + b"\n")

    def count(c, dna):
        dd = H.read_dna_buffer_device(c, fa)
        try:
            assert dd.nreads == len(seqs) and dd.packed().tobytes() == dna[0].tobytes()
            return dd.count(rid_base=RID_BASE if ext else 0)
        finally:
            dd.free()

    assert _check(("both", False), K, M, 1, 65535, ext=ext, count=count)[2] == 3


ZERO_COPY_MIN, SLAB_INGEST_MIN = 16 << 20, 32 << 20      # hsk_count: pinned reads are read in place from 16 MB of packed reads on, in slabs from 32 MB on


@pytest.mark.parametrize("ingest,least", [("zero_copy", ZERO_COPY_MIN), ("slabs", SLAB_INGEST_MIN)])
@pytest.mark.parametrize("K,M", [(31, 17), (51, 17)])
def test_certain_drops_of_pinned_reads_vs_oracle(K, M, ingest, least):
    """Pinned input read in place by the scan, and ingested in slabs.  No switch selects either below 16 / 32 MB of packed reads, and no statistic
    names them (tests/test_gpu_host_path.py holds its inputs to the limits by name, as here), so the input is r copies of the ~1 Mbp one, one
    behind the other: every k-mer has r times its copies, and the list at [r L, r U] is the oracle's list of one copy at [L, U] with r times
    the counts (tests/test_ragged_inputs.py::test_a_tiled_input_scales_the_oracles_list holds the oracle itself to that).  The sample is then the
    first 4 MB, a dozen copies: both k-mers are certain, every one of the r copies of every run goes.  Without payloads (r times ~1 M of them)."""
    import hysortk_amd as H
    from oracle import hsk_oracle as O
    L, U, ntasks = 2, 40, 8
    seqs, dna = _input(("both", False), K)
    r = (least + (1 << 20)) // dna[0].size + 1
    packed, off, lens = R.tiled(dna, r)
    assert least + (1 << 20) <= packed.size < (SLAB_INGEST_MIN if ingest == "zero_copy" else 2 * SLAB_INGEST_MIN) and r * U <= 65535
    every, sample = R.homopolymer_positions(seqs, K)
    assert min(sample["A"] + sample["T"], sample["C"] + sample["G"]) > 65536              # (one copy alone is beyond the threshold, for any U here)
    pinned = (H.pinned_empty(packed.size, np.uint8), H.pinned_empty(off.size, np.uint64), H.pinned_empty(lens.size, np.uint32))
    try:
        for dst, src in zip(pinned, (packed, off, lens)):
            dst[:] = src
        with H.Context(K=K, M=M, L=r * L, U=r * U, ntasks=ntasks, profile=True, tuning=_tuning(None)) as c:
            res = c.count(pinned)
            st = c.stats()
    finally:
        for a in pinned:
            H.pinned_free(a)
    assert int(st["dropped_kmers"]) == r * sum(every.values()) and _scanned(st), st
    want = _oracle(("both", False), K, M, L, U, ntasks, 0)
    assert res.info["total_kmers"] == r * want.stats["total_kmers"]
    assert np.array_equal(res.task_off, want.task_off) and np.array_equal(res.kmers, want.keys) and np.array_equal(res.cnt, want.cnt * np.uint64(r))
    assert H.histogram_text(res.histo) == O.histogram_text(want.cnt * np.uint64(r))


# ---- e. the threshold -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("copies,single", [(65535, False), (65536, False), (65537, False), (65537, True)], ids=["65535", "65536", "65537", "65537-one_run"])
@pytest.mark.parametrize("U", [65535, 40])
@pytest.mark.parametrize("base", ["A", "C"])
@pytest.mark.parametrize("K", [K for K in R.HOMO_EDGE_K if K not in R.HOMO_REFUSED_K])
def test_the_threshold_is_more_than_two_to_the_sixteen_copies(K, base, U, copies, single):
    """exactly 65535, 65536 and 65537 copies inside the sample, in runs of 1 ... 2048 copies between short reads (the sketch's lanes take 64
    positions each and merge a run into one insert) or in one run: 65535 stay in a U = 65535 list with that count, 65536 are in no list and are
    not dropped (the sketch is certain from 2^16 + 1 on), 65537 are dropped, all of them.  An estimate that counted a k-mer twice at a lane's or
    a read's edge would drop the 65535 and the 65536."""
    from oracle import hsk_oracle as O
    M = 25 if K == 57 else 17
    res, st, mask = _check(("edge", copies, base, single), K, M, 1, U)
    assert mask == ((1 if base == "A" else 2) if copies == 65537 else 0) and int(st["dropped_kmers"]) == (65537 if copies == 65537 else 0)
    got = res.cnt[(res.kmers == O.string_to_words(("A" if base == "A" else "C") * K)).all(axis=1)]
    assert got.tolist() == ([65535] if copies == 65535 and U == 65535 else [])


# ---- f. several ranks -------------------------------------------------------------------------------------------------------------------------
def _rank_reads(K, nranks, runs_on_rank0):
    """rank 0: the runs that reach the threshold, the others: ~1500 reads with runs of the same bases, far below it -- or rank 0: ~4500 short
    reads without any run, rank 1: the runs that reach the threshold"""
    if not runs_on_rank0:
        return [R.homopolymer_edge(K, R.SEED, 0, "A"), _input(("both", False), K)[0]]
    return [_input(("both", False), K)[0]] + [R.homopolymer_runs(K, R.SEED + r, "both", nreads=1500, long_record=False, reach=False) for r in range(1, nranks)]


def _check_ranks(K, ext, nranks, runs_on_rank0):
    import hysortk_amd as H
    from oracle import hsk_oracle as O
    M, L, U, ntasks = 17, 1, 65535, 8 * nranks
    parts = _rank_reads(K, nranks, runs_on_rank0)
    with H.Context(K=K, M=M, L=L, U=U, EXT=ext, ntasks=ntasks, profile=True, tuning=_tuning(None)) as c:
        res, owner = c.count_loopback([R.pack(p) for p in parts])
        st = c.stats()
    assert set(owner.tolist()) == set(range(nranks))
    everyone = [s for p in parts for s in p]
    # the virtual ranks share the verdict of the first one's sketch: its sample alone decides, every rank's runs go
    mask = R.expected_drops(parts[0], K, U)[0]
    assert mask == (3 if runs_on_rank0 else 0)
    every = R.homopolymer_positions(everyone, K)[0]
    assert min(R.homopolymer_positions(p, K)[0][b] for p in parts[1:] for b in "ACGT") > 100
    assert int(st["dropped_kmers"]) == (sum(every.values()) if mask else 0), (mask, st)
    assert _scanned(st), st
    packed, off, lens = R.pack(everyone)
    assert sum(int(kl.info["total_kmers"]) for kl in res) == int(np.maximum(lens.astype(np.int64) - K + 1, 0).sum())
    for r in range(nranks):
        ores = O.count(packed, off, lens, k=K, m=M, L=L, U=U, ext=ext, ntasks=ntasks, task_owner=owner, my_rank=r, fast=True)
        if ext:
            assert_list_equals(res[r], oracle_want(ores), (nranks, r))
        else:
            assert np.array_equal(res[r].task_off, ores.task_off) and np.array_equal(res[r].kmers, ores.keys) and np.array_equal(res[r].cnt, ores.cnt), (nranks, r)
            assert H.histogram_text(res[r].histo) == O.histogram_text(ores.cnt), (nranks, r)
        assert len(res[r]) > 1000


@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("ext", [0, 1])
@pytest.mark.parametrize("K", [31, 51])
def test_virtual_ranks_drop_what_the_first_ranks_sketch_is_certain_of(K, ext, nranks):
    _check_ranks(K, ext, nranks, True)


def test_virtual_ranks_drop_nothing_when_the_first_rank_holds_no_runs():
    """the other rank holds more than 2^16 + 1 copies of both k-mers: they are filtered by U, not dropped -- same lists"""
    _check_ranks(31, 0, 2, False)


# ---- g. nothing outlives the call -------------------------------------------------------------------------------------------------------------
def test_the_certain_drops_of_both_kmers_do_not_outlive_the_call():
    """A call that left both k-mers out, then the stage entry points on the same context (they parse without a sketch): every instance is there
    again, the all-C k-mer's included; a second count gives the first list"""
    import hysortk_amd as H
    from oracle import hsk_oracle as O
    K, M, L, U, ntasks = 31, 17, 2, 40, 5
    seqs, dna = _input(("both", False), K)
    every = R.homopolymer_positions(seqs, K)[0]
    total = int(np.maximum(dna[2].astype(np.int64) - K + 1, 0).sum())
    with H.Context(K=K, M=M, L=L, U=U, ntasks=ntasks, profile=True, tuning=_tuning(None)) as c:
        r = c.count(dna)
        assert int(c.stats()["dropped_kmers"]) == sum(every.values()) > 2 * 65536 and int(r.info["total_kmers"]) == total
        keys = np.concatenate([c.stage_task_kmers(dna, t)[0] for t in range(ntasks)])
        assert keys.shape[0] == total
        for b, n in (("A", every["A"] + every["T"]), ("C", every["C"] + every["G"])):
            assert int((keys == O.string_to_words(b * K)).all(axis=1).sum()) == n
        r2 = c.count(dna)
        assert int(c.stats()["dropped_kmers"]) == sum(every.values())
    for x in (r, r2):
        _assert_equals_oracle(x, ("both", False), K, M, L, U, ntasks, 0)
