"""The EXTENSION payloads -- every (PosInRead, ReadId) of every retained k-mer -- against the CPU oracle on inputs that are not 150-base reads
(tests/ragged_inputs.py; tests/test_ext_brute_force.py holds the oracle to the definition on the same inputs).  Only pos and rid depend on the
code this file is about; the k-mers and counts would survive all of it:
  1. the read-index window of scan_kernel (PARSE_RWIN entries per tile, the find_read branch behind it, tile_r0 and the search range of
     resolve_pos_rid_kernel, runs of empty reads that share one offset with the read behind them): crowded_index;
  2. positions far beyond 2^16 and supermers across tile edges (pos = g - 4 roff[r], sm_pos + i0 in the expand kernels): long_records;
  3. groups of more than U records and counts beyond 2^16 beside payloads: past_16_bits, low_complexity;
  4. several virtual ranks whose read counts, empty reads included, add up to rid_base: the loopback cases.
Every case compares EVERY entry: task offsets, k-mers, counts, histogram text, the payload ranges (disjoint, inside the arrays) and the sorted
(entry, rid, pos) triples as whole arrays."""
import collections

import numpy as np
import pytest

from tests import brute_force as B
from tests.ext_compare import assert_list_equals, entry_triples, oracle_want
from tests import ragged_inputs as R

pytestmark = pytest.mark.gpu

FAMILIES = {
    "crowded_index": lambda K: R.crowded_index(K, R.SEED),
    "ragged": lambda K: R.ragged(K, R.SEED),
    "long_records": lambda K: R.long_records(K, R.SEED, 0),
    "long_records_tail": lambda K: R.long_records(K, R.SEED, 1),
    "low_complexity": lambda K: R.low_complexity(K, R.SEED),
    "past_16_bits": lambda K: R.past_16_bits(K, R.SEED, apart=K >= 13),      # (K = 5: the background holds every 5-mer there is)
}
RID_BASE = 1000
_INPUT = {}
_ORACLE = collections.OrderedDict()
_ORACLE_KEPT = 24                                # lists kept at a time (the cases come grouped by input; a list with payloads takes up to ~100 MB)


def _input(family, K):
    """(reads, (packed, read_off, read_len)) of a family at K: built once"""
    if (family, K) not in _INPUT:
        seqs = FAMILIES[family](K)
        _INPUT[family, K] = (seqs, R.pack(seqs))
    return _INPUT[family, K]


def _oracle(family, K, M, L, U, ntasks, rid_base=RID_BASE):
    """the oracle's list of an input with its sorted triples: computed once, shared by every case on it, never written to"""
    from oracle import hsk_oracle as O
    key = (family, K, M, L, U, ntasks, rid_base)
    if key not in _ORACLE:
        packed, off, lens = _input(family, K)[1]
        _ORACLE[key] = oracle_want(O.count(packed, off, lens, k=K, m=M, L=L, U=U, ext=1, ntasks=ntasks, rid_base=rid_base, fast=True))
        while len(_ORACLE) > _ORACLE_KEPT:
            _ORACLE.popitem(last=False)
    return _ORACLE[key]


def _check(family, K, M, L, U, ntasks, tuning=None, plan=None, rid_base=RID_BASE):
    import hysortk_amd as H
    dna = _input(family, K)[1]
    with H.Context(K=K, M=M, L=L, U=U, EXT=1, ntasks=ntasks, profile=True, plan=plan, tuning=tuning) as c:
        res = c.count(dna, rid_base=rid_base)
        st = c.stats()
    want = _oracle(family, K, M, L, U, ntasks, rid_base)
    assert res.info["total_kmers"] == want.total_kmers
    assert_list_equals(res, want, (family, K, M, L, U, ntasks, tuning, plan))
    return res, st


def _filters(family):
    return ((1, 65535), (15, 40)) if family == "past_16_bits" else ((1, 65535), (2, 40))


def _grid():
    for K, M, tasks in [(31, 17, (1, 5, 16)), (5, 3, (8,)), (21, 11, (8,)), (31, 25, (8,)), (27, 5, (8,)), (35, 17, (8,)), (51, 17, (8,)), (77, 17, (8,))]:
        for family in FAMILIES:
            for ntasks in tasks:
                for L, U in _filters(family):
                    yield family, K, M, ntasks, L, U


@pytest.mark.parametrize("family,K,M,ntasks,L,U", list(_grid()))
def test_extension_payloads_on_uneven_inputs_vs_oracle(family, K, M, ntasks, L, U):
    res, st = _check(family, K, M, L, U, ntasks)
    assert st["scan_launches"] > 0 and st["parse_fallbacks"] == 0, st      # (the scan with its read-index window produced the supermers)
    if family == "past_16_bits" and U == 65535 and K >= 13:                # (tests/test_ext_brute_force.py: 65535 instances stay with all their payloads)
        assert int(res.cnt.max()) == 65535
    if family.startswith("long_records") and U == 65535:
        assert int(res.pos.max()) == 2048 * 150 - K > 1 << 18


# (switch, plan, what hsk_stats must say of the run)
FORCED = [
    ("parse_fast=0", None, lambda st: st["scan_launches"] == 0),                     # the general parse kernels
    ("scan_generic=1", None, lambda st: st["scan_launches"] > 0),                    # scan_kernel<0, 0> at the default (K, M)
    ("fused_scatter_ext=0", None, None),                                             # expand + two passes with payload
    ("fused_scatter=0", None, None),
    ("xcd_batch=0", None, lambda st: st["fused_tasks"] == 0),                        # the single-task path
    (None, "no_aggregation", lambda st: st["fused_tasks"] == 0 and st["agg_launches"] == 0),
    (None, "full_sort", lambda st: st["fused_tasks"] == 0 and st["agg_launches"] == 0),
    ("agg_large=0", None, lambda st: st["agg_large_bins"] == 0 and st["agg_large_slices"] == 0),
    ("pool_redzone=4096", None, None),                                               # nothing is written past a block
]
FORCED_FAMILIES = ["crowded_index", "long_records", "ragged"]


@pytest.mark.parametrize("tuning,plan,ran", FORCED, ids=[(t or p) for t, p, _ in FORCED])
@pytest.mark.parametrize("K,M,ntasks", [(31, 17, 16), (51, 17, 8)])
@pytest.mark.parametrize("family", FORCED_FAMILIES)
def test_extension_payloads_forced_paths_vs_oracle(family, K, M, ntasks, tuning, plan, ran):
    res, st = _check(family, K, M, 1, 65535, ntasks, tuning=tuning, plan=plan)
    if ran is not None:
        assert ran(st), (tuning, plan, st)


@pytest.mark.parametrize("K,M", [(51, 35), (77, 65)])
@pytest.mark.parametrize("family", FORCED_FAMILIES)
def test_extension_payloads_wide_minimizers_vs_oracle(family, K, M):
    """M > SCAN_MAX_M: the general parse kernels by themselves"""
    res, st = _check(family, K, M, 1, 65535, 8)
    assert st["scan_launches"] == 0, st


_UNFILTERED = {}


@pytest.mark.parametrize("K,M", [(31, 17), (5, 3)])
@pytest.mark.parametrize("family", ["crowded_index", "long_records"])
def test_stage_task_kmers_payloads_vs_oracle_and_definition(family, K, M):
    """hsk_stage_task_kmers, task by task: each task's instances are the oracle's, and all tasks together are every position of every read"""
    import hysortk_amd as H
    from oracle import hsk_oracle as O
    ntasks = 8
    seqs, dna = _input(family, K)
    ores = O.count(*dna, k=K, m=M, L=1, U=65535, ext=1, ntasks=ntasks, rid_base=RID_BASE, fast=True)
    parts = []
    with H.Context(K=K, M=M, L=1, U=65535, EXT=1, ntasks=ntasks) as c:
        for t in range(ntasks):
            keys, pos, rid = c.stage_task_kmers(dna, t, rid_base=RID_BASE)
            a, b = int(ores.task_off[t]), int(ores.task_off[t + 1])
            pa, pb = int(ores.payoff[a]), int(ores.payoff[b])
            want = B.sort_triples(np.repeat(ores.keys[a:b], ores.cnt[a:b].astype(np.int64), axis=0), ores.rid[pa:pb], ores.pos[pa:pb])
            got = B.sort_triples(keys, rid, pos)
            assert all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want)), t
            parts.append(got)
    if (family, K) not in _UNFILTERED:
        _UNFILTERED[family, K] = B.triples(seqs, K, 1, None, rid_base=RID_BASE)
    allof = B.sort_triples(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]))
    assert all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(allof, _UNFILTERED[family, K]))


@pytest.mark.parametrize("family", ["crowded_index", "ragged"])
def test_read_ids_up_to_the_top_of_int32(family):
    """rid_base = 2^31 - nreads: the last read's id is 2^31 - 1, the largest ReadId there is"""
    seqs, (packed, off, lens) = _input(family, 31)
    base = (1 << 31) - len(seqs)
    res, st = _check(family, 31, 17, 1, 65535, 16, rid_base=base)
    assert int(res.rid.max()) == base + int(np.flatnonzero(lens >= 31)[-1]) and int(res.rid.min()) >= base


@pytest.mark.parametrize("nranks", [2, 3])
def test_virtual_ranks_with_uneven_reads_vs_oracle(nranks):
    """rank 0 ends with empty reads, rank 1 starts with one, rank 2 is five records: rid_base[r] counts every read of the ranks before r"""
    import hysortk_amd as H
    from oracle import hsk_oracle as O
    K, M, L, U, ntasks = 31, 17, 1, 65535, 8 * nranks
    parts = [_input(f, K)[0] for f in ("crowded_index", "ragged", "long_records")[:nranks]]
    assert parts[0][-1] == "" and parts[1][0] == ""
    with H.Context(K=K, M=M, L=L, U=U, EXT=1, ntasks=ntasks) as c:
        res, owner = c.count_loopback([_input(f, K)[1] for f in ("crowded_index", "ragged", "long_records")[:nranks]])
    assert set(owner.tolist()) == set(range(nranks))
    packed, off, lens = R.pack([s for p in parts for s in p])
    for r in range(nranks):
        want = oracle_want(O.count(packed, off, lens, k=K, m=M, L=L, U=U, ext=1, ntasks=ntasks, task_owner=owner, my_rank=r, fast=True))
        assert_list_equals(res[r], want, (nranks, r))
    seen = np.unique(np.concatenate([kl.rid for kl in res]))
    first = np.cumsum([0] + [len(p) for p in parts])
    assert all(((seen >= first[r]) & (seen < first[r + 1])).any() for r in range(nranks))


def test_resident_result_payloads_equal_the_host_result():
    """count_resident + fetch(t) on crowded_index: the CSR of every task, read back from HBM, is the host result's (itself held to the oracle)"""
    import hysortk_amd as H
    K, M, L, U, ntasks = 31, 17, 1, 65535, 16
    dna = _input("crowded_index", K)[1]
    host, _ = _check("crowded_index", K, M, L, U, ntasks)
    with H.Context(K=K, M=M, L=L, U=U, EXT=1, ntasks=ntasks, keep_device=True) as c:
        with c.count_resident(dna, rid_base=RID_BASE) as dev:
            assert dev.n == len(host) and np.array_equal(dev.task_off, host.task_off)
            for t in range(dev.ntasks):
                a, b = int(host.task_off[t]), int(host.task_off[t + 1])
                d = dev.fetch(t)
                assert d["n"] == b - a
                if not d["n"]:
                    continue
                assert np.array_equal(d["kmers"], host.kmers[a:b]) and np.array_equal(d["cnt"], host.cnt[a:b])
                assert np.array_equal(d["payload_off"], host.payload_off[a:b])                      # same numbering as the host arrays
                local = d["payload_off"].astype(np.int64) - d["payload_base"]
                assert (local >= 0).all() and (local + d["cnt"].astype(np.int64) <= d["npay"]).all()
                got = entry_triples(d["cnt"], local, d["rid"], d["pos"])
                want = entry_triples(host.cnt[a:b], host.payload_off[a:b], host.rid, host.pos)
                assert all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want)), t
