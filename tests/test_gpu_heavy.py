"""Heavy-hitter tasks against the oracle (inputs: tests/heavy_inputs.py, validated without a GPU by tests/test_heavy_inputs.py).  With several ranks a
task whose global k-mer count exceeds unbalanced_ratio x the mean is counted on every rank without the frequency filter (heavy_preaggregate: L = 1,
U = INT32_MAX, no long way) and its owner sums the ranks' lists and applies [L, U] (heavy_merge_kernel).  A rank whose finish cannot handle the task
DECLINES it (TaskOut::failed): the task then travels as supermers on every rank (HeavySet::settle).

Every case runs the virtual ranks on the parts and holds each rank's task_off, k-mers, counts and histogram text to the oracle's for the rank's tasks,
and total_kmers over the ranks to the k-mers of the reads.  hsk_stats::heavy_tasks says which way the task went: E is the heavy set of the host-only
classifier on the oracle's per-task instance sums.  Every context has a red zone behind its device blocks (pool_redzone=64: a write past a block
fails the call).

  1. settled and summed     the crowded bin on 2, 3, 8 ranks; per-rank counts below L whose sum is kept, sums of exactly U and U + 1, runs across tiles
  2. declined at the ladder agg_maxrung=0: the crowded bin overflows the first table and there is no next one
  3. declined at the tile finish   no_aggregation, one-word keys: a bin (of 32 prefix bits) no tile sees whole, a single-key run longer than the walk
  4. 2^16                   a k-mer with 65535 / 65536 / 65537 / ~70080 copies inside ONE rank's list, or split below 2^16 on every rank
  5. the switches           plain_classifier, unbalanced_ratio, EXTENSION
  6. two real ranks         the same over the transport: one rank declines alone; a list entry of more than 16 bits travels; the summed filter"""
import json

import numpy as np
import pytest

from tests import ext_compare
from tests import heavy_inputs as HI
from tests import test_gpu_large_bins as LB
from tests import test_heavy_inputs as TI

pytestmark = pytest.mark.gpu

NTASKS, M = HI.NTASKS, HI.M
REDZONE = "pool_redzone=64"
_WANT = {}


def _tuning(*more):
    return ",".join([REDZONE] + [m for m in more if m])


def _want(key, whole, K, L, U, owner, r, ext=0, ntasks=NTASKS):
    """the oracle's list of rank r's tasks: computed once per (input, filter, owner table), never written to"""
    from oracle import hsk_oracle as O
    k = (key, K, L, U, ext, ntasks, owner.tobytes(), r)
    if k not in _WANT:
        _WANT[k] = O.count(*whole, k=K, m=M, L=L, U=U, ext=ext, ntasks=ntasks, task_owner=owner, my_rank=r)
    return _WANT[k]


def _count(parts, K, L, U, tuning, ntasks=NTASKS, calls=1, **kw):
    """`calls` loopback counts on one context: [(lists, owner table, stats)]"""
    import hysortk_amd as H
    out = []
    with H.Context(K=K, M=M, L=L, U=U, ntasks=ntasks, tuning=tuning, **kw) as c:
        for _ in range(calls):
            res, owner = c.count_loopback(list(parts))
            out.append((res, owner, c.stats()))
    return out


def _check(key, parts, K, L, U, res, owner, ext=0, ntasks=NTASKS):
    import hysortk_amd as H
    from oracle import hsk_oracle as O
    whole = HI.join(parts)
    assert len(res) == len(parts) and len(owner) == ntasks
    for r, kl in enumerate(res):
        w = _want(key, whole, K, L, U, owner, r, ext, ntasks)
        if ext:
            ext_compare.assert_list_equals(kl, ext_compare.oracle_want(w), (key, r))       # every payload of every entry
            continue
        assert np.array_equal(kl.task_off, w.task_off), (key, r)
        assert kl.kmers.shape == w.keys.shape and np.array_equal(kl.kmers, w.keys), (key, r)
        assert np.array_equal(kl.cnt, w.cnt), (key, r)
        assert H.histogram_text(kl.histo) == O.histogram_text(w.cnt), (key, r)
    lens = whole[2].astype(np.int64)
    assert sum(int(kl.info["total_kmers"]) for kl in res) == int(np.maximum(lens - K + 1, 0).sum())


def _run(key, parts, K, L, U, heavy, tuning="", **kw):
    (res, owner, st), = _count(parts, K, L, U, _tuning(tuning), **kw)
    print("%s K=%d L=%d U=%d %s %s: heavy_tasks %d (expected %d), entries %s" % (key, K, L, U, tuning, kw, st["heavy_tasks"], heavy, [len(kl) for kl in res]))
    _check(key, parts, K, L, U, res, owner, ntasks=kw.get("ntasks", NTASKS))
    assert st["heavy_tasks"] == heavy, st
    return res, owner, st


def _E(parts, K, ratio=2.3, ntasks=NTASKS):
    return HI.heavy_set(HI.join(parts), K, ntasks=ntasks, ratio=ratio)


# ---- 1. settled and summed --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,U", TI.FILTERS)
@pytest.mark.parametrize("K,R", TI.CROWDED)
def test_crowded_task_is_summed_then_filtered(K, R, L, U):
    parts = HI.crowded(K, R)
    E = _E(parts, K)
    assert len(E) == 1
    res, owner, _ = _run(("crowded", R), parts, K, L, U, heavy=len(E))
    if (L, U) == (1, 65535):
        kl = res[int(owner[E[0]])]
        assert int(kl.task_off[E[0] + 1]) - int(kl.task_off[E[0]]) >= HI.crowded_distinct(K)           # the crowded bin came through the merge


@pytest.mark.parametrize("K", [31, 51])
def test_crowded_task_with_owner_side_items(K):
    """the other tasks travel as supermers with their minimizer bits and the owners build the items; the heavy task still travels as lists"""
    parts = HI.crowded(K, 2)
    res, owner, st = _run(("crowded", 2), parts, K, 12, 65535, heavy=1, tuning="combine_min_bytes=0,plan_sample=0")
    assert st["combine_pairs"] > 0, st


# ---- 2. declined at the ladder ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [31, 51, 77])
def test_task_beyond_the_first_table_is_declined_and_travels_as_supermers(K):
    """agg_maxrung=0: the ladder has no rung after the first table, the crowded bin (more than 2048 distinct k-mers on either rank) overflows it, and under
    forbid_long_way the task is reported, not redone (hsk_host_finish.h, agg_stage2).  Twice on one context: the same lists."""
    parts = HI.crowded(K, 2)
    assert len(_E(parts, K)) == 1
    for call, (res, owner, st) in enumerate(_count(parts, K, 2, 65535, _tuning("agg_maxrung=0"), calls=2)):
        print("K=%d call %d: heavy_tasks %d (E has 1), agg_retried_tasks %d" % (K, call, st["heavy_tasks"], st["agg_retried_tasks"]))
        _check(("crowded", 2), parts, K, 2, 65535, res, owner)
        assert st["heavy_tasks"] == 0, st


# ---- 3. declined at the tile finish -------------------------------------------------------------------------------------------------------------
def _all_a_round_robin(K, R=2):
    dna = LB.build_input(K, "A")
    return [HI.take(dna, np.arange(r, dna[2].size, R)) for r in range(R)]


@pytest.mark.parametrize("which,K,heavy", [("under_32_bits", 31, 0), ("all_a", 31, 0), ("crowded", 31, 1), ("crowded", 51, 1), ("all_a", 51, 1)])
def test_no_aggregation_declines_what_the_tile_finish_cannot_do(which, K, heavy):
    """The no_aggregation plan.  One-word keys finish in tiles (finish_kernel) after passes over the top 32 key bits.  3000 k-mers that share those bits are a
    bin of ~35 000 records on either rank that no tile sees whole (FN_FLAG_MIXED_GIANT); the all-A k-mer (~35 000 copies on either rank) is a
    single-key run longer than FN_MAX_WALK (FN_FLAG_LONG_WALK): under forbid_long_way the task is declined (hsk_host_finish.h, finish_batch_device).
    crowded() is NOT declined: its 3000 k-mers share 16 bits, the bin of the aggregation, and fall into ~3000 bins of the tile finish, each inside
    its owner's halo (tests/test_heavy_inputs.py says so).  Keys of two words have no tile finish: the full-width passes and the two-pass
    counter take the task whatever it holds, and it stays heavy."""
    parts = {"crowded": lambda: HI.crowded(K, 2), "all_a": lambda: _all_a_round_robin(K), "under_32_bits": lambda: HI.crowded_under_32_bits(2)}[which]()
    assert len(_E(parts, K)) == 1
    _run((which, 2), parts, K, 2, 65535, heavy=heavy, plan="no_aggregation")


# ---- 4. 2^16 ------------------------------------------------------------------------------------------------------------------------------------
def _expected_heavy(K, plan, E):
    """None: the aggregation kernels count in 32 bits, any run is one table slot.  full_sort, and no_aggregation with keys of two and three words: the
    two-pass counter (count_kernel), which finishes every task.  no_aggregation with one-word keys: the tile finish walks at most FN_MAX_WALK = 4096
    records of a run; every rank that holds the repeat holds more of it than that, so the task is declined (case 3)."""
    return 0 if (plan == "no_aggregation" and K <= 32) else len(E)


def _check_repeat(res, K, which, copies):
    """said once more on its own: the repeat k-mer is in the lists with 65535 copies when the reads hold 65535, and not at all otherwise"""
    for key in HI.repeat_kmers(K, which):
        found = [int(kl.cnt[i]) for kl in res for i in np.flatnonzero(np.all(kl.kmers == key[None, :], axis=1))]
        assert found == ([65535] if copies == 65535 else []), (copies, found)


@pytest.mark.parametrize("plan", [None, "full_sort", "no_aggregation"])
@pytest.mark.parametrize("K,which,copies", TI.ONE_RANK)
def test_count_of_2_16_and_more_inside_one_ranks_list(K, which, copies, plan):
    copies = copies or TI.ac_copies(K)
    parts = HI.past_16_bits_on_one_rank(K, copies, which)
    E = _E(parts, K)
    assert len(E) == 1
    # (a homopolymer with more than 2^16 copies on a rank that sketches its input is a certain drop: its task would be smaller than the oracle's sum)
    res, _, _ = _run(("one_rank", which, copies), parts, K, 1, 65535, heavy=_expected_heavy(K, plan, E), tuning="drop_certain=0" if copies > 65536 else "", plan=plan)
    _check_repeat(res, K, which, copies)


@pytest.mark.parametrize("plan", [None, "full_sort", "no_aggregation"])
@pytest.mark.parametrize("K,copies,R", TI.ROUND_ROBIN)
def test_sum_at_2_16_of_counts_below_it_on_every_rank(K, copies, R, plan):
    parts = HI.past_16_bits_on_one_rank(K, copies, "A", R=R, round_robin=True)
    E = _E(parts, K)
    assert len(E) == 1
    res, _, _ = _run(("round_robin", R, copies), parts, K, 1, 65535, heavy=_expected_heavy(K, plan, E), plan=plan)
    _check_repeat(res, K, "A", copies)


# ---- 5. the switches ------------------------------------------------------------------------------------------------------------------------------
def _tandem_parts():
    from tests import ragged_inputs as RI
    from tests import test_gpu_rccl as TR
    seqs = TR._heavy_reads()
    return [RI.pack(seqs[:len(seqs) // 2]), RI.pack(seqs[len(seqs) // 2:])]


@pytest.mark.parametrize("which", ["crowded", "tandem"])
def test_plain_classifier_and_unbalanced_ratio(which):
    parts, ntasks, ratio = (HI.crowded(31, 2), NTASKS, TI.RATIO_MANY) if which == "crowded" else (_tandem_parts(), 24, TI.RATIO_MANY_TANDEM)
    E, Emany = _E(parts, 31, ntasks=ntasks), _E(parts, 31, ratio=ratio, ntasks=ntasks)
    assert len(E) == 1 and len(Emany) > 1
    _run((which, 2), parts, 31, 2, 65535, heavy=1, ntasks=ntasks)
    _run((which, 2), parts, 31, 2, 65535, heavy=0, ntasks=ntasks, plain_classifier=True)
    _run((which, 2), parts, 31, 2, 65535, heavy=len(Emany), ntasks=ntasks, unbalanced_ratio=ratio)
    _run((which, 2), parts, 31, 2, 65535, heavy=1, ntasks=ntasks, unbalanced_ratio=1.2)          # (both inputs: every other task is below the mean)


@pytest.mark.parametrize("which", ["crowded", "tandem"])
def test_extension_has_no_heavy_tasks(which):
    """the classifier is forced plain with EXTENSION (heavy_enabled): payload triples equal the oracle's"""
    parts, ntasks = (HI.crowded(31, 2), NTASKS) if which == "crowded" else (_tandem_parts(), 24)
    (res, owner, st), = _count(parts, 31, 2, 65535, _tuning(), ntasks=ntasks, EXT=1)
    _check((which, 2), parts, 31, 2, 65535, res, owner, ext=1, ntasks=ntasks)
    assert st["heavy_tasks"] == 0, st


# ---- 6. two real ranks ----------------------------------------------------------------------------------------------------------------------------
def _two_ranks(tmp_path, port, parts, counts, K, L, U, heavy, tuning="", plan=None, env=None):
    """both ranks' arrays equal the virtual ranks' for the same parts and tuning (which the cases above hold to the oracle)"""
    from tests import test_gpu_rccl as TR
    seqs = [s for p in parts for s in HI.strings(p)]
    reads_json = str(tmp_path / "reads.json")
    json.dump(seqs, open(reads_json, "w"))
    spec = dict(K=K, M=M, L=L, U=U, EXT=0, ntasks=NTASKS, reads=reads_json, out=str(tmp_path / "rank%d.npz"), tuning=_tuning(tuning), plan=plan, counts=counts)
    got = TR._run_ranks(2, spec, tmp_path, port, env)
    from tests import util
    (want, owner, st), = _count(parts, K, L, U, _tuning(tuning, util.tuning(env)), plan=plan)
    _check(("two_ranks", port), parts, K, L, U, want, owner)
    assert st["heavy_tasks"] == heavy, st
    for r in range(2):
        g, w = got[r], want[r]
        assert np.array_equal(g["task_off"], w.task_off) and np.array_equal(g["kmers"], w.kmers) and np.array_equal(g["cnt"], w.cnt) and np.array_equal(g["histo"], w.histo), r
        assert int(g["heavy"][0]) == heavy, (r, int(g["heavy"][0]))
    assert sum(int(g["total_kmers"][0]) for g in got) == sum(max(len(s) - K + 1, 0) for s in seqs)


def test_two_ranks_one_declines_alone(tmp_path):
    """crowded_one_sided with the ladder cut short: rank 0's share of the crowded bin fits the first table, rank 1's does not.  The flags are combined
    (all-reduce, MAX): rank 0 frees the list it did build and sends supermers like its peer."""
    parts, counts = HI.crowded_one_sided(31)
    assert len(_E(parts, 31)) == 1
    _two_ranks(tmp_path, 29701, parts, counts, 31, 2, 65535, heavy=0, env={"HSK_AGG_MAXRUNG": "0"})


def test_two_ranks_exchange_a_count_beyond_16_bits(tmp_path):
    K = 51
    parts = HI.past_16_bits_on_one_rank(K, TI.ac_copies(K), "AC")
    assert len(_E(parts, K)) == 1
    _two_ranks(tmp_path, 29702, parts, [int(p[2].size) for p in parts], K, 1, 65535, heavy=1, tuning="drop_certain=0", plan="full_sort")


def test_two_ranks_filter_on_the_sum(tmp_path):
    parts = HI.crowded(31, 2)
    _two_ranks(tmp_path, 29703, parts, [int(p[2].size) for p in parts], 31, 12, 65535, heavy=1)
