"""The inputs of tests/test_gpu_heavy.py hold what they are built for (checked with the oracle and the host-only classifier, no GPU): without these
conditions the GPU cases could pass without a declined task, without a k-mer that only the SUM of the ranks' counts keeps or drops, without a run of
equal keys across two tiles of the merge kernel, or without a count of 2^16 and more inside one rank's list."""
import numpy as np
import pytest

from oracle import hsk_oracle as O
from tests import heavy_inputs as HI
from tests import test_gpu_large_bins as LB

AG_LOG2CAP_SMALL = 10            # hsk_agg.h: the first table of the ladder, 1024 slots (hsk_ctx::agg_first_cap starts there; hsk_host_finish.h: agg_stage1)
AGL_TAB = LB.AGL_TAB             # 2048: more distinct k-mers than that in one bin are beyond the medium table as well
FILTERS = [(1, 65535), (12, 65535), (23, 23), (24, 65535), (1, 22), (2, 23)]      # the (L, U) of test_gpu_heavy.py's first group
CROWDED = [(31, 2), (31, 3), (31, 8), (51, 2), (77, 2)]
RATIO_MANY = 0.8                 # unbalanced_ratio at which crowded() has more than one heavy task (1.2 leaves one: every other task is below the mean)
RATIO_MANY_TANDEM = 0.7          # the same for test_gpu_rccl.py's _heavy_reads() at 24 tasks


def _fullest_bin(part, K, task):
    r = HI.unfiltered(part, K)
    a, b = int(r.task_off[task]), int(r.task_off[task + 1])
    return int(np.bincount(LB.bin_of(r.keys[a:b], K).astype(np.int64)).max())


@pytest.mark.parametrize("K,R", CROWDED)
def test_crowded_is_heavy_crowded_on_every_rank_and_filtered_on_the_sum(K, R):
    parts = HI.crowded(K, R)
    whole = HI.join(parts)
    assert sum(int(p[2].size) for p in parts) == int(whole[2].size) <= 72000 and int(whole[2].max()) <= 150
    E = HI.heavy_set(whole, K)
    assert len(E) == 1, E
    t = E[0]
    full = HI.unfiltered(whole, K)
    # one crowded bin, and it is crowded on every rank: more distinct k-mers than the medium table holds
    tb = HI.task_of(full).astype(np.int64) * 65536 + LB.bin_of(full.keys, K).astype(np.int64)
    distinct = np.bincount(tb, minlength=HI.NTASKS * 65536)
    assert int((distinct > 64).sum()) == 1 and int(np.argmax(distinct)) // 65536 == t and int(distinct.max()) >= HI.crowded_distinct(K)
    per_rank = [_fullest_bin(p, K, t) for p in parts]
    print("K=%d R=%d: task %d, distinct k-mers of the crowded bin per rank %s" % (K, R, t, per_rank))
    assert min(per_rank) > AGL_TAB, per_rank                       # (R = 8: 2848 and more of the 3000; keys of two and three words: all 2150)
    # the filter on the sum
    first, length, total, largest, _ = HI.merged_runs(parts, K, t)
    assert int(length.max()) <= R and np.array_equal(np.sort(total), np.sort(full.cnt[HI.task_of(full) == t].astype(np.int64)))
    for L, U in FILTERS:
        below = int(((largest < L) & (total >= L) & (total <= U)).sum())
        print("  L=%d U=%d: %d k-mers below L on every rank and kept by the sum; %d with a sum of U, %d of U + 1" % (L, U, below, int((total == U).sum()), int((total == U + 1).sum())))
        if (L, R) == (12, 2):
            assert below >= 100
        if L == 2:
            assert below >= 10
        if U in (22, 23):
            assert int((total == U).sum()) >= 50 and int((total == U + 1).sum()) >= 50
        if L in (23, 24):
            assert int((total == L).sum()) >= 50 and int((total == L - 1).sum()) >= 50
    # a run of equal keys that starts in one tile of the merge kernel and ends in the next
    n = HI.straddling_runs(first, length)
    print("  %d runs across a tile edge of %d records" % (n, HI.HV_TILE))
    assert n >= 1


def test_crowded_under_32_bits_is_one_bin_of_the_tile_finish_that_no_tile_sees_whole():
    K = 31
    parts = HI.crowded_under_32_bits(2)
    whole = HI.join(parts)
    assert int(whole[2].size) <= 71000 and int(whole[2].max()) <= 150
    E = HI.heavy_set(whole, K)
    assert len(E) == 1
    for p in parts:
        r = HI.unfiltered(p, K)
        a, b = int(r.task_off[E[0]]), int(r.task_off[E[0] + 1])
        top = (r.keys[a:b, 0] >> np.uint64(32)) == 0                           # the bin of the 16 leading A
        assert int(top.sum()) >= 2900 and int(r.cnt[a:b][top].sum()) > 10 * HI.FN_NL and int(r.cnt[a:b][top].max()) < 64
    # crowded() itself is no such input: no bin of 32 prefix bits of its heavy task holds more than a few keys
    parts = HI.crowded(K, 2)
    t = HI.heavy_set(HI.join(parts), K)[0]
    for p in parts:
        r = HI.unfiltered(p, K)
        a, b = int(r.task_off[t]), int(r.task_off[t + 1])
        bins, n = np.unique(r.keys[a:b, 0] >> np.uint64(32), return_counts=True)
        rec = np.bincount(np.repeat(np.arange(bins.size), n), weights=r.cnt[a:b][np.argsort(r.keys[a:b, 0], kind="stable")].astype(np.float64))
        assert int(n.max()) <= 8 and int(rec[n > 1].max() if (n > 1).any() else 0) <= 512       # (512: FN_HALO -- every bin of several keys ends inside its owner's halo)


def test_crowded_has_several_heavy_tasks_at_a_lower_ratio():
    for K in (31, 51, 77):
        whole = HI.join(HI.crowded(K, 2))
        assert len(HI.heavy_set(whole, K, ratio=1.2)) == 1                      # every other task is below the mean: no ratio above 1 adds one
        E = HI.heavy_set(whole, K, ratio=RATIO_MANY)
        assert len(E) > 1 and HI.heavy_set(whole, K)[0] in E, E


def test_the_tandem_repeat_reads_have_several_heavy_tasks_at_a_lower_ratio():
    """test_gpu_rccl.py's _heavy_reads() at its 24 tasks: the switch case's second input"""
    from tests import test_gpu_rccl as TR
    from tests import ragged_inputs as RI
    dna = RI.pack(TR._heavy_reads())
    E23, E12, E07 = (HI.heavy_set(dna, 31, ntasks=24, ratio=r) for r in (2.3, 1.2, RATIO_MANY_TANDEM))
    print("heavy at 2.3: %s, at 1.2: %s, at %.1f: %s" % (E23, E12, RATIO_MANY_TANDEM, E07))
    assert len(E23) == 1 and E12 == E23                                        # the repeat's task is eight times the mean, every other task below it
    assert 1 < len(E07) < 24 and set(E23) <= set(E07)


@pytest.mark.parametrize("K", [31])
def test_crowded_one_sided_is_beyond_the_tables_on_rank_1_only(K):
    parts, counts = HI.crowded_one_sided(K)
    whole = HI.join(parts)
    assert counts == [int(p[2].size) for p in parts] and sum(counts) == int(whole[2].size)
    E = HI.heavy_set(whole, K)
    assert len(E) == 1
    t = E[0]
    r0 = HI.unfiltered(parts[0], K)
    a, b = int(r0.task_off[t]), int(r0.task_off[t + 1])
    bins0 = np.bincount(LB.bin_of(r0.keys[a:b], K).astype(np.int64))
    assert int(bins0.max()) == HI.ONE_SIDED_DISTINCT <= (1 << AG_LOG2CAP_SMALL) // 2       # every bin of the task fits half of the first table on rank 0
    assert _fullest_bin(parts[1], K, t) > AGL_TAB
    assert int(r0.cnt[a:b].sum()) > 0


ONE_RANK = [(K, which, copies) for K in (31, 51, 77) for which, copies in (("A", 65535), ("A", 65536), ("A", 65537), ("AC", None))]
ROUND_ROBIN = [(K, copies, R) for K in (31, 51, 77) for copies in (65535, 65536) for R in (2, 3)]


def ac_copies(K):
    return (70000 // (151 - K) + 1) * (151 - K)


def _check_past_16(K, which, copies, parts, want_per_rank):
    whole = HI.join(parts)
    assert int(whole[2].size) <= 71000 and int(whole[2].sum()) <= 3000000          # (homopolymer_edge: runs of up to 2048 copies in one read)
    full = HI.unfiltered(whole, K)
    E = HI.heavy_set(whole, K)
    filt = O.count(*whole, k=K, m=HI.M, L=1, U=65535, ntasks=HI.NTASKS, fast=True)
    lists = [HI.unfiltered(p, K) for p in parts]
    for key in HI.repeat_kmers(K, which):
        per = [HI.count_of(r, key) for r in lists]
        want_per_rank(per)
        assert sum(per) == HI.count_of(full, key) == copies
        at = int(np.flatnonzero(np.all(full.keys == key[None, :], axis=1))[0])
        assert int(HI.task_of(full)[at]) in E                              # its task is heavy
        assert HI.count_of(filt, key) == (65535 if copies == 65535 else 0)
    return E


@pytest.mark.parametrize("K,which,copies", ONE_RANK)
def test_past_16_bits_one_rank_holds_every_copy(K, which, copies):
    copies = copies or ac_copies(K)
    parts = HI.past_16_bits_on_one_rank(K, copies, which)

    def one_sided(per):
        assert per[0] == copies and not any(per[1:]), per
    E = _check_past_16(K, which, copies, parts, one_sided)
    assert len(E) == 1


@pytest.mark.parametrize("K,copies,R", ROUND_ROBIN)
def test_past_16_bits_round_robin_stays_below_on_every_rank(K, copies, R):
    parts = HI.past_16_bits_on_one_rank(K, copies, "A", R=R, round_robin=True)
    assert len(parts) == R

    def below(per):
        assert 4096 < min(per) and max(per) < 65536, per                    # (4096: FN_MAX_WALK, hsk_finish.h -- every rank's run is longer than the tile finish walks)
    E = _check_past_16(K, "A", copies, parts, below)
    assert len(E) == 1
