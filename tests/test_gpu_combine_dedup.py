"""combine_kernel's deduplicating instance (tuning combine_dedup=1, the default: equal supermer items of a work unit are counted in an LDS item
table and rolled once, with their multiplicity) against the CPU oracle and against combine_dedup=0 on the same input.  Every case asserts from
the statistics that the combining extraction produced the list, compares the whole list with the oracle's (task_off, keys, counts, histogram
text, total_kmers) and its digest with the digest of the same context under combine_dedup=0, and holds combine_items / combine_distinct_items to
what the input says: the share of distinct items where the input fixes it, equality with combine_dedup=0.

The inputs aim at the places where such a kernel goes wrong without failing: the bases behind an item's own supermer (they belong to the next
read: equal supermers differ there), an item table that is full, one item thousands of times, and an item whose first word is all ones (the
item table's "not published yet")."""
import numpy as np
import pytest

from tests import ragged_inputs as R
from tests import _combine_worker as W

pytestmark = pytest.mark.gpu

_INPUT, _ORACLE = {}, {}


def _benchmark_shape():
    import hysortk_amd.synth as S
    return S.packed_reads(40000, 150, 40000 * 32 // 150, R.SEED)


def _short_copies():
    """1500 random reads of 36 bases, each 20 times, in random order: behind every item's supermer lie the bases of whichever read came next"""
    rng = np.random.default_rng([R.SEED, 36])
    reads = [R.random_seq(rng, 36) for _ in range(1500)]
    return R.pack([reads[i] for i in rng.permutation(np.repeat(np.arange(1500), 20))])


def _random_reads():
    rng = np.random.default_rng([R.SEED, 150])
    return R.pack([R.random_seq(rng, 150) for _ in range(2000)])


def _all_ones():
    """3000 reads each of: 40 T's and 60 random bases, all T, all A, ordinary -- shuffled"""
    rng = np.random.default_rng([R.SEED, 40])
    reads = ["T" * 40 + R.random_seq(rng, 60) for _ in range(3000)] + ["T" * 100] * 3000 + ["A" * 100] * 3000 + [R.random_seq(rng, 100) for _ in range(3000)]
    return R.pack([reads[i] for i in rng.permutation(len(reads))])


INPUTS = {
    "benchmark_shape": _benchmark_shape,
    "short_copies": _short_copies,
    "random_reads": _random_reads,
    "all_ones": _all_ones,
    "ragged": lambda: R.pack(R.ragged(31, R.SEED)),
    "past_16_bits": lambda: R.pack(R.past_16_bits(31, R.SEED)),
    "low_complexity": lambda: R.pack(R.low_complexity(31, R.SEED)),
}


def _input(name):
    if name not in _INPUT:
        _INPUT[name] = INPUTS[name]()
    return _INPUT[name]


def _oracle(name, K, M, L, U, ntasks):
    """the oracle's list of an input: computed once, shared by every case on it, never written to"""
    from oracle import hsk_oracle as O
    key = (name, K, M, L, U, ntasks)
    if key not in _ORACLE:
        packed, off, lens = _input(name)
        _ORACLE[key] = O.count(packed, off, lens, k=K, m=M, L=L, U=U, ntasks=ntasks, fast=True)
    return _ORACLE[key]


def _check(name, L, U, ntasks, tuning="", K=31, M=17):
    """the list under combine_dedup=1 against the oracle and against combine_dedup=0; returns the statistics of the deduplicating run"""
    import hysortk_amd as H
    from oracle import hsk_oracle as O
    dna = _input(name)
    want = _oracle(name, K, M, L, U, ntasks)
    seen = {}
    for dedup in (1, 0):
        with H.Context(K=K, M=M, L=L, U=U, ntasks=ntasks, profile=True, tuning="combine_min_bytes=0,combine_dedup=%d%s" % (dedup, "," + tuning if tuning else "")) as c:
            res = c.count(dna)
            st = c.stats()
        print("%s K=%d L=%d U=%d ntasks=%d %s dedup=%d: items %d, distinct %d, pairs %d" % (name, K, L, U, ntasks, tuning, dedup, st["combine_items"], st["combine_distinct_items"], st["combine_pairs"]))
        # the combining extraction produced the list: its kernel ran over every k-mer, the instance path's extraction never did
        assert st["combine_launches"] > 0 and st["hist_launches"] == 0 and st["combine_kmers"] == res.info["total_kmers"], st
        assert res.info["total_kmers"] == want.stats["total_kmers"]
        assert np.array_equal(res.task_off, want.task_off)
        assert np.array_equal(res.kmers, want.keys)
        assert np.array_equal(res.cnt, want.cnt)
        assert H.histogram_text(res.histo) == O.histogram_text(want.cnt)
        assert 0 < st["combine_distinct_items"] <= st["combine_items"], st
        seen[dedup] = (W.digest(res), st)
    assert seen[1][0] == seen[0][0]
    assert seen[0][1]["combine_distinct_items"] == seen[0][1]["combine_items"], seen[0][1]
    assert seen[1][1]["combine_items"] == seen[0][1]["combine_items"], (seen[1][1], seen[0][1])      # both instances read the same items
    return seen[1][1]


@pytest.mark.parametrize("L,U", [(1, 65535), (15, 40)])
@pytest.mark.parametrize("ntasks", [1, 5])
def test_benchmark_shape_rolls_a_third_of_its_items_at_most(ntasks, L, U):
    """150-base reads at 32x of a 40 kbp genome, ~1.0e6 k-mers: a simulation of the cut rules gives 0.25 distinct items per item when every item is
    compared on its own bases and 0.41 when it is compared as stored (with what follows it in the read)"""
    st = _check("benchmark_shape", L, U, ntasks)
    assert st["combine_distinct_items"] * 3 <= st["combine_items"], st


def test_bases_behind_the_supermer_are_not_compared():
    """20 copies of 1500 reads of 36 bases: the simulation gives 0.074 distinct items per item on the items' own bases, 0.995 on the stored windows"""
    st = _check("short_copies", 1, 65535, 5)
    assert st["combine_distinct_items"] * 5 <= st["combine_items"], st


@pytest.mark.parametrize("name", ["ragged", "random_reads"])
def test_more_distinct_items_than_the_item_table_holds(name):
    """one bucket per task (combine_bucket beyond every task): units of up to 8192 items, nearly all of them distinct, on an item table of 1024"""
    st = _check(name, 1, 65535, 5, "combine_bucket=1000000000")
    if name == "random_reads":
        # 2000 x 120 k-mers in supermers of at most 16: more than 15000 items, 3000 per task, in units of a whole task; two equal items among random
        # reads would be a 31-mer met twice (expected: 1e-8).  Whatever the table could not hold was rolled all the same: nearly every item is
        assert st["combine_items"] >= 15000 and st["combine_distinct_items"] * 10 >= st["combine_items"] * 9, st


@pytest.mark.parametrize("name,L,U", [("past_16_bits", 1, 65535), ("past_16_bits", 15, 40), ("low_complexity", 1, 65535)])
def test_one_item_very_many_times(name, L, U):
    """multiplicities of thousands added to one slot, sums beyond 2^16; one canonical k-mer several times inside one item"""
    _check(name, L, U, 5)


def test_items_that_start_with_32_T():
    """word 0 of such an item is all ones, which the item table reads as "not published yet": they must be rolled without entering it.
    drop_certain=0 keeps the scan from removing the all-A k-mer's instances before the kernel sees them"""
    _check("all_ones", 1, 65535, 5, "drop_certain=0")
