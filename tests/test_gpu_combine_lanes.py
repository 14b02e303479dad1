"""combine_kernel's deduplicating instance hands the k-mers of a round's distinct items to its lanes as one stream (hsk_combine.h 3a, hsk_lanes.h:
lane tid takes the k-mers [tid * n, (tid + 1) * n) of the list, n = ceil(T / 256), whatever items they belong to).  Every case follows
test_gpu_combine_dedup.py: the whole list under combine_min_bytes=0 against the CPU oracle (task_off, keys, counts, histogram text, total_kmers),
its digest against the digest under combine_dedup=0, and from the statistics that the combining extraction produced it.

The inputs aim at the places where the stream can go wrong without failing: streams shorter than the workgroup and streams that are no multiple
of it (lanes without a k-mer, a short last piece), items of one k-mer (a piece spans many items) and of the full length (a piece starts and ends
inside an item), piece boundaries inside items of large multiplicity, one canonical k-mer twice in one lane's group, a k-mer table that runs over
while lanes hold half-finished pieces, several rounds per unit, direct items in front of the list, and the benchmark's shape."""
import numpy as np
import pytest

from tests import ragged_inputs as R
from tests import _combine_worker as W

pytestmark = pytest.mark.gpu

K, M = 31, 17
_INPUT, _ORACLE = {}, {}


def _few_reads(n, lo, hi, tag):
    """n random reads of lo .. hi bases: a few items per task, so a round's stream is shorter than the 256 lanes or ends in a short piece"""
    rng = np.random.default_rng([R.SEED, tag])
    return R.pack([R.random_seq(rng, int(rng.integers(lo, hi + 1))) for _ in range(n)])


def _one_kmer_copies():
    """300 reads of exactly K bases, 30 copies each, shuffled: every item is one k-mer, a lane's piece spans as many items as it has k-mers"""
    rng = np.random.default_rng([R.SEED, 311])
    reads = [R.random_seq(rng, K) for _ in range(300)]
    return R.pack([reads[i] for i in rng.permutation(np.repeat(np.arange(300), 30))])


def _one_kmer_distinct():
    rng = np.random.default_rng([R.SEED, 312])
    return R.pack([R.random_seq(rng, K) for _ in range(3000)])


def _long_copies():
    """40 random reads of 150 bases, 50 copies each: supermers as long as they come (many cut at 16 k-mers), every one 50 times"""
    rng = np.random.default_rng([R.SEED, 313])
    reads = [R.random_seq(rng, 150) for _ in range(40)]
    return R.pack([reads[i] for i in rng.permutation(np.repeat(np.arange(40), 50))])


def _k_to_k3():
    """1500 reads of K .. K + 3 bases in turn, five copies each: items of one to four k-mers, pieces that span three and more items"""
    rng = np.random.default_rng([R.SEED, 314])
    reads = [R.random_seq(rng, K + i % 4) for i in range(1500)]
    return R.pack([reads[i] for i in rng.permutation(np.repeat(np.arange(1500), 5))])


def _random_reads():
    rng = np.random.default_rng([R.SEED, 150])
    return R.pack([R.random_seq(rng, 150) for _ in range(2000)])


def _all_ones():
    """3000 reads each of: 40 T's and 60 random bases, all T, all A, ordinary -- shuffled (the dedup test's shape: direct items and list items in one unit)"""
    rng = np.random.default_rng([R.SEED, 40])
    reads = ["T" * 40 + R.random_seq(rng, 60) for _ in range(3000)] + ["T" * 100] * 3000 + ["A" * 100] * 3000 + [R.random_seq(rng, 100) for _ in range(3000)]
    return R.pack([reads[i] for i in rng.permutation(len(reads))])


def _benchmark_shape():
    import hysortk_amd.synth as S
    return S.packed_reads(40000, 150, 40000 * 32 // 150, R.SEED)


INPUTS = {
    "dozen": lambda: _few_reads(12, K, K + 12, 301),                  # at most 12 x 13 k-mers in all: below 256 with one task too
    "few_dozen": lambda: _few_reads(36, K, K + 19, 302),              # ~360 k-mers: one task has more than 256, five have fewer each
    "one_kmer_copies": _one_kmer_copies,
    "one_kmer_distinct": _one_kmer_distinct,
    "long_copies": _long_copies,
    "k_to_k3": _k_to_k3,
    "past_16_bits": lambda: R.pack(R.past_16_bits(K, R.SEED)),
    "low_complexity": lambda: R.pack(R.low_complexity(K, R.SEED)),
    "random_reads": _random_reads,
    "ragged": lambda: R.pack(R.ragged(K, R.SEED)),
    "all_ones": _all_ones,
    "benchmark_shape": _benchmark_shape,
}


def _input(name):
    if name not in _INPUT:
        _INPUT[name] = INPUTS[name]()
    return _INPUT[name]


def _oracle(name, L, U, ntasks):
    """the oracle's list of an input: computed once, shared by every case on it, never written to"""
    from oracle import hsk_oracle as O
    key = (name, L, U, ntasks)
    if key not in _ORACLE:
        packed, off, lens = _input(name)
        _ORACLE[key] = O.count(packed, off, lens, k=K, m=M, L=L, U=U, ntasks=ntasks, fast=True)
    return _ORACLE[key]


def _check(name, L, U, ntasks, tuning=""):
    """the list under combine_dedup=1 against the oracle and against combine_dedup=0; returns the statistics of the deduplicating run"""
    import hysortk_amd as H
    from oracle import hsk_oracle as O
    dna = _input(name)
    want = _oracle(name, L, U, ntasks)
    seen = {}
    for dedup in (1, 0):
        with H.Context(K=K, M=M, L=L, U=U, ntasks=ntasks, profile=True, tuning="combine_min_bytes=0,combine_dedup=%d%s" % (dedup, "," + tuning if tuning else "")) as c:
            res = c.count(dna)
            st = c.stats()
        print("%s L=%d U=%d ntasks=%d %s dedup=%d: k-mers %d, items %d, distinct %d, pairs %d" % (name, L, U, ntasks, tuning, dedup, res.info["total_kmers"], st["combine_items"], st["combine_distinct_items"], st["combine_pairs"]))
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


@pytest.mark.parametrize("ntasks", [1, 5])
@pytest.mark.parametrize("name", ["dozen", "few_dozen"])
def test_stream_shorter_than_the_workgroup_and_no_multiple_of_it(name, ntasks):
    """a few dozen reads: a unit's stream has fewer than 256 k-mers (n = 1, lanes beyond T take nothing) or a few more (n = 2, the last piece is short)"""
    st = _check(name, 1, 65535, ntasks)
    packed, off, lens = _input(name)
    total = int(np.maximum(lens.astype(np.int64) - K + 1, 0).sum())
    assert st["combine_kmers"] == total
    if name == "dozen":
        assert total < 256
    else:
        assert 256 < total < 512 and total // 5 < 256


@pytest.mark.parametrize("name", ["one_kmer_copies", "one_kmer_distinct"])
def test_items_of_one_kmer(name):
    """reads of exactly K bases: a lane's piece of n k-mers spans n items, every k-mer starts a fresh window, twin and multiplicity"""
    st = _check(name, 1, 65535, 5)
    assert st["combine_items"] == st["combine_kmers"], st
    if name == "one_kmer_copies":
        assert st["combine_distinct_items"] * 10 <= st["combine_items"], st      # 30 copies, two strands


def test_items_of_the_full_length_at_high_multiplicity():
    """long random reads, 50 copies each: most pieces start and end inside an item, and every add carries a multiplicity"""
    st = _check("long_copies", 1, 65535, 5)
    assert st["combine_distinct_items"] * 20 <= st["combine_items"], st


def test_reads_of_k_to_k_plus_3_bases():
    st = _check("k_to_k3", 1, 65535, 5)
    assert st["combine_items"] * 4 >= st["combine_kmers"], st                    # items of four k-mers at most


@pytest.mark.parametrize("L,U", [(1, 65535), (15, 40)])
@pytest.mark.parametrize("name", ["past_16_bits", "low_complexity"])
def test_piece_boundaries_inside_items_of_large_multiplicity(name, L, U):
    """sums beyond 2^16 from multiplicities of thousands; one canonical k-mer several times inside one item, hence twice in one lane's group"""
    _check(name, L, U, 5)


@pytest.mark.parametrize("name", ["random_reads", "ragged"])
def test_the_kmer_table_runs_over_in_the_middle_of_a_group(name):
    """one bucket per task: units of thousands of distinct k-mers on a table of 2048 and of more distinct items than the item table holds -- several
    A/B rounds, and dumps while lanes hold half-finished pieces"""
    st = _check(name, 1, 65535, 5, "combine_bucket=1000000000")
    if name == "random_reads":
        assert st["combine_items"] >= 15000 and st["combine_distinct_items"] * 10 >= st["combine_items"] * 9, st


def test_direct_items_and_list_items_in_one_unit():
    """items that start with 32 T's never enter the item table: they are rolled one per lane in front of the list's stream (drop_certain=0 keeps the
    scan from removing the all-A k-mer's instances)"""
    _check("all_ones", 1, 65535, 5, "drop_certain=0")


@pytest.mark.parametrize("ntasks,L,U", [(1, 1, 65535), (5, 15, 40)])
def test_benchmark_shape_rolls_what_it_rolled(ntasks, L, U):
    """150-base reads at 32x of a 40 kbp genome: the stream must not change what counts as rolled (a third of the items at most, as the dedup test holds)"""
    st = _check("benchmark_shape", L, U, ntasks)
    assert st["combine_distinct_items"] * 3 <= st["combine_items"], st
