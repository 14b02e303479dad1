"""pair_finish_kernel (hysortk_amd/csrc/hsk_pairfinish.h: the first rung of the weighted finish for one-word keys -- a bin's {k-mer, count} pairs
sorted by a counting sort, equal keys merged, [L, U] applied to the sums, persistent workgroups) against the CPU oracle, k-mer by k-mer, AND
against the table kernel it replaces on that rung (tuning agg_adapt=3): list, counts and histogram equal.  combine_min_bytes=0 and
combine_ratio=1 let inputs of test size take and keep the combining extraction (they stay below plan_min_input: no sketch decides otherwise);
combine_prefix sets the bins' width.  Every case asserts from the statistics that the plan produced the list."""
import numpy as np
import pytest

from tests import ragged_inputs as R

pytestmark = pytest.mark.gpu

K, M = 31, 17
PF_CAP = 2048                        # pairs of a bin pair_finish_kernel takes (hsk_pairrank.h)
PLAN = "combine_min_bytes=0,combine_ratio=1"
TABLES = "agg_adapt=3"               # the table kernel on the first rung too: the form pair_finish_kernel replaced
_ORACLE = {}


def _oracle(name, dna, L, U, ntasks, k=K, m=M):
    """the oracle's list of an input: computed once per (input, filter), shared, never written to"""
    from oracle import hsk_oracle as O
    key = (name, L, U, ntasks, k, m)
    if key not in _ORACLE:
        _ORACLE[key] = O.count(dna[0], dna[1], dna[2], k=k, m=m, L=L, U=U, ntasks=ntasks, fast=True)
    return _ORACLE[key]


def _count(dna, L, U, ntasks, tuning, k=K, m=M):
    import hysortk_amd as H
    with H.Context(K=k, M=m, L=L, U=U, ntasks=ntasks, profile=True, tuning=tuning) as c:
        res = c.count(dna)
        st = c.stats()
    assert st["combine_launches"] > 0 and st["hist_launches"] == 0 and st["combine_kmers"] == res.info["total_kmers"], st
    return res, st


def _check(name, dna, L, U, ntasks, tuning="", k=K, m=M):
    """the input through pair_finish_kernel and through the table kernel: both equal the oracle's list; returns (result, stats) of the former"""
    import hysortk_amd as H
    from oracle import hsk_oracle as O
    want = _oracle(name, dna, L, U, ntasks, k, m)
    out = None
    for pf in (1, 0):
        res, st = _count(dna, L, U, ntasks, ",".join(x for x in (PLAN, tuning, "" if pf else TABLES) if x), k, m)
        assert res.info["total_kmers"] == want.stats["total_kmers"], pf
        assert np.array_equal(res.task_off, want.task_off), pf
        assert np.array_equal(res.kmers, want.keys), pf
        assert np.array_equal(res.cnt, want.cnt), pf
        assert H.histogram_text(res.histo) == O.histogram_text(want.cnt), pf
        out = out or (res, st)
    return out


def _words(want):
    """the k-mers of an oracle list as one word each (K <= 32)"""
    return np.asarray(want.keys, dtype=np.uint64).reshape(len(want.cnt), -1)[:, -1]


def _bin_sizes(want, prefix):
    """distinct k-mers per (task, prefix bin) of an oracle list taken with L = 1: the pairs of the bin when no k-mer left in partial pairs"""
    sizes = []
    for t in range(len(want.task_off) - 1):
        keys = _words(want)[int(want.task_off[t]):int(want.task_off[t + 1])]
        sizes.append(np.bincount((keys >> np.uint64(64 - prefix)).astype(np.int64), minlength=1 << prefix))
    return np.concatenate(sizes)


def _synth(genome, nreads, seed, read_len=150):
    from hysortk_amd import synth
    return list(synth.reads(genome, read_len, nreads, seed))


_INPUT = {}


def _input(name):
    if name not in _INPUT:
        _INPUT[name] = R.pack(_BUILD[name]())
    return _INPUT[name]


def _one_kmer_reads(rng, head, n):
    """n reads of exactly K bases that begin with `head` and do not end in T: the k-mer is its own canonical form (its reverse complement begins
    with C, G or T, `head` with A), so its prefix bin is known"""
    out = set()
    while len(out) < n:
        s = head + R.random_seq(rng, K - len(head) - 1) + "ACG"[int(rng.integers(0, 3))]
        out.add(s)
    return sorted(out)


def _full_bins(extra):
    """one task, bins of nine key bits: bin 0 (k-mers AAAA + A|C ...) holds exactly PF_CAP distinct k-mers, bin 1 (AAAA + G|T ...) PF_CAP + extra;
    every k-mer is a read of its own and occurs once in the whole input, so a pair is a k-mer whatever the work units; some uniform reads fill
    other bins"""
    rng = np.random.default_rng([2025, extra])
    a = [s for x in "AC" for s in _one_kmer_reads(rng, "AAAA" + x, PF_CAP // 2)]
    b = _one_kmer_reads(rng, "AAAAG", PF_CAP // 2) + _one_kmer_reads(rng, "AAAAT", PF_CAP // 2 + extra)
    back = [R.random_seq(rng, 150) for _ in range(200)]
    back = [s for s in back if "AAAA" not in s and "TTTT" not in s]
    reads = a + b + back
    return [reads[i] for i in rng.permutation(len(reads))]


def _bound_sums():
    """k-mers with 1, 2, 3, 4 and 49 .. 52 copies (reads of K bases on either strand) shuffled into error-free 20-fold reads: with one minimizer
    bucket per task (combine_bucket beyond any input) combine_kernel's table is written out again and again, and the copies of a k-mer -- far apart
    in the input -- leave in partial pairs whose counts lie below L, or inside [L, U], while their sum does not"""
    rng = np.random.default_rng([2025, 7])
    out = _synth(30000, 4000, 5)
    for copies in (1, 2, 3, 4, 49, 50, 51, 52):
        for _ in range(12):
            s = R.random_seq(rng, K)
            out += [s if i % 2 else R.revcomp(s) for i in range(copies)]
    return [out[i] for i in rng.permutation(len(out))]


def _past_16_bits():
    """65535, 65536 and 65537 copies of three k-mers (reads of K bases, either strand) among 20-fold reads: their minimizer buckets are cut into
    work units whose partial pairs the finish adds up"""
    rng = np.random.default_rng([2025, 16])
    ks = [R.random_seq(rng, K) for _ in range(3)]
    pool = _synth(20000, 2500, 9) + ks + [R.revcomp(s) for s in ks]
    nb = len(pool) - 6
    idx = [np.arange(nb, dtype=np.int64)] + [nb + j + 3 * rng.integers(0, 2, size=n, dtype=np.int64) for j, n in enumerate((65535, 65536, 65537))]
    return [pool[i] for i in rng.permutation(np.concatenate(idx))]


def _shared_bucket_bits():
    """k-mers that differ only in their last six bases, 600 of them under one 25-base head (and 40 under another), two to four copies each: one
    counting-sort bucket of pair_finish_kernel takes the whole bin whatever the prefix width (at most 4 x 600 / 1.5 < PF_CAP pairs even if every
    copy left as a pair of its own: the bin stays on the first rung)"""
    rng = np.random.default_rng([2025, 3])
    out = []
    for head, n in (("ACCA" + R.random_seq(rng, 21), 600), ("AGGA" + R.random_seq(rng, 21), 40)):
        tails = rng.choice(3 * 4 ** 5, size=n, replace=False)                  # (the last base is never T: the k-mer is its own canonical form)
        for t in tails:
            tail = "".join("ACGT"[(int(t) >> (2 * j)) & 3] for j in range(6))
            out += [head + tail] * (1 + int(t) % 3)
    out = sorted(set(out)) + out
    return [out[i] for i in rng.permutation(len(out))] + _synth(20000, 1000, 11)


_BUILD = {
    "tiny": lambda: _synth(20000, 2000, 3),
    "deep": lambda: _synth(30000, 6400, 4),                      # the benchmark's shape: 32-fold error-free reads of 150 bases
    "uniform": lambda: [R.random_seq(np.random.default_rng([2025, i]), 150) for i in range(3000)],
    "full": lambda: _full_bins(0),
    "full_plus_one": lambda: _full_bins(1),
    "low_complexity": lambda: R.low_complexity(K, R.SEED),
    "bound_sums": _bound_sums,
    "past_16_bits": _past_16_bits,
    "shared_bucket_bits": _shared_bucket_bits,
}


@pytest.mark.parametrize("prefix", [16, 14, 9])
def test_empty_bins_and_bins_of_one_and_two_pairs(prefix):
    """20 000 distinct k-mers over 8 tasks x 2^16 bins: most bins are empty, the others hold one or two pairs (asserted on the oracle's list)"""
    dna = _input("tiny")
    if prefix == 16:
        sizes = _bin_sizes(_oracle("tiny", dna, 1, 65535, 8), 16)
        assert (sizes == 0).sum() > len(sizes) // 2 and (sizes == 1).any() and (sizes == 2).any()
    _check("tiny", dna, 1, 65535, 8, "combine_prefix=%d" % prefix)
    _check("tiny", dna, 2, 40, 8, "combine_prefix=%d" % prefix)


def test_a_bin_of_exactly_the_capacity_stays_and_one_more_takes_the_ladder():
    for name, most in (("full", PF_CAP), ("full_plus_one", PF_CAP + 1)):
        dna = _input(name)
        sizes = _bin_sizes(_oracle(name, dna, 1, 65535, 1), 9)
        assert sizes[0] == PF_CAP and sizes[1] == most and sizes[2:].max() < PF_CAP, (name, sizes[:4])
        res, st = _check(name, dna, 1, 65535, 1, "combine_prefix=9")
        assert st["combine_pairs"] == len(res) == res.info["total_kmers"], (name, st)      # every k-mer once: a bin's pairs are its distinct k-mers
        assert (st["agg_retried_tasks"] > 0) == (most > PF_CAP), (name, st)  # PF_CAP + 1 pairs: listed for the 4096-slot table


@pytest.mark.parametrize("name,L,U,ntasks,tuning,partial", [
    ("deep", 1, 65535, 1, "combine_bucket=1000000000,combine_prefix=12", True),      # one minimizer bucket of 30 000 distinct k-mers: the 2048-slot table of combine_kernel is written out again and again
    ("deep", 2, 40, 1, "combine_bucket=1000000000,combine_prefix=10", True),
    ("low_complexity", 1, 65535, 5, "combine_prefix=11", False),                      # tandem repeats: one canonical k-mer many times in an item, items cut into slices
    ("low_complexity", 2, 40, 5, "combine_prefix=16", False),
])
def test_equal_keys_inside_a_bin(name, L, U, ntasks, tuning, partial):
    dna = _input(name)
    res, st = _check(name, dna, L, U, ntasks, tuning)
    if partial:
        assert st["combine_pairs"] > len(_oracle(name, dna, 1, 65535, ntasks).cnt), st       # more pairs than distinct k-mers: equal keys met in the finish


@pytest.mark.parametrize("L,U", [(2, 50), (3, 51), (1, 49), (4, 51)])
def test_sums_on_the_bounds_from_partial_counts_on_the_other_side(L, U):
    """the filter sees the SUM: copies 1 + 1 = L, 1 + 1 + 1 = L, 25 + 25 = U, 26 + 25 = U + 1, ... in partial pairs of different work units"""
    dna = _input("bound_sums")
    res, st = _check("bound_sums", dna, L, U, 1, "combine_bucket=1000000000,combine_prefix=13")
    all_ = _oracle("bound_sums", dna, 1, 65535, 1)
    for c in (L - 1, L, U, U + 1):
        assert c == 0 or (all_.cnt == c).sum() >= 12, c
    assert st["combine_pairs"] > len(all_.cnt), st                          # k-mers did leave in partial pairs
    assert (res.cnt == L).sum() >= 12 and (res.cnt == U).sum() >= 12 and int(res.cnt.min()) >= L and int(res.cnt.max()) <= U


@pytest.mark.parametrize("L,U", [(1, 65535), (15, 40)])
def test_sums_of_65535_65536_and_65537(L, U):
    """U = 65535 is the largest the library takes: 65535 copies stay, 65536 and 65537 do not, and no sum that wrapped at 2^16 (0 and 1) comes back
    inside [L, U]; sums beyond U = 65535 with a larger bound are the CPU exerciser's (tests/pairfinish_test.cpp)"""
    dna = _input("past_16_bits")
    res, st = _check("past_16_bits", dna, L, U, 4, "combine_prefix=12")
    if U == 65535:
        assert int(res.cnt.max()) == 65535 and int((res.cnt == 65535).sum()) == 1
    assert st["combine_pairs"] > len(_oracle("past_16_bits", dna, 1, 65535, 4).cnt)


@pytest.mark.parametrize("prefix", [9, 14, 16])
def test_a_bin_whose_keys_share_the_bucket_bits(prefix):
    dna = _input("shared_bucket_bits")
    want = _oracle("shared_bucket_bits", dna, 1, 65535, 2)
    assert np.unique(_words(want) >> np.uint64(14), return_counts=True)[1].max() == 600       # 600 k-mers equal in their first 25 bases
    for L, U in ((1, 65535), (2, 3)):
        res, st = _check("shared_bucket_bits", dna, L, U, 2, "combine_prefix=%d" % prefix)
        assert st["agg_retried_tasks"] == 0, st                              # the crowded bin was not handed to the table ladder


@pytest.mark.parametrize("name,L,U,ntasks,tuning", [
    ("deep", 2, 50, 8, ""),                          # the benchmark's shape at small scale, the library's own bin width
    ("deep", 2, 50, 1, "combine_prefix=9"),          # ... in bins of ~60 pairs
    ("uniform", 1, 65535, 8, ""),                    # uniform reads: every k-mer once, as many pairs as k-mers
    ("uniform", 1, 65535, 1, "combine_prefix=9"),    # ... ~700 pairs per bin: three lane slots
])
def test_benchmark_shape_and_uniform_reads(name, L, U, ntasks, tuning):
    _check(name, _input(name), L, U, ntasks, tuning)
