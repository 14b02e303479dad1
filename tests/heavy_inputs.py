"""Inputs for the heavy-hitter path (tests/test_gpu_heavy.py; validated on the CPU by tests/test_heavy_inputs.py): with several ranks a task whose
global k-mer count exceeds unbalanced_ratio x the mean is pre-aggregated on every rank (L = 1, no upper bound, no long way) and summed by its
owner.  Every builder returns the reads PER RANK, a list of (packed, read_off, read_len) parts, built from the inputs of
tests/test_gpu_large_bins.py (a prefix bin of 3000 distinct k-mers; all-A and (AC)n reads of ~70 000 copies) and tests/ragged_inputs.py (an exact
number of homopolymer k-mers around 2^16):

  crowded(K, R)                  the crowded bin on every rank, ~200 of its k-mers once more than the others, dealt by a seeded permutation: per-rank
                                 counts below L whose sum is not, sums of exactly U and U + 1, runs of equal keys across the merge kernel's tiles
  crowded_under_32_bits(R)       K = 31: 3000 k-mers that share the 32 key bits the tile finish orders by first
  crowded_one_sided(K)           two ranks; only rank 1's share of the crowded bin is beyond the tables of the aggregation
  past_16_bits_on_one_rank(...)  a k-mer with 2^16 copies and more inside ONE rank's list, or below 2^16 on every rank with the sum at the edge

Plain functions, seeded and deterministic; the builders keep what they built (computed once, never written to).  The helpers below say what an input holds from the oracle alone."""
import functools

import numpy as np

from tests import ragged_inputs as RI
from tests import test_gpu_large_bins as LB

M = LB.M
NTASKS = LB.NTASKS
SEED = 777
NO_LIMIT = (1 << 31) - 1
HV_TILE = 256                    # records per workgroup of heavy_merge_kernel (hsk_heavy.h: HV_THREADS)
BUMPED = 200                     # crowded(): k-mers of the crowded bin with one copy more than the others
SINGLES = 256                    # crowded(): reads of K random bases added once, and as many added twice
_LUT =np.frombuffer(b"ACGT", dtype=np.uint8)


# ---- reads in the packed form ------------------------------------------------------------------------------------------------------
def take(dna, idx):
    """the reads `idx` (in that order) of a packed input, every read on a byte boundary again"""
    packed, off, lens = dna
    idx = np.asarray(idx, dtype=np.int64)
    nb = (lens[idx].astype(np.int64) + 3) // 4
    noff = np.zeros(idx.size, dtype=np.int64)
    if idx.size:
        noff[1:] = np.cumsum(nb)[:-1]
    src = np.repeat(off[idx].astype(np.int64) - noff, nb) + np.arange(int(nb.sum()), dtype=np.int64)
    return np.ascontiguousarray(packed[src], dtype=np.uint8), noff.astype(np.uint64), np.ascontiguousarray(lens[idx], dtype=np.uint32)


def join(parts):
    """the parts one behind the other: the whole input, in the order the ranks hold it"""
    base, offs = 0, []
    for p in parts:
        offs.append(p[1] + np.uint64(base)); base += p[0].size
    return np.concatenate([p[0] for p in parts]), np.concatenate(offs).astype(np.uint64), np.concatenate([p[2] for p in parts])


def strings(dna):
    """the reads as strings (the two-rank worker takes a JSON list)"""
    packed, off, lens = dna
    codes = np.stack([(packed >> 6) & 3, (packed >> 4) & 3, (packed >> 2) & 3, packed & 3], axis=1).reshape(-1)
    text = _LUT[codes].tobytes().decode()
    return [text[4 * int(o):4 * int(o) + int(n)] for o, n in zip(off, lens)]


def read_rows(dna, length):
    """(indices of the reads of exactly `length` bases, their packed bytes as rows)"""
    packed, off, lens = dna
    idx = np.flatnonzero(lens == length)
    nb = (length + 3) // 4
    return idx, packed[off[idx].astype(np.int64)[:, None] + np.arange(nb, dtype=np.int64)[None, :]]


def deal(n, R, rng):
    """n reads to R ranks by a seeded permutation: R index arrays"""
    perm = rng.permutation(n)
    return [perm[r::R] for r in range(R)]


# ---- what an input holds, from the oracle ------------------------------------------------------------------------------------------------
def unfiltered(dna, K, ntasks=NTASKS):
    """every k-mer with its count, task by task"""
    from oracle import hsk_oracle as O
    return O.count(*dna, k=K, m=M, L=1, U=NO_LIMIT, ntasks=ntasks, fast=True)


def task_of(res, ntasks=NTASKS):
    return np.repeat(np.arange(ntasks), np.diff(res.task_off).astype(np.int64))


def task_sums(res, ntasks=NTASKS):
    """k-mer instances per task"""
    return np.bincount(task_of(res, ntasks), weights=res.cnt.astype(np.float64), minlength=ntasks).astype(np.uint64)


def heavy_set(dna, K, ntasks=NTASKS, ratio=2.3):
    """E: the tasks the classifier calls heavy on the oracle's per-task instance sums"""
    import hysortk_amd as H
    return [int(t) for t in np.flatnonzero(H.plan_classify(task_sums(unfiltered(dna, K, ntasks), ntasks), ratio) == 1)]


def key_order(keys):
    """the order the library gives keys: the most significant word has the highest index"""
    return np.lexsort([keys[:, w] for w in range(keys.shape[1])])


def merged_runs(parts, K, task, ntasks=NTASKS):
    """The owner's view of `task`: the parts' unfiltered lists one behind the other, ordered by key (stable).  Returns (first record of every run of
    equal keys, its length, the sum of its counts, its largest per-rank count, the keys of the run heads)."""
    ks, cs = [], []
    for p in parts:
        r = unfiltered(p, K, ntasks)
        a, b = int(r.task_off[task]), int(r.task_off[task + 1])
        ks.append(r.keys[a:b]); cs.append(r.cnt[a:b].astype(np.int64))
    keys, cnt = np.concatenate(ks), np.concatenate(cs)
    o = np.lexsort([keys[:, w] for w in range(keys.shape[1])])       # (stable)
    keys, cnt = keys[o], cnt[o]
    head = np.ones(len(keys), dtype=bool)
    head[1:] = np.any(keys[1:] != keys[:-1], axis=1)
    first = np.flatnonzero(head)
    length = np.diff(np.concatenate((first, [len(keys)])))
    return first, length, np.add.reduceat(cnt, first), np.maximum.reduceat(cnt, first), keys[first]


def straddling_runs(first, length):
    """runs that start in one tile of heavy_merge_kernel and end in the next"""
    return int(((first // HV_TILE) != ((first + length - 1) // HV_TILE)).sum())


# ---- a. the crowded bin on every rank ---------------------------------------------------------------------------------------------------
def crowded_distinct(K):
    """Distinct k-mers of the crowded bin.  One-word keys: the 3000 of build_input; their last table has 8192 slots.  Keys of two and three words end at
    AG_LOG2CAP_LARGE = 4096 slots, where a bin gives up as soon as one probe sequence grows long: 3000 keys (load 0.73) are at that edge -- mostly
    counted, now and then declined, with the right lists either way -- so heavy_tasks could not be asserted.  2150 (load 0.52) are more than the
    medium table's 2048 and well inside the large one."""
    return 3000 if K <= 32 else 2150


@functools.lru_cache(maxsize=None)
def _crowded_whole(K):
    """build_input(K, "many"), crowded_distinct(K) of its 3000 chosen k-mers, and ~BUMPED of those (reads of exactly K bases, 23 copies each) a 24th time"""
    dna = LB.build_input(K, "many")
    idx, rows = read_rows(dna, K)
    _, firsts, inv = np.unique(rows, axis=0, return_index=True, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    assert firsts.size == 3000 and idx.size == 3000 * 23
    n = crowded_distinct(K)
    if n < 3000:                                                     # keys of two and three words: the reads of the other k-mers are left out
        keep = np.ones(dna[2].size, dtype=bool)
        keep[idx[inv >= n]] = False
        dna = take(dna, np.flatnonzero(keep))
        idx, rows = read_rows(dna, K)
        _, firsts = np.unique(rows, axis=0, return_index=True)
        assert firsts.size == n and idx.size == n * 23
    extra = idx[np.sort(firsts)[::n // BUMPED][:BUMPED]]
    # every k-mer above is on both of two ranks: runs of two from an even record on, none across a tile of 256.  Reads of K random bases, once (a run of
    # one wherever they fall) and twice (1 + 1 where the copies part: below L = 2 on either rank)
    rng = np.random.default_rng([SEED, K, 2])
    once = [RI.random_seq(rng, K) for _ in range(SINGLES)]
    twice = [RI.random_seq(rng, K) for _ in range(SINGLES)]
    return join([take(dna, np.concatenate((np.arange(dna[2].size), extra))), RI.pack(once + twice + twice)])


@functools.lru_cache(maxsize=None)
def crowded(K, R):
    dna = _crowded_whole(K)
    rng = np.random.default_rng([SEED, K, R, 1])
    return [take(dna, ix) for ix in deal(dna[2].size, R, rng)]


# ---- a'. crowded under the tile finish's 32 prefix bits ------------------------------------------------------------------------------------------
FN_NL = 2048 + 512               # records an owner tile of finish_kernel sees (hsk_finish.h: FN_TILE + FN_HALO)


@functools.lru_cache(maxsize=None)
def crowded_under_32_bits(R=2):
    """K = 31.  The tile finish (one-word keys without the aggregation) orders by the top 32 key bits first: crowded()'s 3000 k-mers share 16 bits and
    fall into ~3000 of ITS bins.  Here 3000 k-mers of one task share their first 16 bases (A), 23 copies each: one bin of ~69 000 records and 3000
    keys, which no tile sees whole."""
    from oracle import hsk_oracle as O
    from tests import util
    K = 31
    rng = np.random.default_rng([SEED, K, 16])
    reads = LB.background(rng)
    cand = ["A" * 16 + RI.random_seq(rng, K - 16) for _ in range(32000)]
    r = O.count(*RI.pack(cand), k=K, m=M, L=1, U=NO_LIMIT, ntasks=NTASKS, fast=True)
    task, top = task_of(r), (r.keys[:, 0] >> np.uint64(32)) == 0
    t0 = int(np.argmax(np.bincount(task[top], minlength=NTASKS)))
    sel = np.flatnonzero(top & (task == t0))[:3000]
    assert sel.size == 3000
    for s in util.result_strings(r.keys[sel], K):
        reads += [s] * 23
    dna = RI.pack(reads)
    return [take(dna, ix) for ix in deal(dna[2].size, R, rng)]


# ---- b. the crowded bin beyond the tables on one rank only ----------------------------------------------------------------------------------
ONE_SIDED_DISTINCT = 300         # k-mers of the crowded bin that rank 0 sees


@functools.lru_cache(maxsize=None)
def crowded_one_sided(K):
    """(parts, reads per rank): rank 0 holds the background and 11 copies each of ONE_SIDED_DISTINCT of the bin's k-mers, rank 1 everything else"""
    dna = LB.build_input(K, "many")
    idx, rows = read_rows(dna, K)
    _, inv = np.unique(rows, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    few = idx[inv < ONE_SIDED_DISTINCT]
    seen = np.zeros(ONE_SIDED_DISTINCT, dtype=np.int64)
    mine = []
    for i, c in zip(few, inv[inv < ONE_SIDED_DISTINCT]):
        if seen[c] < 11:
            seen[c] += 1; mine.append(int(i))
    is0 = dna[2] != K
    is0[mine] = True
    parts = [take(dna, np.flatnonzero(is0)), take(dna, np.flatnonzero(~is0))]
    return parts, [int(p[2].size) for p in parts]


# ---- c. 2^16 copies and more ------------------------------------------------------------------------------------------------------------------
def repeat_kmers(K, which):
    """the canonical repeat k-mers of the input as key rows: all-A, or the two of (AC)n"""
    from oracle import hsk_oracle as O
    if which == "A":
        return [O.string_to_words("A" * K)]
    unit = "AC" * K
    return [O.string_to_words(min(s, RI.revcomp(s))) for s in (unit[:K], unit[1:K + 1])]


@functools.lru_cache(maxsize=None)
def _repeat_whole(K, copies, which):
    """(reads as strings, which of them hold the repeat)"""
    if which == "A":
        seqs = RI.homopolymer_edge(K, SEED, copies, "A")
        rep = np.array([("A" * K in s) or ("T" * K in s) for s in seqs])
    else:
        assert copies == (70000 // (151 - K) + 1) * (151 - K)
        seqs = strings(LB.build_input(K, "AC"))
        unit = "AC" * 76
        fam = {"A" * 150, unit[:150], unit[1:151]}
        rep = np.array([s in fam for s in seqs])
    return seqs, rep


@functools.lru_cache(maxsize=None)
def past_16_bits_on_one_rank(K, copies, which, R=2, round_robin=False):
    """One-sided: rank 0 holds every read with a repeat k-mer and its share of the others, the other ranks hold background only.  round_robin: read i goes
    to rank i % R (copies below 2^16 on every rank, their sum at the edge)."""
    seqs, rep = _repeat_whole(K, copies, which)
    if round_robin:
        return [RI.pack(seqs[r::R]) for r in range(R)]
    back = np.flatnonzero(~rep)
    parts = []
    for r in range(R):
        ix = np.sort(np.concatenate((np.flatnonzero(rep), back[0::R]))) if r == 0 else back[r::R]
        parts.append(RI.pack([seqs[i] for i in ix]))
    return parts


def count_of(res, key):
    """the count of one k-mer (a key row) in an oracle result, 0 when it is not there"""
    hit = np.flatnonzero(np.all(res.keys == np.asarray(key, dtype=np.uint64)[None, :], axis=1))
    assert hit.size <= 1
    return int(res.cnt[hit[0]]) if hit.size else 0
