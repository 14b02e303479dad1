"""The inputs of tests/test_gpu_combine_ragged.py hold what they are built for (checked with the oracle, no GPU): without these conditions the GPU
tests could pass without ever meeting the item cut, a supermer across a tile edge, a k-mer twice in one item or a count beyond 2^16."""
import numpy as np
import pytest

from oracle import hsk_oracle as O
from tests import ragged_inputs as R

NTASKS = 8


def _canonical_words(s):
    return O.string_to_words(min(s, R.revcomp(s)))


@pytest.mark.parametrize("K,M", R.GRID)
def test_ragged_meets_the_item_cut_and_every_packing_phase(K, M):
    seqs = R.ragged(K, R.SEED)
    packed, off, lens = R.pack(seqs)
    for a, b in zip((packed, off, lens), O.pack_reads(seqs)):
        assert np.array_equal(a, b)
    assert len(seqs[0]) == 0 and len(seqs[-1]) == 0 and {int(n) % 4 for n in lens if n} == {0, 1, 2, 3}
    assert any("N" in s for s in seqs) and any(s and s == s.lower() for s in seqs)
    kc = R.item_cut(K)
    longer = shorter = exact = 0
    for r in range(len(seqs)):
        if lens[r] < K:
            continue
        d = O.dests(packed[int(off[r]):], int(lens[r]), K, M, NTASKS)
        cuts = np.flatnonzero(d[1:] != d[:-1]) + 1
        run = np.diff(np.concatenate(([0], cuts, [d.size])))           # runs of equal destinations, in k-mers
        longer += int((run > kc).sum()); shorter += int((run < kc).sum()); exact += int((run == kc).sum())
    assert longer >= 100 and shorter >= 100 and exact >= 1, (longer, shorter, exact)


@pytest.mark.parametrize("K", [5, 31, 51])
def test_crowded_index_straddles_the_read_index_window(K):
    """what tests/test_gpu_ext_ragged.py needs of crowded_index(), from pack()'s offsets alone"""
    seqs = R.crowded_index(K, R.SEED)
    assert seqs == R.crowded_index(K, R.SEED) and sum(len(s) for s in seqs) <= 200000
    packed, off, lens = R.pack(seqs)
    for a, b in zip((packed, off, lens), O.pack_reads(seqs)):
        assert np.array_equal(a, b)
    off, lens = off.astype(np.int64), lens.astype(np.int64)
    nb = (lens + 3) // 4
    n, T, run = len(seqs), R.INDEX_TILE, R.CROWDED_RUN
    # runs of empty reads: at the start and in the middle in front of a read with k-mers (same offset as that read), and at the end of the buffer
    empty = np.concatenate(([0], np.cumsum(lens == 0)))
    behind_run = [r for r in range(run, n) if empty[r] - empty[r - run] == run and lens[r] >= K]
    assert behind_run[0] == run and not lens[:run].any() and off[run] == 0
    assert any(lens[:r - run].max() >= K and lens[r + 1:].max() >= K and off[r - run] == off[r] for r in behind_run[1:])
    assert not lens[-run:].any() and lens[-run - 1] > 0 and (off[-run:] == packed.size).all()
    # tiles by the number of read offsets inside their 512 bytes, empty reads included
    tile = off // T
    count = np.bincount(tile)
    last = np.zeros(count.size, dtype=np.int64)
    last[tile] = np.arange(n)                                           # the last read that starts in the tile (offsets ascend)
    first = np.searchsorted(tile, np.arange(count.size))                # the first one
    holder = np.searchsorted(off + nb, np.arange(count.size) * T, side="right")      # the read that holds the tile's first byte
    for want in R.CROWDED_COUNTS:
        tiles = np.flatnonzero(count == want)
        assert (lens[last[tiles]] >= K).all()                           # a read with k-mers comes last, behind the window's edge or just inside it
        assert any(off[first[t]] == t * T for t in tiles), want         # the window starts at the tile's first read ...
        assert any(off[first[t]] > t * T and off[last[t]] + 3 == (t + 1) * T for t in tiles), want      # ... or one read earlier; the last read starts at the very end
    assert R.INDEX_WINDOW in R.CROWDED_COUNTS and R.INDEX_WINDOW - 2 in R.CROWDED_COUNTS and R.INDEX_WINDOW + 2 in R.CROWDED_COUNTS
    crowd = [t for t in np.flatnonzero(count >= 300) if lens[last[t]] >= K and lens[first[t]:last[t]].max() <= 4 and lens[first[t]:last[t]].min() == 0]
    assert crowd, count.max()
    # a record of several tiles; more than a window of reads follow it in its last tile, the last of them with k-mers
    assert any(count[t] > R.INDEX_WINDOW and lens[last[t]] >= K and holder[t] < first[t] and tile[holder[t]] <= t - 3 for t in range(3, count.size))
    # K ... K + 3 bases (the four packing phases) in threes with an empty and a one-base read, in every order
    threes = {tuple(lens[i:i + 3]) for i in range(n - 2)}
    for p in range(4):
        for order in ((0, 1, K + p), (0, K + p, 1), (1, 0, K + p), (1, K + p, 0), (K + p, 0, 1), (K + p, 1, 0)):
            assert order in threes, order
    # one small genome: most k-mers occur in several reads
    ores = O.count(packed, off.astype(np.uint64), lens.astype(np.uint32), k=K, m=min(17, K - 2), L=1, U=65535, ntasks=NTASKS, fast=True)
    assert (ores.cnt >= 2).sum() > len(ores.cnt) // 2


def _runs_of(seqs, K, off):
    """the maximal runs of at least K - 1 bases: (read, start, length, code, position of the run's first base in the packed buffer)"""
    read, start, n, code = R.base_runs(seqs)
    sel = n >= K - 1
    read, start, n, code = read[sel], start[sel], n[sel], code[sel]
    return read, start, n, code, 4 * off.astype(np.int64)[read] + start


_RUN_CASES = [(K, M, which, False) for K, M in R.HOMO_GRID + R.HOMO_NO_DROP_GRID for which in R.HOMO_WHICH] + \
    [(K, M, which, True) for K, M in R.HOMO_UNIFORM_GRID for which in R.HOMO_WHICH]


@pytest.mark.parametrize("K,M,which,uniform", _RUN_CASES)
def test_homopolymer_runs_meet_the_threshold_the_read_edges_and_the_holes(K, M, which, uniform):
    """what tests/test_gpu_certain_drops.py needs of homopolymer_runs(), for every (K, which) it uses.  The neighbours of the holes: at L = 1,
    U = 65535 the oracle keeps at least 1000 entries whose k-mer starts with min(K - 1, 24) equal bases without being a homopolymer; for K <= 25
    that means K - 1 equal bases and one other, of which there are 4 x 3 (fewer as canonical forms): at K = 21, 11 and 5 every one of them that
    is its own canonical form is in the list, for the bases whose runs are dropped, and together they hold at least 1000 instances."""
    seqs = R.homopolymer_runs(K, R.SEED, which, uniform)
    if (K, which) == (31, "both"):
        assert seqs == R.homopolymer_runs(K, R.SEED, which, uniform)
    packed, off, lens = R.pack(seqs)
    for a, b in zip((packed, off, lens), O.pack_reads(seqs)):
        assert np.array_equal(a, b)
    nbases = int(lens.astype(np.int64).sum())
    assert len(seqs) - 1 >= 4096 and 800000 <= nbases <= 1600000 and packed.size < 4 << 20
    if uniform:
        assert (lens == 150).all()
    else:
        assert int(lens.max()) >= 70000 and int(np.sort(lens)[-2]) <= 260 and int(lens.min()) >= min(K + 40, 150)
    every, sample = R.homopolymer_positions(seqs, K)
    last = R.as_packed(seqs[-1])
    assert not any(b * K in last for b in "ACGT") and every == sample                      # the last read has no run: every run is in the sketch's sample
    at, cg = sample["A"] + sample["T"], sample["C"] + sample["G"]
    reach = {"AT": (True, False), "CG": (False, True), "both": (True, True), "AT_over": (True, False)}[which]
    for n, must in zip((at, cg), reach):
        assert n >= 65537 if must else n < 60000, (at, cg)
    if which == "AT_over":
        assert 1000 <= cg <= 60000, cg
    if which in ("AT", "CG") and K >= 21:                                                   # (no run of the other family, and none by chance)
        assert (cg if which == "AT" else at) == 0
    mask = (1 if reach[0] else 0) | (2 if reach[1] else 0)
    for U in (40, 65535):
        assert R.expected_drops(seqs, K, U) == (mask, (every["A"] + every["T"] if reach[0] else 0) + (every["C"] + every["G"] if reach[1] else 0))
    # the runs that are dropped (K bases or more of a family that reaches the threshold) and the runs of K - 1 bases beside them
    read, start, n, code, g = _runs_of(seqs, K, off)
    fam = np.isin(code, [c for c in range(4) if reach[0 if c in (0, 3) else 1]])
    rl = lens.astype(np.int64)[read]
    drop = fam & (n >= K)
    assert int((drop & (start == 0)).sum()) >= 100 and int((drop & (start + n == rl)).sum()) >= 100
    assert int((drop & (start == 0) & (n == rl)).sum()) >= 50                               # whole reads
    inner = fam & (start > 0) & (start + n < rl)
    for d in (-1, 0, 1, 7, 8, 9):
        assert int((inner & (n == K + d)).sum()) >= 50, d
    assert {int(x) % 8 for x in g[drop]} == set(range(8))                                   # the lane's eight positions
    assert int((drop & (g // 2048 != (g + n - K) // 2048)).sum()) >= 20                     # a run's k-mers start in two parse tiles
    if not uniform:
        assert int((drop & (start > 65536)).sum()) >= 5                                    # positions beyond 2^16
    # two runs one base apart; a run directly behind a run of another base
    order = np.lexsort((start, read))
    r2, s2, n2, c2 = read[order], start[order], n[order], code[order]
    big = n2 >= K
    nxt_same_read = (r2[1:] == r2[:-1]) & big[1:] & big[:-1]
    assert int((nxt_same_read & (s2[1:] == s2[:-1] + n2[:-1] + 1) & (c2[1:] == c2[:-1])).sum()) >= 50
    assert int((nxt_same_read & (s2[1:] == s2[:-1] + n2[:-1]) & (c2[1:] == 3 - c2[:-1])).sum()) >= 50
    if which in ("both", "AT_over"):
        assert int((nxt_same_read & (s2[1:] == s2[:-1] + n2[:-1]) & (c2[:-1] == 0) & (c2[1:] == 1)).sum()) >= 20      # A then C
    assert sum("N" in s and "a" in s for s in seqs) >= 20 if reach[0] else sum("c" in s or "g" in s for s in seqs) >= 20
    # the neighbours of the holes stay in the list
    ores = O.count(packed, off, lens, k=K, m=M, L=1, U=65535, ntasks=NTASKS, fast=True)
    strs = [O.mer_string(w, K) for w in ores.keys[np.flatnonzero(_leading_equal(ores.keys, K) >= min(K - 1, 24))]]
    near = [s for s in strs if s != s[0] * K]
    if K - min(K - 1, 24) >= 5:
        assert len(near) >= 1000, len(near)
    else:
        runs_of = "".join(f for f, must in zip(("AT", "CG"), reach) if must)
        want = {s for b in runs_of for x in "ACGT" if x != b for s in (b * (K - 1) + x,) if s < R.revcomp(s)}
        assert len(want) >= 3 and want <= set(near), (want, near)
        assert int(ores.cnt[np.flatnonzero(_leading_equal(ores.keys, K) == K - 1)].sum()) >= 1000
    # what the list holds of the homopolymer k-mers themselves: nothing of a family beyond 65535 copies, the exact count of the others
    for name, n in (("A", at), ("C", cg)):
        got = [int(c) for c in ores.cnt[(ores.keys == O.string_to_words(name * K)).all(axis=1)]]
        assert got == ([n] if 0 < n <= 65535 else []), (name, n, got)


def _leading_equal(keys, K):
    """per k-mer (words, first base in the top bits of word 0) the number of leading bases equal to the first one"""
    n = keys.shape[0]
    out = np.zeros(n, dtype=np.int64)
    alive = np.ones(n, dtype=bool)
    first = (keys[:, 0] >> np.uint64(62)) & np.uint64(3)
    for i in range(K):
        b = (keys[:, i // 32] >> np.uint64(2 * (31 - i % 32))) & np.uint64(3)
        alive &= b == first
        out += alive
    return out


@pytest.mark.parametrize("base", ["A", "C"])
@pytest.mark.parametrize("K", R.HOMO_EDGE_K)
def test_homopolymer_edge_holds_exactly_the_copies_it_names(K, base):
    """what the threshold cases need of homopolymer_edge(): exactly 65535, 65536, 65537 copies, all inside the sample, in runs of every size of
    HOMO_SIZES; the oracle keeps the k-mer with 65535 copies and not with more"""
    M = 25 if K == 57 else 17
    fam = (base, R.revcomp(base))
    key = O.string_to_words(base * K)
    for copies, single in ((65535, False), (65536, False), (65537, False), (65537, True)):
        seqs = R.homopolymer_edge(K, R.SEED, copies, base, single_run=single)
        assert seqs == R.homopolymer_edge(K, R.SEED, copies, base, single_run=single)
        packed, off, lens = R.pack(seqs)
        for a, b in zip((packed, off, lens), O.pack_reads(seqs)):
            assert np.array_equal(a, b)
        assert len(seqs) >= 4096 + 256 and packed.size < 200000 and int((lens < K).sum()) >= 100
        every, sample = R.homopolymer_positions(seqs, K)
        assert every == sample and every[fam[0]] + every[fam[1]] == copies and sum(every.values()) == copies
        assert min(every[fam[0]], every[fam[1]]) > 0 or single
        assert R.expected_drops(seqs, K, 40) == R.expected_drops(seqs, K, 65535) == ((1 if base == "A" else 2, copies) if copies > 65536 else (0, 0))
        read, start, n, code = R.base_runs(seqs)
        runs = np.sort(n[n >= K] - K + 1)
        if single:
            assert runs.tolist() == [copies] and int(lens.max()) >= copies + K - 1
        else:
            assert set(R.HOMO_SIZES) <= set(runs.tolist()) and runs.size >= 150
        for U, n_far in ((65535, 100), (40, 100)):
            ores = O.count(packed, off, lens, k=K, m=M, L=1, U=U, ntasks=NTASKS, fast=True)
            got = [int(c) for c in ores.cnt[(ores.keys == key).all(axis=1)]]
            assert got == ([65535] if copies == 65535 and U == 65535 else []), (copies, U, got)
            assert len(ores.cnt) > n_far


def test_a_tiled_input_scales_the_oracles_list():
    """The argument the pinned-input cases of tests/test_gpu_certain_drops.py rest on (zero copy and the slab ingest start at 16 and 32 MB of packed
    reads, far beyond what the oracle counts in a test): r copies of an input one behind the other hold every k-mer r times as often, so the list
    at [r L, r U] is the list of one copy at [L, U] with r times the counts, task by task.  Here against the oracle itself, r = 3."""
    K, M, L, U, r = 31, 17, 1, 40, 3
    dna = R.pack(R.homopolymer_edge(K, R.SEED, 65537, "C"))
    one = O.count(*dna, k=K, m=M, L=L, U=U, ntasks=NTASKS, fast=True)
    many = O.count(*R.tiled(dna, r), k=K, m=M, L=r * L, U=r * U, ntasks=NTASKS, fast=True)
    assert len(one.cnt) > 1000 and np.array_equal(many.keys, one.keys) and np.array_equal(many.cnt, one.cnt * np.uint64(r))
    assert np.array_equal(many.task_off, one.task_off) and many.stats["total_kmers"] == r * one.stats["total_kmers"]


@pytest.mark.parametrize("K,M", R.GRID)
def test_long_records_sit_on_the_tile_edges(K, M):
    for variant in (0, 1):
        seqs = R.long_records(K, R.SEED, variant)
        packed, off, lens = R.pack(seqs)
        assert (int(off[1]) * 4) % 2048 == 0 and len(seqs[2]) < K
        if variant == 0:
            assert packed.size % 512 == 0
        else:
            assert packed.size % 4 != 0
        crossing = 0
        for r in range(len(seqs)):
            d = O.dests(packed[int(off[r]):], int(lens[r]), K, M, NTASKS)
            for _, start, n in O.supermers(d, K):
                g = int(off[r]) * 4 + start
                crossing += g // 2048 != (g + n - K) // 2048              # (first and last k-mer of the supermer start in different tiles)
        assert crossing >= 1, variant


@pytest.mark.parametrize("K,M", R.GRID)
def test_low_complexity_repeats_a_kmer_inside_a_supermer_below_16_bits(K, M):
    seqs = R.low_complexity(K, R.SEED)
    packed, off, lens = R.pack(seqs)
    twice = False
    for r in range(len(seqs)):
        if twice:
            break
        d = O.dests(packed[int(off[r]):], int(lens[r]), K, M, NTASKS)
        for _, start, n, b in O.supermers(d, K, packed[int(off[r]):]):
            mers = O.rep_mers(b, n, K)
            if len(np.unique(mers, axis=0)) < len(mers):
                twice = True
                break
    assert twice
    if K % 2 == 0:                                                    # a k-mer that is its own reverse complement occurs
        assert any(s[i:i + K] == R.revcomp(s[i:i + K]) for s in R.low_complexity_reads(K, R.SEED) for i in range(len(s) - K + 1))
    ores = O.count(packed, off, lens, k=K, m=M, L=1, U=65535, ntasks=NTASKS, fast=True)
    assert int(ores.cnt.sum()) == ores.stats["total_kmers"] and int(ores.cnt.max()) > 1000        # nothing beyond 65535: U = 65535 filters nothing


@pytest.mark.parametrize("K,M", R.GRID)
def test_past_16_bits_wraps_into_the_filter_range(K, M):
    seqs = R.past_16_bits(K, R.SEED)
    packed, off, lens = R.pack(seqs)
    four = [_canonical_words(s) for s in R.past_16_bits_kmers(K, R.SEED)]
    assert [n % 65536 for n in R.PAST_16_COPIES] == [65535, 0, 20, 17]

    def counts(res):
        return [[int(c) for c in res.cnt[(res.keys == w).all(axis=1)]] for w in four]

    ores = O.count(packed, off, lens, k=K, m=M, L=1, U=65535, ntasks=NTASKS, fast=True)
    assert counts(ores) == [[65535], [], [], []]
    assert ores.stats["total_kmers"] - int(ores.cnt.sum()) == sum(R.PAST_16_COPIES[1:])      # (and nothing else is beyond U)
    ores = O.count(packed, off, lens, k=K, m=M, L=15, U=40, ntasks=NTASKS, fast=True)
    assert counts(ores) == [[], [], [], []] and len(ores.cnt) > 1000
