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
