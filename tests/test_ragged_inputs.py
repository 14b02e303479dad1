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
