"""The oracle's EXTENSION result against the definition (tests/brute_force.py: no minimizers, supermers or tasks) on the uneven inputs of
tests/ragged_inputs.py, no GPU: tests/test_gpu_ext_ragged.py holds every (k-mer, read, position) of the GPU's lists to the oracle, and this file
says the oracle is right there -- on runs of empty reads, tiles crowded with read offsets, positions beyond 2^18, k-mers with more than 2^16
instances and read ids up to 2^31 - 1."""
import numpy as np
import pytest

from oracle import hsk_oracle as O
from tests import brute_force as B
from tests import ragged_inputs as R

FAMILIES = {
    "crowded_index": lambda K: R.crowded_index(K, R.SEED),
    "ragged": lambda K: R.ragged(K, R.SEED),
    "long_records": lambda K: R.long_records(K, R.SEED, 0),
    "long_records_tail": lambda K: R.long_records(K, R.SEED, 1),
    "low_complexity": lambda K: R.low_complexity(K, R.SEED),
    "past_16_bits": lambda K: R.past_16_bits(K, R.SEED, apart=K >= 13),
}
RID_BASE = {"crowded_index": 1000, "ragged": 7, "long_records": 2000000000, "long_records_tail": 5, "low_complexity": 123456, "past_16_bits": 3}
GRID = [(5, 3), (31, 17), (51, 17), (77, 17)]
NTASKS = 8
_ROWS = {}


def _rows(family, K):
    """(reads, packed arrays, all instances sorted) of a family at K: built once, never written to"""
    if (family, K) not in _ROWS:
        _ROWS.clear()                                                   # (one input at a time: the cases come grouped by input)
        seqs = FAMILIES[family](K)
        _ROWS[family, K] = (seqs, R.pack(seqs), B.sort_triples(*B.instances(seqs, K, RID_BASE[family])))
    return _ROWS[family, K]


def _narrow(family):
    return (15, 40) if family == "past_16_bits" else (2, 40)


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("K,M", GRID)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_oracle_extension_equals_the_definition(family, K, M):
    seqs, (packed, off, lens), rows = _rows(family, K)
    assert len(rows[1]) == int(np.maximum(lens.astype(np.int64) - K + 1, 0).sum())
    for L, U in ((1, 65535), _narrow(family)):
        ores = O.count(packed, off, lens, k=K, m=M, L=L, U=U, ext=1, ntasks=NTASKS, rid_base=RID_BASE[family], fast=True)
        assert np.array_equal(np.diff(ores.payoff.astype(np.int64)), ores.cnt.astype(np.int64)) and int(ores.payoff[0]) == 0
        assert ores.cnt.size == 0 or (int(ores.cnt.min()) >= L and int(ores.cnt.max()) <= U)
        want = B.kept(rows, L, U)
        assert _same(B.result_triples(ores.keys, ores.cnt, ores.payoff, ores.rid, ores.pos), want), (L, U)
        assert len(want[1]) > 0 or (K == 5 and U == 40)                 # (512 canonical 5-mers: none of them is that rare)


@pytest.mark.parametrize("variant", [0, 1])
def test_long_records_hold_positions_beyond_18_bits(variant):
    family = "long_records_tail" if variant else "long_records"
    _, (packed, off, lens), rows = _rows(family, 31)
    ores = O.count(packed, off, lens, k=31, m=17, L=1, U=65535, ext=1, ntasks=NTASKS, rid_base=RID_BASE[family], fast=True)
    assert int(ores.pos.max()) == 2048 * 150 - 31 > 1 << 18 and int(rows[2].max()) == int(ores.pos.max())
    assert int(ores.rid.min()) == RID_BASE[family] and len(set(ores.rid.tolist())) == 4      # (the record shorter than K has no k-mer)


def test_read_ids_up_to_the_top_of_int32():
    seqs, (packed, off, lens), _ = _rows("crowded_index", 31)
    base = (1 << 31) - len(seqs)
    ores = O.count(packed, off, lens, k=31, m=17, L=1, U=65535, ext=1, ntasks=NTASKS, rid_base=base, fast=True)
    assert _same(B.result_triples(ores.keys, ores.cnt, ores.payoff, ores.rid, ores.pos), B.triples(seqs, 31, 1, 65535, rid_base=base))
    last = int(np.flatnonzero(lens >= 31)[-1])
    assert int(ores.rid.max()) == base + last and int(ores.rid.min()) == base + R.CROWDED_RUN and base + len(seqs) - 1 == (1 << 31) - 1


@pytest.mark.parametrize("K,M", [(31, 17), (51, 17), (77, 17)])
def test_past_16_bits_payloads(K, M):
    """the k-mer with 65 535 instances keeps all its payloads, the three with more have none, and the entries around them own exactly their own"""
    seqs, (packed, off, lens), rows = _rows("past_16_bits", K)
    four = [O.string_to_words(min(s, R.revcomp(s))) for s in R.past_16_bits_kmers(K, R.SEED)]
    ores = O.count(packed, off, lens, k=K, m=M, L=1, U=65535, ext=1, ntasks=NTASKS, rid_base=RID_BASE["past_16_bits"], fast=True)
    at = [np.flatnonzero((ores.keys == w).all(axis=1)) for w in four]
    assert [len(a) for a in at] == [1, 0, 0, 0]
    i = int(at[0][0])
    a, b = int(ores.payoff[i]), int(ores.payoff[i + 1])
    assert b - a == 65535 == int(ores.cnt[i]) and not ores.pos[a:b].any()
    first = R.past_16_bits_kmers(K, R.SEED)[0]
    copies = {r for r, s in enumerate(seqs) if s in (first, R.revcomp(first))}
    assert {int(r) - RID_BASE["past_16_bits"] for r in ores.rid[a:b]} == copies and len(copies) == 65535
    assert np.array_equal(np.diff(ores.payoff.astype(np.int64)), ores.cnt.astype(np.int64))
    assert int(ores.payoff[-1]) == len(ores.pos) == len(rows[1]) - sum(R.PAST_16_COPIES[1:])
    # the neighbours: entries next to the full one and next to where the dropped three would stand, payload by payload (the whole list is
    # compared in test_oracle_extension_equals_the_definition)
    want = B.kept(rows, 1, 65535)
    for j in {max(i - 1, 0), min(i + 1, len(ores.cnt) - 1)}:
        sel = (want[0] == ores.keys[j]).all(axis=1)
        a, b = int(ores.payoff[j]), int(ores.payoff[j + 1])
        assert sorted(zip(ores.rid[a:b].tolist(), ores.pos[a:b].tolist())) == sorted(zip(want[1][sel].tolist(), want[2][sel].tolist()))
