"""The combining extraction itself (scan_kernel with tile_sub, place_items_kernel, the bucket order, combine_kernel / combine2_kernel, the weighted
finish) against the CPU oracle, k-mer by k-mer, on inputs that are not 150-base reads of one length (tests/ragged_inputs.py; what they hold is
checked in tests/test_ragged_inputs.py): reads of every length around K and around the item cut, empty reads, N, lower case; records of hundreds
of tiles with their ends on tile edges; tandem repeats (one canonical k-mer many times in one item); k-mers with more than 2^16 copies (partial
pair counts that add up beyond 16 bits).  combine_min_bytes=0 lets inputs of this size take the plan; EVERY case asserts from the statistics
that the plan produced the list (a call that started again on the instance path would otherwise pass unnoticed)."""
import numpy as np
import pytest

from tests import ragged_inputs as R
from tests import _combine_worker as W

pytestmark = pytest.mark.gpu

FAMILIES = {
    "ragged": lambda K: R.ragged(K, R.SEED),
    "long_records": lambda K: R.long_records(K, R.SEED, 0),
    "long_records_tail": lambda K: R.long_records(K, R.SEED, 1),
    "low_complexity": lambda K: R.low_complexity(K, R.SEED),
    "past_16_bits": lambda K: R.past_16_bits(K, R.SEED),
}
_INPUT, _ORACLE = {}, {}


def _input(family, K):
    """(packed, read_off, read_len) of a family at K: built once"""
    if (family, K) not in _INPUT:
        _INPUT[family, K] = R.pack(FAMILIES[family](K))
    return _INPUT[family, K]


def _oracle(family, K, M, L, U, ntasks):
    """the oracle's list of an input: computed once, shared by every case on it, never written to"""
    from oracle import hsk_oracle as O
    key = (family, K, M, L, U, ntasks)
    if key not in _ORACLE:
        packed, off, lens = _input(family, K)
        _ORACLE[key] = O.count(packed, off, lens, k=K, m=M, L=L, U=U, ntasks=ntasks, fast=True)
    return _ORACLE[key]


def _check(family, K, M, L, U, ntasks, tuning, combining=True, plan=None):
    import hysortk_amd as H
    from oracle import hsk_oracle as O
    dna = _input(family, K)
    with H.Context(K=K, M=M, L=L, U=U, ntasks=ntasks, profile=True, plan=plan, tuning=tuning) as c:
        res = c.count(dna)
        st = c.stats()
    if combining:           # the combining extraction produced the list: its kernel ran over every k-mer, the instance path's extraction never did
        assert st["combine_launches"] > 0 and st["hist_launches"] == 0 and st["combine_kmers"] == res.info["total_kmers"], st
    else:
        assert st["combine_launches"] == 0 and st["combine_kmers"] == 0, st
    want = _oracle(family, K, M, L, U, ntasks)
    assert res.info["total_kmers"] == want.stats["total_kmers"]
    assert np.array_equal(res.task_off, want.task_off)
    assert np.array_equal(res.kmers, want.keys)
    assert np.array_equal(res.cnt, want.cnt)
    assert H.histogram_text(res.histo) == O.histogram_text(want.cnt)
    return res


def _grid():
    for K, M in R.GRID:
        for ntasks in ((1, 5, 16) if (K, M) in ((31, 17), (51, 17)) else (8,)):      # the padded batch, an odd count, two batches
            for family in FAMILIES:
                for L, U in ((1, 65535), (15, 40)) if family == "past_16_bits" else ((1, 65535), (2, 40)):
                    yield K, M, ntasks, family, L, U


@pytest.mark.parametrize("K,M,ntasks,family,L,U", list(_grid()))
def test_combining_extraction_on_uneven_inputs_vs_oracle(K, M, ntasks, family, L, U):
    res = _check(family, K, M, L, U, ntasks, "combine_min_bytes=0")
    if family == "past_16_bits" and U == 65535:               # (what the CPU test says of the oracle's list: exactly 65535 copies stay, one more do not)
        assert int(res.cnt.max()) == 65535


@pytest.mark.parametrize("tuning,why", [
    ("scan_place=1", "the scan places the items itself"),
    ("combine_bucket=1000000000", "tables written out in the middle of a bucket: partial pairs"),
    ("combine_prefix=11", "few, long bins: the ladder of the weighted finish"),
    ("pool_redzone=4096", "nothing is written past a block"),
])
@pytest.mark.parametrize("family", ["ragged", "low_complexity"])
@pytest.mark.parametrize("L,U", [(1, 65535), (2, 40)])
@pytest.mark.parametrize("K,M", [(31, 17), (51, 17)])
def test_combining_extraction_tunings_on_uneven_inputs_vs_oracle(K, M, L, U, family, tuning, why):
    _check(family, K, M, L, U, 5, "combine_min_bytes=0," + tuning)


@pytest.mark.parametrize("K,plan", [(31, None), (51, None), (77, None), (31, "no_aggregation"), (31, "full_sort")])
@pytest.mark.parametrize("L,U", [(1, 65535), (15, 40)])
def test_counts_beyond_16_bits_on_the_instance_path(K, plan, L, U):
    """65535, 65536, 65536 + 20 and 2 x 65536 + 17 copies through every finish that counts records: a count that wrapped at 2^16 would come back
    as 0, 20 or 17, and 20 and 17 lie inside [15, 40]"""
    _check("past_16_bits", K, 17, L, U, 8, "combine=0", combining=False, plan=plan)


def _byte_copies(nbytes_min, seed, K=31, genome=2000000):
    """ragged lengths again, cut from the packed genome at whole bytes: every read is a byte copy (pad bits cleared), built without a string per read"""
    rng = np.random.default_rng([seed, 7])
    g = rng.integers(0, 256, size=genome // 4, dtype=np.uint8)
    classes = np.array(R.ragged_lengths(K), dtype=np.int64)
    n = int(nbytes_min / ((classes + 3) // 4).mean()) + len(classes)
    lens = classes[np.arange(n) % len(classes)]
    nb = (lens + 3) // 4
    off = np.concatenate(([0], np.cumsum(nb)[:-1]))
    start = rng.integers(0, g.size - int(nb.max()), size=n)
    packed = g[np.repeat(start - off, nb) + np.arange(int(nb.sum()), dtype=np.int64)]
    part = np.flatnonzero(lens % 4)
    packed[off[part] + nb[part] - 1] &= (0xFF << (2 * (4 - lens[part] % 4))).astype(np.uint8)
    return packed, off.astype(np.uint64), lens.astype(np.uint32)


def test_uneven_reads_from_pinned_memory_in_slabs():
    """44 MB of uneven reads from pinned memory: the ingest runs in slabs pipelined with the scan and the item placement, the store is laid out
    [slab][virtual task].  Too large for the oracle: same digest as the instance path on the same reads."""
    import hysortk_amd as H
    packed, off, lens = _byte_copies(44 << 20, R.SEED)
    # hsk_count ingests pinned input in slabs from 32 MB of packed reads on (slab_ingest in hsk_count; h2d_slabs at its default of 16, set nowhere
    # here).  No statistic counts the slabs, so the input is held to that limit by name: if the limit is raised, SLAB_INGEST_MIN and the size follow
    SLAB_INGEST_MIN = 32 << 20
    assert packed.size >= SLAB_INGEST_MIN + (8 << 20) and int(off[-1]) + (int(lens[-1]) + 3) // 4 == packed.size
    pinned = (H.pinned_empty(packed.size, np.uint8), H.pinned_empty(off.size, np.uint64), H.pinned_empty(lens.size, np.uint32))
    try:
        for dst, src in zip(pinned, (packed, off, lens)):
            dst[:] = src
        seen = []
        for tuning in ("combine=0", "combine_min_bytes=0", "combine_min_bytes=0,scan_place=1"):
            with H.Context(K=31, M=17, L=2, U=200, ntasks=16, profile=True, tuning=tuning) as c:
                r = c.count(pinned)
                st = c.stats()
            if tuning == "combine=0":
                assert st["combine_launches"] == 0, st
            else:
                assert st["combine_launches"] > 0 and st["hist_launches"] == 0 and st["combine_kmers"] == r.info["total_kmers"] and st["parse_fallbacks"] == 0, (tuning, st)
            seen.append((W.digest(r), len(r), r.info["total_kmers"]))
    finally:
        for a in pinned:
            H.pinned_free(a)
    assert seen[0][1] > 100000 and seen[0][2] == int(np.maximum(lens.astype(np.int64) - 30, 0).sum())
    assert seen[1] == seen[0] and seen[2] == seen[0]
