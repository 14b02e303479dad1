"""Every table size of the finish for two- and three-word keys (hysortk_amd/csrc/hsk_agg.h: aggw_finish_kernel<cap, NW, W>): one 16-bit prefix
bin of one task holds about 2300 distinct k-mers, so it overflows the 1024-slot and the 2048-slot table and is done by the 4096-slot one (load
0.56: a key that outruns 32 triangular probes there, which would send the task the long way, is out of the question).  K = 51 and K = 77 on the
instance path (combine=0: the plain instances) and K = 51 through the combining extraction (the weighted instances).  The list must be the
oracle's, no task may take the long way, and the statistics must show the climb 1024 -> 2048 -> 4096.

The input is the background of tests/test_gpu_large_bins.py plus k-mers built the way its "many" case builds them (helpers imported, not copied);
the CPU-side assertions of _case() keep it from going vacuous."""
import numpy as np
import pytest

from tests import ragged_inputs as R
from tests import test_gpu_large_bins as LB

pytestmark = pytest.mark.gpu

NTASKS, M = 8, 17
NDISTINCT, TIMES = 2300, 3
SEED = 5151

_CASES = {}
_ORACLE = {}


def _case(K):
    """the input of a K, checked on the CPU: computed once, never written to"""
    from oracle import hsk_oracle as O
    from tests import util
    if K in _CASES:
        return _CASES[K]
    rng = np.random.default_rng([SEED, K])
    reads = LB.background(rng)
    # candidates through the oracle once: NDISTINCT that fall into bin 0 of one task as they are stored (an eighth of them lands in any one task,
    # and multi-word keys keep only half of them as written)
    r = O.count(*R.pack(LB.satellites(rng, K, "A" * K, 44000)), k=K, m=M, L=1, U=(1 << 31) - 1, ntasks=NTASKS, fast=True)
    task = np.repeat(np.arange(NTASKS), np.diff(r.task_off).astype(np.int64))
    b = LB.bin_of(r.keys, K)
    t0 = int(np.argmax(np.bincount(task[b == 0], minlength=NTASKS)))
    sel = np.flatnonzero((b == 0) & (task == t0))[:NDISTINCT]
    assert sel.size == NDISTINCT
    for s in util.result_strings(r.keys[sel], K):
        reads += [s] * TIMES
    dna = R.pack([reads[i] for i in rng.permutation(len(reads))])
    # every k-mer with its count: distinct k-mers and records of each (task, bin)
    full = O.count(*dna, k=K, m=M, L=1, U=(1 << 31) - 1, ntasks=NTASKS, fast=True)
    task = np.repeat(np.arange(NTASKS), np.diff(full.task_off).astype(np.int64))
    tb = task.astype(np.int64) * 65536 + LB.bin_of(full.keys, K).astype(np.int64)
    distinct = np.bincount(tb, minlength=NTASKS * 65536)
    records = np.bincount(tb, weights=full.cnt.astype(np.float64), minlength=NTASKS * 65536)
    big = np.flatnonzero(distinct > 2048)
    assert big.size == 1 and distinct[big[0]] <= 2400, (big, distinct[big])
    assert records[big[0]] < LB.AG_LARGE_BIN, records[big[0]]
    assert int(np.delete(distinct, big[0]).max()) < 700
    _CASES[K] = dna
    return dna


def _oracle(K, L, U):
    from oracle import hsk_oracle as O
    if (K, L, U) not in _ORACLE:
        _ORACLE[(K, L, U)] = O.count(*_case(K), k=K, m=M, L=L, U=U, ntasks=NTASKS, fast=True)
    return _ORACLE[(K, L, U)]


@pytest.mark.parametrize("L,U", [(1, 65535), (2, 40)])
@pytest.mark.parametrize("K,tuning", [(51, "combine=0"), (77, "combine=0"), (51, "combine_min_bytes=0")])
def test_a_bin_of_2300_distinct_kmers_climbs_to_the_4096_slot_table(K, tuning, L, U):
    import hysortk_amd as H
    from oracle import hsk_oracle as O
    dna, want = _case(K), _oracle(K, L, U)
    with H.Context(K=K, M=M, L=L, U=U, ntasks=NTASKS, profile=True, tuning=tuning) as c:
        res = c.count(dna)
        st = c.stats()
    print("K=%d %s L=%d U=%d: entries %d, combine_launches %d, redone_tasks %d, agg_retried_tasks %d, agg_launches %d"
          % (K, tuning, L, U, len(res.cnt), st["combine_launches"], st["redone_tasks"], st["agg_retried_tasks"], st["agg_launches"]))
    if tuning == "combine=0":
        assert st["combine_launches"] == 0, st
    else:
        assert st["combine_launches"] > 0, st                      # (a plan that left the extraction would run the plain instances a second time)
    assert np.array_equal(res.task_off, want.task_off)
    assert np.array_equal(res.kmers, want.keys)
    assert np.array_equal(res.cnt, want.cnt)
    assert H.histogram_text(res.histo) == O.histogram_text(want.cnt)
    assert st["redone_tasks"] == 0, st                              # nothing took the long way: the 4096-slot instance did the bin
    assert st["agg_retried_tasks"] >= 2 and st["agg_launches"] >= 3, st
