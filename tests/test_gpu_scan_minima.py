"""scan_kernel's window minima through v_min_f64 (hysortk_amd/csrc/hsk_fmin.h, step 3 of scan_kernel in hsk_parse.h) against the CPU oracle, on
inputs that hold what the clamped double-precision minimum can get wrong: windows whose hashes ALL lie in the sentinel class (top word from
0x7FEFFFFF up: the wave has to take the integer compares) and windows whose minimum is a denormal bit pattern (top word below 0x00100000: a
flushed denormal would come back as zero).  The test counts both from the oracle's m-mer hashes before it looks at the GPU.

The (K, M) pairs: (31, 17) a window of 15; (24, 17) a window of 8, the edge of the branch; (51, 17) a window of 35, block minima; (31, 25) a
window of 7, the narrow path that the change leaves alone, as a control.

Two kinds of check.  hsk_stage_destinations gives the task of every k-mer position with 1024 tasks (a wrong minimum shows in all but 1/1024 of
cases): that call runs the general parse kernels (parse_kernel<PARSE_DUMP>), so it pins the inputs, the oracle's destinations and the general
path, not the scan.  The scan itself is held by the whole call: hsk_count with 64 tasks, whose list is compared task by task (a k-mer with
a wrong window minimum lands in another task's range in all but 1/64 of cases) with the oracle -- the combining extraction, the instance path
(HSK_FLAG_NO_COMBINE) and, with parse_rec_cap forced low, the general kernels on the same reads; the statistics say which parse ran."""
import numpy as np
import pytest

from tests import ragged_inputs as R

pytestmark = pytest.mark.gpu

PAIRS = [(31, 17), (24, 17), (51, 17), (31, 25)]
SEED = 31017
SENTINEL_TOP = 0x7FEFFFFF           # hsk_fmin.h FMIN_SENTINEL
DENORMAL_TOP = 0x00100000
REPEAT_UNITS = ["A", "C", "G", "T", "AC", "AG", "AT", "CG", "CT", "GT", "TA", "GC"]
_CACHE = {}


def _reads():
    """~2 Mbp: 13000 random reads of 150 bases; 640 ragged reads of 120 ... 183 bases (every read starts on a byte, so their last k-mers end at every
    offset inside a lane's eight positions, and so do the first ones of their successors); homopolymer and dinucleotide repeats of 150 - 400 bases"""
    if "reads" not in _CACHE:
        rng = np.random.default_rng([SEED, 1])
        reads = [R.random_seq(rng, 150) for _ in range(13000)]
        reads += [R.random_seq(rng, 120 + i % 64) for i in range(640)]
        first_repeat = len(reads)
        for unit in REPEAT_UNITS:
            for n in (150, 151, 277, 400):
                reads.append((unit * (n // len(unit) + 1))[:n])
        order = rng.permutation(len(reads))
        _CACHE["reads"] = [reads[i] for i in order]
        _CACHE["repeat_reads"] = [int(j) for j in np.flatnonzero(order >= first_repeat)]
        _CACHE["arrays"] = R.pack(_CACHE["reads"])
    return _CACHE["reads"], _CACHE["arrays"], _CACHE["repeat_reads"]


def _windows(K, M):
    """from the oracle's m-mer hashes: (positions whose whole window is in the sentinel class, positions whose window minimum is a denormal pattern,
    repeat reads whose every m-mer hash is in the sentinel class)"""
    if ("win", K, M) not in _CACHE:
        from oracle import hsk_oracle as O
        reads, (packed, off, lens), repeats = _reads()
        W = K - M + 1
        n_class = n_denormal = 0
        class_repeats = []
        hs, nk = [], []
        for r in range(len(reads)):
            h = O.mmer_hashes(packed[int(off[r]):], int(lens[r]), M)
            hs.append(h); nk.append(max(0, int(lens[r]) - K + 1))
        for r in repeats:
            if hs[r].size and int(hs[r].min() >> np.uint64(32)) >= SENTINEL_TOP:
                class_repeats.append(r)
        allh = np.concatenate(hs)
        start = np.concatenate(([0], np.cumsum([h.size for h in hs])))[:-1]
        mn = allh.copy()
        for j in range(1, W):                                       # minimum of allh[p .. p + W): windows that run over a read's end are not looked at
            mn[:-j] = np.minimum(mn[:-j], allh[j:])
        valid = np.zeros(allh.size, dtype=bool)
        for s, n in zip(start, nk):
            valid[s:s + n] = True
        top = (mn[valid] >> np.uint64(32)).astype(np.int64)
        n_class, n_denormal = int((top >= SENTINEL_TOP).sum()), int((top < DENORMAL_TOP).sum())
        _CACHE["win", K, M] = (n_class, n_denormal, class_repeats)
    return _CACHE["win", K, M]


def _oracle(K, M, L, U, ntasks):
    if ("count", K, M, L, U, ntasks) not in _CACHE:
        from oracle import hsk_oracle as O
        packed, off, lens = _reads()[1]
        _CACHE["count", K, M, L, U, ntasks] = O.count(packed, off, lens, k=K, m=M, L=L, U=U, ntasks=ntasks, fast=True)
    return _CACHE["count", K, M, L, U, ntasks]


def _assert_input_holds_the_cases(K, M):
    n_class, n_denormal, class_repeats = _windows(K, M)
    print("K %d M %d: %d positions with the whole window in the sentinel class, %d with a denormal minimum, %d repeat reads in the class" %
          (K, M, n_class, n_denormal, len(class_repeats)))
    assert len(class_repeats) >= 1, "no repeat read has all its m-mer hashes in the sentinel class"
    assert n_class >= 20 and n_denormal >= 100, (n_class, n_denormal)


@pytest.mark.parametrize("K,M", PAIRS)
def test_destinations_vs_oracle_with_1024_tasks(K, M):
    import hysortk_amd as H
    from oracle import hsk_oracle as O
    _assert_input_holds_the_cases(K, M)
    reads, (packed, off, lens), _ = _reads()
    with H.Context(K=K, M=M, ntasks=1024) as c:
        dest, doff = c.stage_destinations((packed, off, lens))
    bad = []
    for r in range(len(reads)):
        want = O.dests(packed[int(off[r]):], int(lens[r]), K, M, 1024)
        if not np.array_equal(dest[int(doff[r]):int(doff[r + 1])], want):
            bad.append(r)
    assert not bad, "reads with a wrong destination: %s" % bad[:10]


@pytest.mark.parametrize("plan,tuning,fallback,why", [
    (None, "combine_min_bytes=0", False, "scan_kernel with the minimizer bits, the combining extraction"),
    ("no_combine", None, False, "scan_kernel with plain records, the instance path"),
    ("no_combine", "parse_rec_cap=64", True, "the scan's record store runs over: parse_kernel and emit_kernel answer for the same reads"),
], ids=["combine", "instance", "general_kernels"])
@pytest.mark.parametrize("K,M", PAIRS)
def test_whole_call_vs_oracle_task_by_task(K, M, plan, tuning, fallback, why):
    import hysortk_amd as H
    _assert_input_holds_the_cases(K, M)
    arrays = _reads()[1]
    with H.Context(K=K, M=M, L=1, U=65535, ntasks=64, profile=True, plan=plan, tuning=tuning) as c:
        res = c.count(arrays)
        st = c.stats()
    assert (st["parse_fallbacks"] > 0) == fallback, st
    if plan is None:
        assert st["combine_launches"] > 0 and st["combine_kmers"] == res.info["total_kmers"], st
    else:
        assert st["combine_launches"] == 0, st
    want = _oracle(K, M, 1, 65535, 64)
    assert res.info["total_kmers"] == want.stats["total_kmers"]
    assert np.array_equal(res.task_off, want.task_off)
    assert np.array_equal(res.kmers, want.keys)
    assert np.array_equal(res.cnt, want.cnt)
