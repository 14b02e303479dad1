"""Prefix bins of very many records (hysortk_amd/csrc/hsk_agg.h: AggLarge) in every record shape: one repeat read many times over puts more
than AG_LARGE_BIN = 65536 records into ONE 16-bit prefix bin of ONE task.  The bin is cut into slices that many workgroups count (and, with
EXTENSION, place); the list must be the oracle's and the one the same context gives with the slices switched off (agg_large=0), and
hsk_stats::agg_large_bins must say that the slices ran.  The inputs are small (no sketch, no combining extraction: combine=0 says so by name).

The bin holds more than the repeat: a few dozen k-mers that share its 16 prefix bits and are seen 3 .. 12 times, so that kept entries (and
with EXTENSION their payloads) come out of the sliced bin.  agg_bin_of is restated here; the CPU-side assertions of _case() keep the inputs
from going vacuous (they hold without a GPU as well)."""
import numpy as np
import pytest

from tests import ragged_inputs as R

pytestmark = pytest.mark.gpu

AG_LARGE_BIN = 1 << 16
AGL_TAB = 2048
NTASKS, M, L = 8, 17, 2
SEED = 4242


def prefix_positions(K):
    """the eight bases that make the 16-bit bin prefix (agg_bin_of): the first bases of the most significant word, continued by the first of the
    word below when the top word holds fewer than eight (AggArgs::top_bits = 2 x its bases)"""
    nw = (K + 31) // 32
    top = min(8, K - 32 * (nw - 1))
    return [32 * (nw - 1) + j for j in range(top)] + ([32 * (nw - 2) + j for j in range(8 - top)] if top < 8 else [])


def bin_of(keys, K):
    """agg_bin_of on a [n, nw] key array"""
    keys = np.asarray(keys, dtype=np.uint64)
    nw = keys.shape[1]
    top_bits = 16 if nw == 1 else min(16, 2 * (K - 32 * (nw - 1)))
    if 0 < top_bits < 16:
        return ((keys[:, nw - 1] >> np.uint64(64 - top_bits)) << np.uint64(16 - top_bits)) | (keys[:, nw - 2] >> np.uint64(48 + top_bits))
    return keys[:, nw - 1] >> np.uint64(48)


def background(rng, nreads=2000, read_len=150, coverage=30):
    g = R.random_seq(rng, nreads * read_len // coverage)
    out = []
    for _ in range(nreads):
        at = int(rng.integers(0, len(g) - read_len + 1))
        s = g[at:at + read_len]
        out.append(R.revcomp(s) if rng.integers(0, 2) else s)
    return out


def satellites(rng, K, repeat, n):
    """n reads of exactly K bases: the repeat's bases at the bin-prefix positions, random elsewhere"""
    out = []
    P = prefix_positions(K)
    for _ in range(n):
        s = list(R.random_seq(rng, K))
        for p in P:
            s[p] = repeat[p]
        out.append("".join(s))
    return out


def build_input(K, kind):
    """kind "A": all-A reads; "AC": (AC)n reads in both rotations as well (two more large bins); "many": no repeat, 3000 distinct k-mers of one
    prefix bin and task 23 times each (a large bin of another kind)"""
    rng = np.random.default_rng([SEED, K, {"A": 0, "AC": 1, "many": 2}[kind]])
    reads = background(rng)
    per_read = 151 - K
    if kind == "many":
        # candidates through the oracle once: 3000 that fall into bin 0 of one task as they are stored (an eighth of them lands in any one task, and
        # multi-word keys keep only half of them as written, the others as their reverse complement in other bins)
        from oracle import hsk_oracle as O
        from tests import util
        r = O.count(*R.pack(satellites(rng, K, "A" * K, 56000)), k=K, m=M, L=1, U=(1 << 31) - 1, ntasks=NTASKS, fast=True)
        task = np.repeat(np.arange(NTASKS), np.diff(r.task_off).astype(np.int64))
        b = bin_of(r.keys, K)
        t0 = int(np.argmax(np.bincount(task[b == 0], minlength=NTASKS)))
        sel = np.flatnonzero((b == 0) & (task == t0))[:3000]
        assert sel.size == 3000
        for s in util.result_strings(r.keys[sel], K):
            reads += [s] * 23
    else:
        reads += ["A" * 150] * (70000 // per_read + 1)
        if kind == "AC":
            unit = "AC" * 76
            reads += [unit[:150]] * (70000 // per_read + 1) + [unit[1:151]] * (70000 // per_read + 1)
        for s in satellites(rng, K, "A" * K, 240):
            reads += [s] * int(rng.integers(3, 13))
    return R.pack([reads[i] for i in rng.permutation(len(reads))])


_CASES = {}


def _case(K, ext, kind="A"):
    """input, the oracle's lists for U = 65535 and U = 40, and what the CPU can say about the repeat's bin: computed once, never written to"""
    from oracle import hsk_oracle as O
    key = (K, ext, kind)
    if key in _CASES:
        return _CASES[key]
    dna = build_input(K, kind)
    want = {U: O.count(*dna, k=K, m=M, L=L, U=U, ext=ext, ntasks=NTASKS, fast=True) for U in (65535, 40)}
    # every k-mer with its count (L = 1, no upper limit worth the name): the records of each (task, bin)
    full = O.count(*dna, k=K, m=M, L=1, U=(1 << 31) - 1, ext=0, ntasks=NTASKS, fast=True)
    task = np.repeat(np.arange(NTASKS), np.diff(full.task_off).astype(np.int64))
    tb = task.astype(np.int64) * 65536 + bin_of(full.keys, K).astype(np.int64)
    records = np.bincount(tb, weights=full.cnt.astype(np.float64), minlength=NTASKS * 65536)
    distinct = np.bincount(tb, minlength=NTASKS * 65536)
    large = np.flatnonzero(records >= AG_LARGE_BIN)
    w = want[65535]
    wtask = np.repeat(np.arange(NTASKS), np.diff(w.task_off).astype(np.int64))
    wtb = wtask.astype(np.int64) * 65536 + bin_of(w.keys, K).astype(np.int64)
    if kind == "many":
        assert large.size == 1 and distinct[large[0]] > AGL_TAB, (large, distinct[large])
    else:
        assert large.size == (3 if kind == "AC" else 1), large
        zero = np.zeros((1, (K + 31) // 32), dtype=np.uint64)                         # the all-A k-mer: bin 0 of its task
        rep = [b for b in large if b % 65536 == int(bin_of(zero, K)[0])]
        assert len(rep) == 1 and distinct[rep[0]] <= 200
        assert int((wtb == rep[0]).sum()) >= 2, "the repeat's bin must hold kept entries"
        assert int(full.cnt.max()) > 65535 and int(w.cnt.max()) <= 65535               # the repeat itself is never kept
    _CASES[key] = (dna, want, int(large.size))
    return _CASES[key]


def _payload_sets(res_off, cnt, pos, rid):
    out = []
    for i in range(len(cnt)):
        a = int(res_off[i]); b = a + int(cnt[i])
        out.append(np.sort((rid[a:b].astype(np.int64) << 32) | pos[a:b].astype(np.int64)))
    return out


def _run(dna, K, ext, U, tuning):
    import hysortk_amd as H
    with H.Context(K=K, M=M, L=L, U=U, EXT=ext, ntasks=NTASKS, tuning=tuning) as c:
        res = c.count(dna)
        st = c.stats()
    return res, st


def _check(K, ext, kind, extra=""):
    """the three assertions of a case, for U = 65535 and U = 40"""
    dna, want, nlarge = _case(K, ext, kind)
    for U in (65535, 40):
        res, st = _run(dna, K, ext, U, "combine=0" + extra)
        off, st0 = _run(dna, K, ext, U, "combine=0,agg_large=0" + extra)
        w = want[U]
        print("K=%d ext=%d %s U=%d: entries %d, agg_large_bins %d, agg_large_slices %d" % (K, ext, kind, U, len(res.cnt), st["agg_large_bins"], st["agg_large_slices"]))
        # 1. the oracle's list
        for r in (res, off):
            assert r.info["total_kmers"] == w.stats["total_kmers"]
            assert np.array_equal(r.task_off, w.task_off) and np.array_equal(r.kmers, w.keys) and np.array_equal(r.cnt, w.cnt)
        # 2. byte for byte what the same configuration gives without the slices
        assert res.kmers.tobytes() == off.kmers.tobytes() and res.cnt.tobytes() == off.cnt.tobytes() and res.task_off.tobytes() == off.task_off.tobytes()
        assert np.array_equal(res.histo, off.histo)
        if ext:
            assert np.array_equal(res.payload_off, off.payload_off)
            po = res.payload_off.astype(np.int64)
            n = len(res.cnt)
            assert po.size == n + 1 and (n == 0 or (np.all(np.diff(po[:n]) >= res.cnt[:-1].astype(np.int64)) and po[n] >= po[n - 1] + int(res.cnt[-1])))
            got, ref, alt = _payload_sets(po, res.cnt, res.pos, res.rid), _payload_sets(w.payoff.astype(np.int64), w.cnt, w.pos, w.rid), _payload_sets(off.payload_off.astype(np.int64), off.cnt, off.pos, off.rid)
            for i in range(n):
                assert np.array_equal(got[i], ref[i]) and np.array_equal(got[i], alt[i]), (i, int(res.cnt[i]))
        # 3. the slices ran, and only when they are switched on
        if kind == "many":
            assert st["agg_large_bins"] == 0 and st["agg_large_slices"] == 0, st
        else:
            assert st["agg_large_bins"] >= nlarge and st["agg_large_slices"] >= 2 * st["agg_large_bins"], st
        assert st0["agg_large_bins"] == 0 and st0["agg_large_slices"] == 0, st0


NEW_SHAPES = [(77, 0, "A"), (69, 0, "A"), (35, 0, "A"), (31, 1, "A"), (51, 1, "A"), (77, 1, "A"), (35, 0, "AC"), (31, 1, "AC")]


@pytest.mark.parametrize("K,ext,kind", NEW_SHAPES)
def test_large_bins_of_every_shape_are_counted_in_slices(K, ext, kind):
    if K == 69:
        assert 0 < min(16, 2 * (K - 64)) < 16               # the prefix is split between words 2 and 1
    _check(K, ext, kind)


@pytest.mark.parametrize("K,ext", [(31, 0), (51, 0)])
def test_shapes_that_were_sliced_before_are_counted_too(K, ext):
    _check(K, ext, "A")


@pytest.mark.parametrize("K,ext", [(31, 0), (77, 0), (31, 1)])
def test_a_large_bin_of_many_distinct_kmers_is_counted_the_old_way(K, ext):
    _check(K, ext, "many")


@pytest.mark.parametrize("K,ext", [(77, 0), (35, 0), (31, 1), (77, 1)])
def test_large_bins_write_nothing_past_a_block(K, ext):
    _check(K, ext, "A", ",pool_redzone=4096")
