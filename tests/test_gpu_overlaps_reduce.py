"""hsk_overlaps_reduce (include/hsk.h): the string graph of a list of overlap rows in HBM -- contained reads out, dovetails turned into arcs,
transitive arcs marked -- against the definition in plain Python (tests/strgraph_ref.py, itself held to hand-written rows by
tests/test_strgraph_ref.py).  The rows are fabricated from layouts of reads on a line (strgraph_ref.layout_rows): only lengths are needed.
Everything is integer work and compared for equality: the class of every row, the kept rows, the contained bits and every count.  Every case
runs with wave_degree 0 (the library's default), 1 (every vertex by a workgroup) and 0xFFFFFFFF (none), unless it says otherwise, and must
give the same result.  tests/test_gpu_overlaps_reduce_hubs.py holds the wave path's length rule, dead records, narrowing and grid-stride loop
to the same reference on vertices of several chunks, and has the tile edges, the 33-bit sums and the top of the read-id range."""
import ctypes as C

import numpy as np
import pytest

from tests import strgraph_ref as S
from tests.test_strgraph_ref import hand_cases

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
DEGREES = (0, 1, NONE)
CHUNK = 1024                                              # RD_CHUNK of hysortk_amd/csrc/hsk_reduce.h: the records of out(v) the wave path holds in LDS at a time
COUNTS = S.NAMES + ("input_rows", "contained_reads", "arcs", "max_degree", "wave_vertices")


@pytest.fixture(scope="module")
def H():
    import hysortk_amd
    return hysortk_amd


@pytest.fixture(scope="module")
def ctx(H):
    with H.Context(K=31) as c:
        yield c


class _DeviceRows:
    """rows put into HBM by the HIP runtime itself (the library has no call that uploads a list and leaves it as it is)"""
    _hip = None

    def __init__(self, rows):
        import ctypes.util
        import os
        if _DeviceRows._hip is None:
            name = ctypes.util.find_library("amdhip64") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")
            _DeviceRows._hip = C.CDLL(name)
            _DeviceRows._hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            _DeviceRows._hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            _DeviceRows._hip.hipFree.argtypes = [C.c_void_p]
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        p = C.c_void_p()
        assert self._hip.hipMalloc(C.byref(p), max(rows.nbytes, 64)) == 0
        self.ptr = p.value
        assert self._hip.hipMemcpy(self.ptr, rows.ctypes.data_as(C.c_void_p), rows.nbytes, 1) == 0      # (1: host to device; returns when the copy is done)
        assert self.ptr % 16 == 0

    def data_ptr(self):
        return self.ptr

    def close(self):
        if self.ptr:
            self._hip.hipFree(self.ptr)
            self.ptr = None


def _to_device(rows):
    return _DeviceRows(rows)


def _device_list(H, rows, t):
    z = np.zeros(0, np.uint64)
    return H.Overlaps(z, z, z, z, z, z, rows_dev=t.data_ptr(), n=np.asarray(rows).reshape(-1, 6).shape[0])


def _check(H, c, g, rows, ref, what):
    """one result against the reference: classes, kept rows, contained bits, every count"""
    n = rows.shape[0]
    if g.row_class is None:                               # left in HBM: fetch all three
        assert g.edges.rows().shape == (0, 6) and (g.edges.rows_dev or not len(g)) and g.row_class_dev and g.contained_dev
        cls, contained = g.host_copy()
        kept = c.d2h(g.edges.rows_dev, len(g) * 48).view(np.uint64).reshape(len(g), 6) if len(g) else np.zeros((0, 6), np.uint64)
    else:
        cls, contained, kept = g.row_class, g.contained, g.edges.rows()
    want = S.expected_info(ref, n, g.info["wave_degree"])
    print("%s: %d rows, %s, arcs %d, max degree %d, wave vertices %d (threshold %d), %.3f ms (classify %.3f, sort %.3f, reduce %.3f)" % (
        what, n, " ".join("%s %d" % (k, g.info[k]) for k in S.NAMES), g.info["arcs"], g.info["max_degree"], g.info["wave_vertices"], g.info["wave_degree"], g.info["ms_total"],
        g.info["ms_classify"], g.info["ms_sort"], g.info["ms_reduce"]))
    bad = np.flatnonzero(cls != ref["row_class"]) if cls.shape == ref["row_class"].shape else None
    assert bad is not None and bad.size == 0, "%s: row %s has class %s, the reference says %s" % (what, bad[:1], cls[bad[:1]], ref["row_class"][bad[:1]])
    assert np.array_equal(kept, ref["kept"]) and len(g) == ref["kept"].shape[0], what
    assert np.array_equal(contained, ref["contained"]), what
    assert {k: g.info[k] for k in COUNTS} == {k: want[k] for k in COUNTS}, what
    assert sum(g.info[k] for k in S.NAMES) == n == g.info["input_rows"]


def _all_degrees(H, c, rows, lens, ref, fuzz, rid_base=0, degrees=DEGREES, src=None, what=""):
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 6)
    src = H.Overlaps.from_rows(rows) if src is None else src
    for wd in degrees:
        for on_device in (False, True):
            with src.reduce(c, np.asarray(lens, dtype=np.uint32), rid_base=rid_base, fuzz=fuzz, wave_degree=wd, on_device=on_device) as g:
                assert g.info["wave_degree"] == (wd if wd else g.info["wave_degree"]) and g.info["wave_degree"] >= 1
                _check(H, c, g, rows, ref, "%s wave_degree %d on_device %d" % (what, wd, on_device))


# ---- 1. the rows by hand -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", hand_cases(), ids=lambda k: k[0])
def test_hand_rows(H, ctx, case):
    name, rows, lens, fuzz, classes, contained = case
    ref = S.reduce_rows(rows, lens, fuzz=fuzz)
    assert ref["row_class"].tolist() == classes
    _all_degrees(H, ctx, rows, lens, ref, fuzz, what=name)                                # host rows
    t = _to_device(rows)
    _all_degrees(H, ctx, rows, lens, ref, fuzz, src=_device_list(H, rows, t), what=name + " (rows in HBM)")
    t.close()
    ref7 = S.reduce_rows(_moved(rows, 7), lens, rid_base=7, fuzz=fuzz)                    # the same reads numbered from 7
    _all_degrees(H, ctx, _moved(rows, 7), lens, ref7, fuzz, rid_base=7, what=name + " (rid_base 7)")
    assert ref7["row_class"].tolist() == classes


def _moved(rows, base):
    out = np.array(rows, dtype=np.uint64).reshape(-1, 6).copy()
    out[:, 0] += np.uint64(base << 32 | base)
    return out


# ---- 2. random layouts ---------------------------------------------------------------------------------------------------------------------------
SEED, NREADS, GENOME, MIN_OV = 11, 3000, 40000, 30


def _stray_rows(rng, lens, live, pairs_taken, starts, count, internal):
    """fabricated rows between reads that lie far apart on the line: dovetails of all four kinds (they have no witness: KEPT), or rows that
    stop inside both reads (INTERNAL)"""
    rows = []
    while len(rows) < count:
        a, b = sorted(rng.choice(live, 2, replace=False).tolist())
        if abs(int(starts[a]) - int(starts[b])) < 2000 or (a, b) in pairs_taken:
            continue
        pairs_taken.add((a, b))
        la, lb, ov, o = int(lens[a]), int(lens[b]), int(rng.integers(30, 60)), int(rng.integers(0, 2))
        if internal:
            rows.append(S.make_row(a, b, o, 5, la - 5, 7, lb - 7, la, lb))
        elif rng.integers(0, 2):                          # a in front: a_hi == la
            rows.append(S.make_row(a, b, o, la - ov, la, *((0, ov) if o == 0 else (lb - ov, lb)), la, lb))
        else:
            rows.append(S.make_row(a, b, o, 0, ov, *((lb - ov, lb) if o == 0 else (0, ov)), la, lb))
    return np.array(rows, dtype=np.uint64)


def _random_case(jitter):
    rng = np.random.default_rng(SEED)
    starts, lens, strands = S.random_layout(rng, NREADS, GENOME, 100, 400)
    base = S.layout_rows(starts, lens, strands, MIN_OV, jitter=jitter, rng=rng)
    e = base[:, 4] & np.uint64(15)
    gone = np.zeros(NREADS, bool)                         # the reads some row marks contained
    lo = np.uint64(0xFFFFFFFF)
    gone[((base[:, 0] >> np.uint64(32)) & np.uint64(0x7FFFFFFF)).astype(np.int64)[(e & np.uint64(3)) == 3]] = True
    gone[(base[:, 0] & lo).astype(np.int64)[((e & np.uint64(3)) != 3) & ((e & np.uint64(12)) == 12)]] = True
    live = np.flatnonzero(~gone)
    taken = set()
    stray = _stray_rows(rng, lens, live, taken, starts, base.shape[0] // 50, False)
    inner = _stray_rows(rng, lens, live, taken, starts, base.shape[0] // 50, True)
    rows = np.concatenate([base, stray, inner])
    rows = rows[np.argsort(rows[:, 0] & np.uint64((1 << 63) - 1), kind="stable")]
    return starts, lens, rows, {tuple(p) for p in S.row_pairs(stray)}


@pytest.fixture(scope="module")
def layouts():
    return {jitter: _random_case(jitter) for jitter in (0, 3)}


@pytest.mark.parametrize("jitter,fuzz", [(0, 0), (0, 10), (3, 0), (3, 10)])
def test_random_layouts(H, ctx, layouts, jitter, fuzz):
    starts, lens, rows, strays = layouts[jitter]
    ref = S.reduce_rows(rows, lens, fuzz=fuzz)
    assert rows.shape[0] > 40000 and all(ref["counts"][S.NAMES[k]] > 0 for k in range(6)), ref["counts"]       # every class 0 - 5 occurs
    kept = S.row_pairs(ref["kept"])
    assert strays <= set(kept) and len(strays) > 500                                      # the stray dovetails have no witness
    if jitter == 0 and fuzz == 0:                         # without the reference: the edges of an exact layout are the neighbouring live reads
        assert set(kept) - strays == S.neighbour_pairs(starts, lens, ref["contained"], MIN_OV) and len(kept) == len(set(kept))
    _all_degrees(H, ctx, rows, lens, ref, fuzz, what="jitter %d fuzz %d" % (jitter, fuzz))


# ---- 3. an all-bins style list: doubled rows --------------------------------------------------------------------------------------------------
def test_doubled_rows(H, ctx, layouts):
    starts, lens, rows, strays = layouts[3]
    single = S.reduce_rows(rows, lens, fuzz=10)
    dove = np.flatnonzero(np.isin(single["row_class"], (S.KEPT, S.REDUCED, S.DROPPED_READ)))[::10]
    extra = rows[dove].copy()
    extra[0::2, 1] += np.uint64(3)                        # the copy wins ...
    extra[1::2, 1] -= np.uint64(1)                        # ... or loses; every third copy has the original's score: the lower index stays
    extra[2::3, 1] = rows[dove][2::3, 1]
    doubled = np.insert(rows, dove + 1, extra, axis=0)
    origin = np.insert(np.arange(rows.shape[0]), dove + 1, -1 - np.arange(dove.size))     # where a row of the doubled list came from (copies: -1 - t)
    ref = S.reduce_rows(doubled, lens, fuzz=10)
    live = single["row_class"][dove] != S.DROPPED_READ
    assert ref["counts"]["duplicate"] == int(live.sum()) > 300
    # the survivors have the classes of the undoubled list
    surv = ref["row_class"] != S.DUPLICATE
    src = np.where(origin >= 0, origin, dove[np.clip(-1 - origin, 0, dove.size - 1)])
    assert np.array_equal(ref["row_class"][surv], single["row_class"][src[surv]]) and ref["arcs"] == single["arcs"]
    _all_degrees(H, ctx, doubled, lens, ref, 10, what="doubled")


# ---- 4. degree edges: a staggered pile ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1])
def test_staggered_pile(H, ctx, d):
    """Read j starts at base j, all reads have one length and share at least 20 bases: none is contained, every pair is a dovetail and
    vertex 0 has d out-arcs.  In closed form: a row is KEPT iff its reads are neighbours, every other row is REDUCED.  The run without the
    wave path is limited to d <= 65: its walk of deg^2 searches per vertex is the reason the wave path exists.  This pins the mechanics of
    the chunks (63 to 1025 records, one chunk and two), not the length rule: every arc that is not between neighbours has hundreds of
    witnesses far below L, fuzz is 0 and no record is dead, so a wave path with a wrong comparison or a wrong range of out(w) gives the
    same classes here.  The hubs of tests/test_gpu_overlaps_reduce_hubs.py are what pins those."""
    n = d + 1
    rng = np.random.default_rng(d)
    lens = np.full(n, d + 50)
    rows = S.layout_rows(np.arange(n), lens, rng.integers(0, 2, n), 20)
    assert rows.shape[0] == n * (n - 1) // 2
    pairs = np.array(S.row_pairs(rows))
    cls = np.where(pairs[:, 1] - pairs[:, 0] == 1, S.KEPT, S.REDUCED).astype(np.uint8)
    counts = dict({k: 0 for k in S.NAMES}, kept=n - 1, reduced=rows.shape[0] - (n - 1))
    for wd in ((0, 1, 64, NONE) if d <= 65 else (0, 1)):
        for on_device in (False, True):
            with H.Overlaps.from_rows(rows).reduce(ctx, lens, fuzz=0, wave_degree=wd, on_device=on_device) as g:
                got, contained = g.host_copy()
                kept = g.edges.rows() if not on_device else ctx.d2h(g.edges.rows_dev, len(g) * 48).view(np.uint64).reshape(-1, 6)
                print("d %d wave_degree %d: %.3f ms, reduce %.3f ms, wave vertices %d" % (d, wd, g.info["ms_total"], g.info["ms_reduce"], g.info["wave_vertices"]))
                assert np.array_equal(got, cls) and np.array_equal(kept, rows[cls == S.KEPT]) and not contained.any() and contained.size == n
                thr = g.info["wave_degree"]
                want = dict(counts, input_rows=rows.shape[0], contained_reads=0, arcs=2 * rows.shape[0], max_degree=d, wave_vertices=0 if wd == NONE else 2 * max(n - max(thr, 1), 0))
                assert {k: g.info[k] for k in COUNTS} == want


# ---- 5. end to end: count -> strands -> pair_diagonals -> extend_gapped -> reduce, the rows never on the host -------------------------------------
@pytest.fixture(scope="module")
def chain(H):
    """the noisy 1500 reads of tests/test_gpu_extend_gapped.py: (context, dna, par, the diagonal rows in HBM)"""
    from tests import extend_ref as X
    from tests import gapped_ref as G
    from tests.test_gpu_strands import _seqs
    from tests.test_gpu_extend import _pipeline
    seqs, par = _seqs("clean")
    rng = np.random.default_rng(131)
    noisy = []
    for s in seqs:
        f, _ = G.mutate(np.array(X.codes(s)), np.zeros(len(s), bool), rng, 0.01, 0.005)
        noisy.append("".join("ACGT"[x] for x in f))
    c, dna, pd, pd_dev = _pipeline(H, noisy, par)
    yield c, dna, par, pd_dev
    pd_dev.close()
    c.close()


def test_end_to_end(H, chain):
    c, dna, par, pd_dev = chain
    base = par["rid_base"]
    lens = dna.arrays()[2]
    with pd_dev.extend_gapped(c, dna, rid_base=base, on_device=True) as ov:
        assert ov.rows_dev and len(ov) > 5000 and ov.rows().shape == (0, 6)
        host = c.d2h(ov.rows_dev, len(ov) * 48).view(np.uint64).reshape(len(ov), 6)      # for the reference only
        ref = S.reduce_rows(host, lens, rid_base=base, fuzz=10)
        with ov.reduce(c, dna, rid_base=base, on_device=True) as g:
            _check(H, c, g, host, ref, "end to end, everything in HBM")
            assert g.info["kept"] > 0 and g.info["reduced"] > 0 and len(g.edges) == g.info["kept"] and g.edges.rows_dev
        for wd in (1, NONE):
            for reads in (dna, dna.arrays(), lens):      # a DnaBuffer, a tuple, bare lengths
                _check(H, c, ov.reduce(c, reads, rid_base=base, wave_degree=wd), host, ref, "end to end wave_degree %d" % wd)
        g = H.Overlaps.from_rows(host).reduce(c, lens, rid_base=base)
        v, w, ln, row = g.arcs(lens)
        assert sorted(zip(v.tolist(), w.tolist(), ln.tolist(), row.tolist())) == ref["kept_arcs"] and v.size == 2 * g.info["kept"]
        # fewer edges are explained away when the sums may not exceed the long arc at all
        assert H.Overlaps.from_rows(host).reduce(c, lens, rid_base=base, fuzz=0).info["kept"] >= g.info["kept"]


def test_lengths_on_the_device(H, chain):
    """a DeviceDna gives its lengths where they lie"""
    c, dna, par, pd_dev = chain
    dp, nb, do, dl = c.synth_reads(20000, 150, 40, 29)
    ddna = H.DeviceDna(c, dp, nb, do, dl, 40, 3)
    rows = S.layout_rows(np.arange(40) * 30, np.full(40, 150), np.zeros(40, np.int64), 20, rid_base=3)
    ref = S.reduce_rows(rows, np.full(40, 150), rid_base=3, fuzz=0)
    _check(H, c, H.Overlaps.from_rows(rows).reduce(c, ddna, fuzz=0), rows, ref, "lengths in HBM")
    assert ref["counts"]["kept"] == 39 and ref["counts"]["reduced"] > 0
    ddna.free()


# ---- 6. refusals and edges -----------------------------------------------------------------------------------------------------------------------
def test_refusals_and_edges(H, ctx, layouts):
    from hysortk_amd import _lib
    c = ctx
    starts, lens, rows, strays = layouts[0]
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    rows = np.ascontiguousarray(rows[:5000])
    n = rows.shape[0]
    ref = S.reduce_rows(rows, lens, fuzz=10)
    ov = H.Overlaps.from_rows(rows)
    t = _to_device(rows)
    ov_dev = _device_list(H, rows, t)

    def works():
        _check(H, c, ov_dev.reduce(c, lens), rows, ref, "works")

    def refused(text, fn, *a, **kw):
        with pytest.raises(H.HskError) as e:
            fn(*a, **kw)
        msg = str(e.value)                                # the case, the call, and how many rows (a NULL list has none to name)
        assert e.value.status == 1 and text in msg and "hsk_overlaps_reduce" in msg and (str(n) in msg or text == "NULL"), msg
        print(str(e.value))
        works()

    works()
    top = int(((rows[:, 0] >> np.uint64(32)) & np.uint64(0x7FFFFFFF)).max())
    refused("outside [", ov.reduce, c, lens[:top])                                        # the last read a row names has no length
    refused("outside [", ov_dev.reduce, c, lens, rid_base=1)
    other = lens.copy()
    other[::2] += 1
    refused("not the lengths", ov.reduce, c, other)                                       # lengths of other reads
    refused("not the lengths of the reads the rows were computed from", ov_dev.reduce, c, other)
    one = rows.copy()
    one[17, 4] ^= np.uint64(1)                                                            # one ends bit that the coordinates do not give
    refused("of 1 of %d rows" % n, H.Overlaps.from_rows(one).reduce, c, lens)
    one = rows.copy()
    one[17, 2] = (one[17, 2] & np.uint64(0xFFFFFFFF)) << np.uint64(32) | (one[17, 2] & np.uint64(0xFFFFFFFF))      # a_lo == a_hi
    refused("of 1 of %d rows" % n, H.Overlaps.from_rows(one).reduce, c, lens)
    refused("2^31", ov.reduce, c, lens, rid_base=2_147_483_000)
    refused("2^31", ov.reduce, c, lens, rid_base=-1)

    vp = C.c_void_p
    opts = _lib.ReduceOpts(fuzz=10, wave_degree=0)

    def raw(pov, plens=lens.ctypes.data_as(vp), popts=C.byref(opts), out=None):
        rd = _lib.Reduced()
        c._check(c.lib.hsk_overlaps_reduce(c.h, pov, plens, lens.size, 0, 0, popts, 0, C.byref(rd) if out is None else out))
        g = H.OverlapGraph._wrap(c, rd, False, 0)
        return g

    good = _lib.Overlaps(n=n, rows=rows.ctypes.data_as(C.POINTER(C.c_uint64)))
    _check(H, c, raw(C.byref(good)), rows, ref, "a struct filled in by hand, priv NULL")
    refused("NULL", raw, C.byref(good), plens=None)
    refused("NULL", raw, None)
    refused("NULL", raw, C.byref(good), popts=None)
    refused("neither rows nor rows_dev", raw, C.byref(_lib.Overlaps(n=n)))
    refused("16-byte aligned", raw, C.byref(_lib.Overlaps(n=n, rows_dev=t.data_ptr() + 8)))
    with pytest.raises(H.HskError) as e:                                                  # (the text names its own number of rows)
        raw(C.byref(_lib.Overlaps(n=1 << 32, rows_dev=t.data_ptr())))
    assert e.value.status == 1 and "%d rows are 2^32 or more" % (1 << 32) in str(e.value), str(e.value)
    works()
    assert c.lib.hsk_overlaps_reduce(c.h, C.byref(good), lens.ctypes.data_as(vp), lens.size, 0, 0, C.byref(opts), 0, None) == 1
    works()

    # an empty list is an empty graph
    for on_device in (False, True):
        with H.Overlaps.from_rows(np.zeros((0, 6), np.uint64)).reduce(c, lens, on_device=on_device) as g:
            cls, contained = g.host_copy()
            assert len(g) == 0 and cls.size == 0 and contained.size == lens.size and not contained.any()
            assert all(g.info[k] == 0 for k in COUNTS) and g.info["ms_sort"] == 0
    g = raw(C.byref(_lib.Overlaps(n=0)))
    assert len(g) == 0 and g.edges.rows().shape == (0, 6)
    # every read is contained: no arcs, so nothing is sorted and nothing reduced
    l3 = np.array([100, 100, 100], dtype=np.uint32)
    allc = np.array([S.make_row(0, 1, 0, 0, 100, 0, 100, 100, 100), S.make_row(1, 2, 1, 0, 100, 0, 100, 100, 100), S.make_row(2, 0, 0, 0, 100, 0, 100, 100, 100),
                     S.make_row(0, 1, 0, 10, 100, 0, 90, 100, 100), S.make_row(1, 1, 0, 10, 100, 0, 90, 100, 100)], dtype=np.uint64)
    refc = S.reduce_rows(allc, l3)
    assert refc["row_class"].tolist() == [S.A_CONTAINED] * 3 + [S.DROPPED_READ, S.SELF] and refc["contained"].all()
    for wd in DEGREES:
        g = H.Overlaps.from_rows(allc).reduce(c, l3, wave_degree=wd)
        _check(H, c, g, allc, refc, "every read contained")
        assert g.info["arcs"] == 0 and g.info["ms_sort"] == 0 and len(g) == 0
    t.close()
    assert c.lib.hsk_abi_version() == 4
