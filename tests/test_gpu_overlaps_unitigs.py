"""hsk_overlaps_unitigs (include/hsk.h): the maximal non-branching paths of a list of string graph edges in HBM, every member read's
orientation and position -- against the definition in plain Python (tests/unitig_ref.py, itself held to layouts typed out by hand by
tests/test_unitig_ref.py).  The edges are fabricated from layouts of reads on a line and around a circle and reduced by the reference
(tests/strgraph_ref.py).  Everything is integer work and compared for equality: the layout rows, the unitig rows and every count.  Every case
runs with the result on the host and left in HBM, and with the rows (and the contained bits) given from the host and from HBM."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from tests import strgraph_ref as S
from tests import unitig_ref as U
from tests.test_gpu_overlaps_reduce import _device_list, _stray_rows, _to_device
from tests.test_unitig_ref import hand_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    import hysortk_amd
    return hysortk_amd


@pytest.fixture(scope="module")
def ctx(H):
    with H.Context(K=31) as c:
        yield c


def _same(ut, ref, what):
    """one result against the reference: layout rows, unitig rows, every count; and the views of a host result against its rows"""
    lay, tab = ut.host_copy()
    i = ut.info
    print("%s: %d rows, %s, rounds %d, %.3f ms (arcs %.3f, sort %.3f, rank %.3f, emit %.3f, d2h %.3f)" % (
        what, i["input_rows"], " ".join("%s %d" % (k, i[k]) for k in U.COUNTS), i["rounds"], i["ms_total"], i["ms_arcs"], i["ms_sort"], i["ms_rank"], i["ms_emit"], i["ms_d2h"]))
    assert lay.shape == ref["layout"].shape and tab.shape == ref["table"].shape, what
    bad = np.flatnonzero((lay != ref["layout"]).any(axis=1))
    assert bad.size == 0, "%s: layout row %d is %s, the reference says %s" % (what, bad[0], lay[bad[0]], ref["layout"][bad[0]])
    assert np.array_equal(tab, ref["table"]), what
    assert {k: i[k] for k in U.COUNTS} == ref["info"], what
    assert len(ut) == ref["info"]["unitigs"]
    if ut.rows_dev is None and ut.table_dev is None:
        lo = np.uint64(0xFFFFFFFF)
        assert np.array_equal(ut.rows(), lay) and np.array_equal(ut.table(), tab)
        assert np.array_equal(ut.unitig.astype(np.uint64) << np.uint64(32) | ut.rank.astype(np.uint64), lay[:, 0]) and np.array_equal(ut.rid.astype(np.uint64) << np.uint64(1) | ut.reverse, lay[:, 1])
        assert np.array_equal(ut.offset, lay[:, 2]) and np.array_equal(ut.link_len.astype(np.uint64) << np.uint64(32) | ut.link_row.astype(np.uint64), lay[:, 3])
        assert np.array_equal(ut.first, tab[:, 0]) and np.array_equal(ut.reads, tab[:, 1]) and np.array_equal(ut.bases, tab[:, 2]) and np.array_equal(ut.circular, tab[:, 3] != 0)
        if len(ut):
            u = len(ut) - 1
            rid, rev, off = ut.members(u)
            assert np.array_equal(rid, (lay[int(tab[u, 0]):, 1] >> np.uint64(1)).astype(np.uint32)) and rid.size == tab[u, 1] and off[0] == 0 and rev.dtype == bool
            assert (ut.link_row[ut.link_len == ut.NO_LINK] == ut.NO_LINK).all() and (lay[:, 3] & lo)[ut.link_len != ut.NO_LINK].max(initial=0) < max(i["input_rows"], 1)
    else:
        assert ut.rows().shape == (0, 4) and (ut.rows_dev or not i["members"]) and (ut.table_dev or not i["unitigs"])


def _bits_to_device(H, contained):
    """the packed contained bits in HBM (as whole 64-bit words: what the helper of the reduce test uploads)"""
    w = np.ascontiguousarray(H.OverlapGraph.pack_contained(contained))
    return _to_device(np.concatenate([w, np.zeros(w.size % 2 + 2, np.uint32)]).view(np.uint64))


def _all_ways(H, c, rows, lens, contained, ref, rid_base=0, what=""):
    """host rows and bits, rows and bits in HBM; each with the result on the host and left in HBM.  Returns the info of the last run."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 6)
    lens = np.asarray(lens, dtype=np.uint32)
    contained = np.zeros(lens.size, bool) if contained is None else np.asarray(contained, dtype=bool)
    t, tb = _to_device(rows), _bits_to_device(H, contained)
    host = H.OverlapGraph(H.Overlaps.from_rows(rows), None, contained, {}, rid_base, lens.size)
    dev = H.OverlapGraph(_device_list(H, rows, t), None, None, {}, rid_base, lens.size, contained_dev=tb.data_ptr())
    info = None
    for g, where in ((host, "host rows"), (dev, "rows in HBM")):
        for on_device in (False, True):
            with g.unitigs(c, lens, on_device=on_device) as ut:
                _same(ut, ref, "%s, %s, on_device %d" % (what, where, on_device))
                info = ut.info
    t.close()
    tb.close()
    return info


def _moved(rows, base):
    out = np.array(rows, dtype=np.uint64).reshape(-1, 6).copy()
    out[:, 0] += np.uint64(base << 32 | base)
    return out


# ---- 1. the cases by hand ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", hand_cases(), ids=lambda k: k[0])
def test_hand_cases(H, ctx, case):
    name, rows, lens, contained, layout, table, counts = case
    ref = U.unitigs(rows, lens, contained)
    assert ref["layout"].tolist() == layout and ref["table"].tolist() == table and ref["info"] == counts
    _all_ways(H, ctx, rows, lens, contained, ref, what=name)
    ref7 = U.unitigs(_moved(rows, 7), lens, contained, rid_base=7)                       # the same reads numbered from 7
    assert np.array_equal(ref7["layout"][:, 1], ref["layout"][:, 1] + np.uint64(14)) and np.array_equal(ref7["table"], ref["table"])
    _all_ways(H, ctx, _moved(rows, 7), lens, contained, ref7, rid_base=7, what=name + " (rid_base 7)")


# ---- 2. lines ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 64, 65, 1025, 5000])
def test_lines(H, ctx, n):
    rng = np.random.default_rng(n)
    lens = np.full(n, 100)
    red = S.reduce_rows(S.layout_rows(np.arange(n) * 40, lens, rng.integers(0, 2, n), 20), lens, fuzz=0)
    ref = U.unitigs(red["kept"], lens, red["contained"])
    assert ref["info"]["unitigs"] == 1 and ref["table"].tolist() == [[0, n, 40 * (n - 1) + 100, 0]] and not red["contained"].any() and red["kept"].shape[0] == n - 1
    info = _all_ways(H, ctx, red["kept"], lens, None, ref, what="line of %d" % n)
    # two doubling phases of at most ceil(log2 nv) rounds, and slack for the cut: a condition, not a measurement -- a walk link by link would
    # need thousands of rounds
    if n == 5000:
        assert info["rounds"] <= 2 * math.ceil(math.log2(2 * n)) + 4, info["rounds"]


# ---- 3. rings: at the powers of two a doubled pointer returns to its own vertex -------------------------------------------------------------------
@pytest.mark.parametrize("step", [40, 60])
@pytest.mark.parametrize("n", [2, 3, 4, 64, 65, 1000, 1024])
def test_rings(H, ctx, n, step):
    rng = np.random.default_rng(100 * n + step)
    lens = np.full(n, 100)
    rows = U.ring_rows(n, rng.integers(0, 2, n), 100, step)
    ref = U.unitigs(rows, lens)
    assert ref["table"].tolist() == [[0, n, n * step, 1]] and ref["info"]["circular"] == 1 and ref["info"]["links"] == 2 * n
    assert int(ref["layout"][0, 1]) == 0 and int(ref["layout"][-1, 3]) != U.NO_LINK       # starts at read 0, forward; the last member links back
    _all_ways(H, ctx, rows, lens, None, ref, what="ring of %d, step %d" % (n, step))


# ---- 4. random layouts ---------------------------------------------------------------------------------------------------------------------------
SEED, NREADS, GENOME, MIN_OV, STRAYS = 23, 3000, 40000, 30, 12


@functools.lru_cache(maxsize=None)
def _layout_case(kind, jitter, fuzz):
    """(lens, the rows, the reference's reduction): "plain" -- the 3000 reads, "stray" -- with 12 stray dovetails, "thin" -- 600 reads of the same
    genome, with coverage gaps"""
    rng = np.random.default_rng(SEED)
    starts, lens, strands = S.random_layout(rng, 600 if kind == "thin" else NREADS, GENOME, 100, 400)
    rows = S.layout_rows(starts, lens, strands, MIN_OV, jitter=jitter, rng=rng)
    if kind == "stray":
        live = np.flatnonzero(~S.reduce_rows(rows, lens, fuzz=fuzz)["contained"])
        rows = np.concatenate([rows, _stray_rows(rng, lens, live, set(), starts, STRAYS, False)])
    return lens, rows, S.reduce_rows(rows, lens, fuzz=fuzz)


@pytest.mark.parametrize("jitter,fuzz", [(0, 0), (3, 10)])
@pytest.mark.parametrize("kind", ["plain", "stray", "thin"])
def test_random_layouts(H, ctx, kind, jitter, fuzz):
    lens, rows, red = _layout_case(kind, jitter, fuzz)
    ref = U.unitigs(red["kept"], lens, red["contained"])
    i = ref["info"]
    print(kind, jitter, fuzz, i)
    assert i["members"] == i["live_reads"] == int((~red["contained"]).sum()) and i["circular"] == 0
    if (jitter, fuzz) == (0, 0):                          # what the case is there for
        if kind == "plain":
            assert i["unitigs"] == 1 and i["longest"] == i["members"] > 64 and i["branch_vertices"] == 0
        if kind == "stray":
            assert i["branch_vertices"] > 0 and i["longest"] > 64 and i["unitigs"] > STRAYS
        if kind == "thin":
            assert i["singletons"] > 0 and i["unitigs"] > i["singletons"] and i["longest"] > 1 and i["branch_vertices"] == 0
    _all_ways(H, ctx, red["kept"], lens, red["contained"], ref, what="%s, jitter %d fuzz %d" % (kind, jitter, fuzz))
    # and on the graph the library reduced itself, everything resident
    with H.Overlaps.from_rows(rows).reduce(ctx, lens, fuzz=fuzz, on_device=True) as g:
        with g.unitigs(ctx, lens, on_device=True) as ut:
            _same(ut, ref, "%s, jitter %d fuzz %d, the resident graph" % (kind, jitter, fuzz))
        _same(g.unitigs(ctx, lens), ref, "%s, jitter %d fuzz %d, the resident graph, result on the host" % (kind, jitter, fuzz))


# ---- 5. end to end: count -> strands -> pair_diagonals -> extend_gapped -> reduce -> unitigs, the rows never on the host -----------------------------
@pytest.fixture(scope="module")
def chain(H):
    """the noisy 1500 reads of tests/test_gpu_overlaps_reduce.py: (context, dna, par, the diagonal rows in HBM)"""
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
        with ov.reduce(c, dna, rid_base=base, on_device=True) as g:
            assert g.edges.rows_dev and g.contained_dev and len(g) > 0
            with g.unitigs(c, dna, on_device=True) as ut:
                assert ut.rows_dev and ut.table_dev and ut.rows().shape == (0, 4)
                kept = c.d2h(g.edges.rows_dev, len(g) * 48).view(np.uint64).reshape(len(g), 6)      # for the reference only
                contained = g.host_copy()[1]
                ref = U.unitigs(kept, lens, contained, rid_base=base)
                _same(ut, ref, "end to end, everything in HBM")
                lay, tab = ut.host_copy()
            for reads in (dna, dna.arrays(), lens):      # a DnaBuffer, a tuple, bare lengths
                _same(g.unitigs(c, reads), ref, "end to end, result on the host")
    # every live read exactly once
    rid = (lay[:, 1] >> np.uint64(1)).astype(np.int64) - base
    assert np.array_equal(np.sort(rid), np.flatnonzero(~contained)) and ut.info["members"] == int((~contained).sum()) and ut.info["unitigs"] > 1 and ut.info["longest"] > 1
    # every link is a row of the edges whose arc it is
    arcs = {}
    av, aw, al, ar = H.OverlapGraph(H.Overlaps.from_rows(kept), None, contained, {}, base, lens.size).arcs(lens)
    for v, w, ln, row in zip(av.tolist(), aw.tolist(), al.tolist(), ar.tolist()):
        arcs[(v, w, row)] = ln
    vert = ((lay[:, 1] >> np.uint64(1)).astype(np.int64) - base) * 2 + (lay[:, 1] & np.uint64(1)).astype(np.int64)
    linked = 0
    for first, reads, bases, circular in tab.tolist():
        for k in range(reads):
            link = int(lay[first + k, 3])
            if link == U.NO_LINK:
                assert k == reads - 1 and not circular
                continue
            nxt = first + (k + 1) % reads
            assert k + 1 < reads or circular
            assert arcs[(int(vert[first + k]), int(vert[nxt]), link & 0xFFFFFFFF)] == link >> 32 and link & 0xFFFFFFFF < kept.shape[0]
            linked += 1
    assert 2 * linked == ut.info["links"] > 0


# ---- 6. refusals and edges -----------------------------------------------------------------------------------------------------------------------
def test_refusals_and_edges(H, ctx):
    from hysortk_amd import _lib
    c = ctx
    lens, raw, red = _layout_case("plain", 0, 0)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    rows, contained = np.ascontiguousarray(red["kept"]), red["contained"]
    n = rows.shape[0]
    ref = U.unitigs(rows, lens, contained)
    t = _to_device(rows)

    def graph(r=rows, con=contained, dev=False, nreads=lens.size, base=0):
        return H.OverlapGraph(_device_list(H, r, t) if dev else H.Overlaps.from_rows(r), None, con, {}, base, nreads)

    def works():
        _same(graph(dev=True).unitigs(c, lens), ref, "works")

    def refused(text, fn, *a, rows_named=n, **kw):
        with pytest.raises(H.HskError) as e:
            fn(*a, **kw)
        msg = str(e.value)                                # the case, the call, and how many rows (a NULL list has none to name)
        assert e.value.status == 1 and text in msg and "hsk_overlaps_unitigs" in msg and (str(rows_named) in msg or text == "NULL"), msg
        print(msg)
        works()

    works()
    top = int(((rows[:, 0] >> np.uint64(32)) & np.uint64(0x7FFFFFFF)).max())
    refused("outside [", graph(nreads=top, con=contained[:top]).unitigs, c, lens[:top])   # the last read a row names has no length
    refused("outside [", graph(dev=True).unitigs, c, lens, rid_base=lens.size)          # every read a row names lies below the first id
    other = lens.copy()
    other[::2] += 1
    refused("not the lengths of the reads the rows were computed from", graph().unitigs, c, other)
    refused("not the lengths", graph(dev=True).unitigs, c, other)
    one = rows.copy()
    one[17, 4] ^= np.uint64(1)                                                            # one ends bit that the coordinates do not give
    refused("of 1 of %d rows" % n, graph(one).unitigs, c, lens)
    refused("2^31", graph().unitigs, c, lens, rid_base=2_147_483_000)
    refused("2^31", graph().unitigs, c, lens, rid_base=-1)
    # an unreduced list is no list of edges: the raw rows of the layout hold contained reads and internal matches
    own = [S.own_class(S.fields(r, lens)) for r in raw]
    no_dove = sum(1 for k in own if k != S.KEPT)
    assert 0 < no_dove < raw.shape[0]
    refused("%d of %d rows are no dovetails: this is not a list of string graph edges" % (no_dove, raw.shape[0]), graph(raw, None).unitigs, c, lens, rows_named=raw.shape[0])
    for bad in (S.make_row(5, 5, 0, 40, int(lens[5]), 0, int(lens[5]) - 40, int(lens[5]), int(lens[5])), S.make_row(0, 1, 0, 3, int(lens[0]) - 3, 4, int(lens[1]) - 4, int(lens[0]), int(lens[1]))):      # SELF, INTERNAL
        refused("1 of %d rows are no dovetails" % (n + 1), graph(np.concatenate([rows, np.array([bad], dtype=np.uint64)])).unitigs, c, lens, rows_named=n + 1)
    # the kept list with one contained bit flipped: a live read of an edge becomes contained
    flipped = contained.copy()
    flipped[int(rows[0, 0] & np.uint64(0xFFFFFFFF))] = True
    named = int(((((rows[:, 0] >> np.uint64(32)) & np.uint64(0x7FFFFFFF)) == (rows[0, 0] & np.uint64(0xFFFFFFFF))) | ((rows[:, 0] & np.uint64(0xFFFFFFFF)) == (rows[0, 0] & np.uint64(0xFFFFFFFF)))).sum())
    refused("%d of %d rows name a read whose contained bit is set" % (named, n), graph(con=flipped).unitigs, c, lens)
    tb = _bits_to_device(H, flipped)
    g = H.OverlapGraph(_device_list(H, rows, t), None, None, {}, 0, lens.size, contained_dev=tb.data_ptr())
    refused("rows name a read whose contained bit is set", g.unitigs, c, lens, on_device=True)
    tb.close()

    vp = C.c_void_p
    opts = _lib.UnitigOpts()
    bits = np.ascontiguousarray(H.OverlapGraph.pack_contained(contained))

    def rawcall(pov, pcon=bits.ctypes.data_as(vp), plens=lens.ctypes.data_as(vp), popts=C.byref(opts), con_dev=0, nreads=lens.size):
        ut = _lib.Unitigs()
        c._check(c.lib.hsk_overlaps_unitigs(c.h, pov, pcon, con_dev, plens, nreads, 0, 0, popts, 0, C.byref(ut)))
        return H.Unitigs._wrap(c, ut, False)

    good = _lib.Overlaps(n=n, rows=rows.ctypes.data_as(C.POINTER(C.c_uint64)))
    _same(rawcall(C.byref(good)), ref, "a struct filled in by hand, priv NULL")
    refused("NULL", rawcall, C.byref(good), plens=None)
    refused("NULL", rawcall, None)
    refused("NULL", rawcall, C.byref(good), popts=None)
    refused("neither rows nor rows_dev", rawcall, C.byref(_lib.Overlaps(n=n)))
    refused("16-byte aligned", rawcall, C.byref(_lib.Overlaps(n=n, rows_dev=t.data_ptr() + 8)))
    tb = _bits_to_device(H, contained)
    _same(rawcall(C.byref(good), pcon=tb.data_ptr(), con_dev=1), ref, "the bits in HBM, by hand")
    refused("not 4-byte aligned", rawcall, C.byref(good), pcon=tb.data_ptr() + 2, con_dev=1)
    tb.close()
    refused("2^31", rawcall, C.byref(good), nreads=(1 << 31) + 1)                         # more reads than ids (nothing of the lengths is read)
    with pytest.raises(H.HskError) as e:                                                  # (the text names its own number of rows)
        rawcall(C.byref(_lib.Overlaps(n=1 << 32, rows_dev=t.data_ptr())))
    assert e.value.status == 1 and "%d rows are 2^32 or more" % (1 << 32) in str(e.value), str(e.value)
    works()
    assert c.lib.hsk_overlaps_unitigs(c.h, C.byref(good), bits.ctypes.data_as(vp), 0, lens.ctypes.data_as(vp), lens.size, 0, 0, C.byref(opts), 0, None) == 1
    works()
    # contained NULL: no read is contained -- the contained reads of this layout become singletons
    every = U.unitigs(rows, lens, None)
    _same(rawcall(C.byref(good), pcon=None), every, "contained NULL")
    assert every["info"]["singletons"] == int(contained.sum()) > 0 and every["info"]["live_reads"] == lens.size

    # an empty list: every live read is a unitig of its own
    l5 = np.full(5, 100, np.uint32)
    c5 = np.array([False, True, False, False, True])
    ref5 = U.unitigs(np.zeros((0, 6), np.uint64), l5, c5)
    assert ref5["info"]["unitigs"] == ref5["info"]["singletons"] == 3 and ref5["layout"][:, 1].tolist() == [0, 4, 6] and ref5["table"][:, 2].tolist() == [100] * 3
    info = _all_ways(H, c, np.zeros((0, 6), np.uint64), l5, c5, ref5, what="an empty list")
    assert info["rounds"] == 0 and info["ms_sort"] == 0
    # every read contained: no unitigs
    none = U.unitigs(np.zeros((0, 6), np.uint64), l5, np.ones(5, bool))
    assert none["info"]["unitigs"] == 0 and none["layout"].shape == (0, 4)
    _all_ways(H, c, np.zeros((0, 6), np.uint64), l5, np.ones(5, bool), none, what="every read contained")
    # no reads at all
    _all_ways(H, c, np.zeros((0, 6), np.uint64), np.zeros(0, np.uint32), None, U.unitigs(np.zeros((0, 6), np.uint64), []), what="no reads")
    t.close()
    assert c.lib.hsk_abi_version() == 4
