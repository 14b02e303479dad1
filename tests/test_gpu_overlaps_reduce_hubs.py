"""hsk_overlaps_reduce where only the GPU can check it: reduce_wave_kernel (hysortk_amd/csrc/hsk_reduce.h) shares no code with the lane path or
with the header that runs on the CPU -- its chunks of out(v) in LDS, its prune by the chunk's longest arc, its narrowing of out(w) to the
chunk's targets, its search, its length rule, its skip of dead records and its 64-bit sums are its own.  The lists come from
tests/strgraph_inputs.py, arc by arc, and tests/test_strgraph_inputs.py shows on the CPU that they tell a right kernel from a wrong one:
two hubs of three and two chunks whose every target has a witness at exactly L + fuzz, one base above it or none, dead records that would
be witnesses or would be explained, runs of equal keys across the chunk edges, and more vertices than the kernel has workgroups, so that
a workgroup meets the LDS its last vertex left.  Further: lengths whose sums need 33 bits on both paths, lists that end at the edges of the
1024-row tiles, and read ids up to 2^31 - 1.  Everything is compared for equality with tests/strgraph_ref.py: classes, kept rows,
contained bits and every count."""
import numpy as np
import pytest

from tests import strgraph_inputs as I
from tests import strgraph_ref as S
from tests.test_gpu_overlaps_reduce import DEGREES, NONE, H, _all_degrees, _check, _moved, ctx  # noqa: F401  (H, ctx: the fixtures)

pytestmark = pytest.mark.gpu


# ---- 1. two hubs of more than one chunk ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hub():
    """the list of tests/test_strgraph_inputs.py and its reference (2.9 s), once"""
    rows, lens, plan = I.hub_graph(np.random.default_rng(I.HUB_SEED))
    return rows, lens, plan, S.reduce_rows(rows, lens, fuzz=plan["fuzz"])


@pytest.mark.parametrize("wd", [0, 1, I.DEG_B, I.DEG_B + 1, I.DEG_A + 1, NONE])
def test_hubs(H, ctx, hub, wd):
    """wave_degree 0: the default, both hubs by workgroups; 1: every vertex, and the workgroups take a second and a third one; 1025: both
    hubs; 1026: A alone, B by lanes; 2086: the wave kernel finds no vertex; 0xFFFFFFFF: it is not launched"""
    rows, lens, plan, ref = hub
    assert np.array_equal(ref["row_class"][plan["index"]], plan["cls"])
    n = rows.shape[0]
    want = {0: 2, 1: len(ref["degree"]), I.DEG_B: 2, I.DEG_B + 1: 1, I.DEG_A + 1: 0, NONE: 0}[wd]
    assert S.expected_info(ref, n, wd or 256)["wave_vertices"] == want and S.expected_info(ref, n, wd)["max_degree"] == I.DEG_A
    _all_degrees(H, ctx, rows, lens, ref, plan["fuzz"], degrees=(wd,), what="hubs")


def test_hubs_fuzz_0(H, ctx, hub):
    """the same rows with no slack at all: the rows with a witness at L + 10 are KEPT, and the prune by the chunk's longest arc has more to pass over"""
    rows, lens, plan, ref = hub
    ref0 = S.reduce_rows(rows, lens, fuzz=0)
    assert (ref0["row_class"][plan["index"]][plan["cls"] == S.REDUCED] == S.KEPT).all() and ref0["counts"]["reduced"] > 0
    _all_degrees(H, ctx, rows, lens, ref0, 0, degrees=(0, 1), what="hubs, fuzz 0")


def test_hubs_top_read_ids(H, ctx, hub):
    """rid_base + nreads == 2^31: the last read has the largest id there is; one more is refused, and the context works afterwards"""
    rows, lens, plan, ref = hub
    base = 2 ** 31 - lens.size
    moved = _moved(rows, base)
    assert int(((moved[:, 0] >> np.uint64(32)) & np.uint64(0x7FFFFFFF)).max()) <= 2 ** 31 - 1 == int((moved[:, 0] & np.uint64(0xFFFFFFFF)).max())
    ref_top = S.reduce_rows(moved, lens, rid_base=base, fuzz=plan["fuzz"])
    assert np.array_equal(ref_top["row_class"], ref["row_class"])
    _all_degrees(H, ctx, moved, lens, ref_top, plan["fuzz"], rid_base=base, degrees=(0, 1), what="hubs, rid_base 2^31 - %d" % lens.size)
    with pytest.raises(H.HskError) as e:
        H.Overlaps.from_rows(moved).reduce(ctx, np.asarray(lens, dtype=np.uint32), rid_base=base + 1, fuzz=plan["fuzz"])
    assert e.value.status == 1 and "2^31" in str(e.value) and "hsk_overlaps_reduce" in str(e.value), str(e.value)
    _all_degrees(H, ctx, moved, lens, ref_top, plan["fuzz"], rid_base=base, degrees=(0,), what="hubs, after the refusal")


# ---- 2. sums above 2^32 on both paths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuzz", [10, 0xFFFFFFFF])
def test_sums_above_32_bits(H, ctx, fuzz):
    """arcs of 3e9 + 3e9 against one of 2e9 between reads of 2^32 - 1 bases: KEPT at fuzz 10 (a sum in 32 bits wraps to 1.7e9 and reduces
    it), REDUCED at fuzz 2^32 - 1 (L + fuzz in 32 bits wraps to 2e9 - 1 and keeps it); by workgroups and by lanes"""
    rows, lens, classes = I.huge_case()
    ref = S.reduce_rows(rows, lens, fuzz=fuzz)
    assert ref["row_class"].tolist() == classes[fuzz]
    _all_degrees(H, ctx, rows, lens, ref, fuzz, degrees=(1, NONE), what="huge, fuzz %d" % fuzz)
    g = H.Overlaps.from_rows(rows).reduce(ctx, np.asarray(lens, dtype=np.uint32), fuzz=fuzz, wave_degree=1)
    assert g.row_class.tolist() == classes[fuzz] and g.info["wave_vertices"] == len(ref["degree"]) == 7


# ---- 3. lists that end at the edges of the 1024-row tiles -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1023, 1024, 1025, 2047, 2048, 2049])
def test_tile_edges(H, ctx, n):
    """reduce_arcs_kernel and the compaction of the kept rows work on tiles of 1024 rows: lists of one row less, exactly and one row more
    than one and two tiles, with rows that give arcs on both sides of every edge; and the refusals count rows on both sides of an edge"""
    rows, lens = I.tile_rows(np.random.default_rng(n), n)
    lens = np.asarray(lens, dtype=np.uint32)
    ref = S.reduce_rows(rows, lens)
    edges = [e for e in (1022, 1023, 1024, 2047, 2048) if e < n]
    assert rows.shape[0] == n and all(ref["row_class"][e] <= S.REDUCED for e in edges), ref["row_class"][edges]
    _all_degrees(H, ctx, rows, lens, ref, S.DEFAULT_FUZZ, degrees=DEGREES, what="%d rows" % n)
    if n <= 1024:
        return

    def refused(text, bad):
        with pytest.raises(H.HskError) as e:
            H.Overlaps.from_rows(bad).reduce(ctx, lens)
        assert e.value.status == 1 and text in str(e.value) and "hsk_overlaps_reduce" in str(e.value), str(e.value)
        print(str(e.value))
        _check(H, ctx, H.Overlaps.from_rows(rows).reduce(ctx, lens), rows, ref, "%d rows, after the refusal" % n)

    bad = rows.copy()
    bad[1023:1025, 4] ^= np.uint64(1)                     # an ends bit that the coordinates do not give, in the last row of a tile and the first of the next
    refused("of 2 of %d rows do not agree" % n, bad)
    bad = rows.copy()
    bad[1024, 0] = (bad[1024, 0] & ~np.uint64(0xFFFFFFFF)) | np.uint64(lens.size)          # read b is the first one without a length
    refused("1 of %d rows name a read outside [0, %d)" % (n, lens.size), bad)
    if n > 2048:
        bad = rows.copy()
        bad[2047:2049, 4] ^= np.uint64(8)
        refused("of 2 of %d rows do not agree" % n, bad)
