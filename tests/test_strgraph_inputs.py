"""tests/strgraph_inputs.py against the plain-Python definition (tests/strgraph_ref.py), without a GPU: what the lists of
tests/test_gpu_overlaps_reduce_hubs.py are built to be, shown by the reference alone -- every designed row gets its designed class, the
hubs have the degrees and the runs across the chunk edges that the wave path is to meet, and the list tells a correct length rule from
one that is off by a base, and a live record from a dead one."""
import collections
import itertools

import numpy as np
import pytest

from tests import strgraph_inputs as I
from tests import strgraph_ref as S


# ---- arc_row: the arc table read backwards ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sv,sw,exchanged,rid_base", list(itertools.product((0, 1), (0, 1), (False, True), (0, 5))))
def test_arc_row(sv, sw, exchanged, rid_base):
    lens = [300, 170, 90]
    for p, q in ((0, 2), (2, 1), (1, 0)):
        for length, reach in ((1, None), (60, 1), (lens[p] - 1, lens[q] - 1), (17, 33)):
            v, w = 2 * p + sv, 2 * q + sw
            row = I.arc_row(v, w, length, lens, exchanged=exchanged, rid_base=rid_base, reach=reach)
            f = S.fields(row, lens, rid_base)                          # (raises unless coordinates, lengths and ends bits agree)
            assert (f["a"], f["b"]) == ((q, p) if exchanged else (p, q)) and S.own_class(f) == S.KEPT
            arcs = S.row_arcs(f)
            reach = min(lens[p] - length, lens[q] - 1) if reach is None else reach
            assert (v, w, length) in arcs and sorted(arcs) == sorted([(v, w, length), (w ^ 1, v ^ 1, lens[q] - reach)])
            assert row[1] == f["a_hi"] - f["a_lo"] and I.arc_row(v, w, length, lens, exchanged=exchanged, score=7, reach=reach)[1] == 7
    for bad in (dict(v=0, w=1, length=5), dict(v=0, w=2, length=0), dict(v=0, w=2, length=300), dict(v=0, w=2, length=5, reach=170), dict(v=0, w=2, length=5, reach=0)):
        with pytest.raises(ValueError):
            I.arc_row(lens=lens, **bad)


# ---- hub_graph -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hub():
    """the list, its plan and its reference, built once (the reference takes 2.9 s on this list of 45 172 rows: the two hubs alone are
    2085^2 + 1025^2 = 5.4e6 steps of its inner loop)"""
    rows, lens, plan = I.hub_graph(np.random.default_rng(I.HUB_SEED))
    return rows, lens, plan, S.reduce_rows(rows, lens, fuzz=plan["fuzz"])


def test_designed_classes(hub):
    """every designed row has its designed class, exactly: background and pool do not meet, and the complement arcs explain nothing"""
    rows, lens, plan, ref = hub
    got = ref["row_class"][plan["index"]]
    bad = np.flatnonzero(got != plan["cls"])
    assert bad.size == 0, [(int(plan["index"][b]), str(plan["kind"][b]), int(got[b]), int(plan["cls"][b])) for b in bad[:10]]
    assert plan["index"].size == np.unique(plan["index"]).size == rows.shape[0] - int(plan["index"].min())      # all rows behind the background are designed
    bg_reads = set(np.array(S.row_pairs(rows[:int(plan["index"].min())])).ravel().tolist())
    pool_reads = set(np.array(S.row_pairs(rows[plan["index"]])).ravel().tolist())
    assert not bg_reads & pool_reads and max(bg_reads) < min(pool_reads)


def test_hub_shape(hub):
    rows, lens, plan, ref = hub
    a, b = plan["hub_a"], plan["hub_b"]
    arcs = collections.defaultdict(list)                  # v -> the targets of its records, dead ones included: what the sorted arc array holds
    for i in np.flatnonzero(np.isin(ref["row_class"], (S.KEPT, S.REDUCED, S.DUPLICATE))):
        for v, w, ln in S.row_arcs(S.fields(rows[i], lens)):
            arcs[v].append(w)
    assert ref["degree"][a] == len(arcs[a]) == I.DEG_A == 2 * I.CHUNK + 37 and ref["degree"][b] == len(arcs[b]) == I.DEG_B == I.CHUNK + 1
    assert max(ref["degree"].values()) == I.DEG_A and sorted(ref["degree"].values())[-3] < 256            # no third vertex takes the wave path by default
    assert b == a + I.GRID and (b >> 1) - (a >> 1) == 8192                                              # one workgroup treats A, then B
    # the runs of equal keys lie across the chunk edges: records 1023 | 1024 and 2047 | 2048 of out(A), 1023 | 1024 of out(B)
    assert [(h, pos) for h, x, pos in plan["edges"]] == [(a, 1023), (a, 2047), (b, 1023)]
    for h, x, pos in plan["edges"]:
        run = sorted(arcs[h])
        assert run[pos] == run[pos + 1] == x and run.count(x) == 2 and (pos + 1) % I.CHUNK == 0
    # below rank 1100 of out(A) no target has a second record but the one at the first edge
    run = sorted(arcs[a])
    assert len(set(run[:1100])) == 1099
    dead_targets = {S.row_arcs(S.fields(rows[i], lens))[k][1] for i in plan["index"][plan["kind"] == "dup_target"] for k in (0, 1)} & set(run)
    assert len(dead_targets) == 40 and min(run.index(x) for x in dead_targets) > 1100
    # every designed kind often enough on both hubs, under every dovetail kind and both orders of a and b
    count = collections.Counter(zip(plan["kind"].tolist(), plan["on_a"].tolist()))
    assert all(count[(k, True)] >= 300 and count[(k, False)] >= 150 for k in ("none", "exact", "over", "witness")), count
    assert count[("dup_target", True)] == 40 and count[("dup_witness", True)] == 40 and count[("edge_long", True)] == 2 and count[("edge_dup", False)] == 1
    seen = collections.Counter()
    for i, kind in zip(plan["index"], plan["kind"]):
        f = S.fields(rows[i], lens)
        seen[(str(kind), f["o"], f["e"])] += 1
    assert all(seen[("witness", o, e)] >= 20 for o, e in S.DOVETAILS), seen
    mine = {(0, 6), (0, 9), (1, 5) if a & 1 else (1, 10)}                                   # the rows with an arc out of a vertex of the hubs' strand
    assert all(seen[(k, o, e)] >= 20 for k in ("none", "exact", "over") for o, e in mine), seen
    # the three score orders of a copy: the larger score behind, equal scores, the larger score in front
    order = collections.Counter((l["loser"] < l["winner"], int(rows[l["loser"], 1]) == int(rows[l["winner"], 1])) for l in plan["losers"])
    assert order[(True, False)] >= 20 and order[(False, True)] >= 20 and order[(False, False)] >= 20 and order[(True, True)] == 0
    # every class 0 - 6 occurs, 0 - 5 in the background too; more vertices carry arcs than the wave path has workgroups
    assert all(ref["counts"][S.NAMES[c]] > 0 for c in range(7)), ref["counts"]
    assert set(range(6)) <= set(ref["row_class"][:int(plan["index"].min())].tolist())
    assert len(ref["degree"]) > I.GRID and sum(1 for c in collections.Counter(v % I.GRID for v in ref["degree"]).values() if c >= 2) > 1000
    assert (a - I.GRID) in ref["degree"]                  # A's workgroup arrives from a vertex with arcs, with wave_degree 1


def test_lengths_discriminate(hub):
    """one base of fuzz less turns exactly the rows with an exact witness KEPT, one more exactly those with a witness one base too long
    REDUCED: a length rule that is off by one in either direction changes the designed rows' classes"""
    rows, lens, plan, ref = hub
    fuzz, want = plan["fuzz"], plan["cls"]
    exact = np.isin(plan["kind"], ("exact", "edge_long"))
    over = plan["kind"] == "over"
    assert np.array_equal(exact, want == S.REDUCED) and exact.sum() > 1000 and over.sum() > 1000
    less = S.reduce_rows(rows, lens, fuzz=fuzz - 1)["row_class"][plan["index"]]
    assert np.array_equal(less != want, exact) and (less[exact] == S.KEPT).all()
    more = S.reduce_rows(rows, lens, fuzz=fuzz + 1)["row_class"][plan["index"]]
    assert np.array_equal(more != want, over) and (more[over] == S.REDUCED).all()


def test_scores_decide(hub):
    """with the losers' scores above the winners' the designed rows change class: a dead record taken for a live one changes the result"""
    rows, lens, plan, ref = hub
    raised, want = I.raise_losers(rows, plan)
    got = S.reduce_rows(raised, lens, fuzz=plan["fuzz"])["row_class"][plan["index"]]
    assert np.array_equal(got, want)
    changed = np.flatnonzero(want != plan["cls"])
    kinds = collections.Counter(plan["kind"][changed].tolist())
    assert kinds == {"dup_target": 40, "none": 40, "dup_witness": 40, "witness": 40, "over": 40, "edge_dup": 1, "edge_short": 1}, kinds
    assert (want[plan["kind"] == "dup_target"] == S.REDUCED).all() and (want[plan["kind"] == "edge_dup"] == S.REDUCED).all()


# ---- the small lists -----------------------------------------------------------------------------------------------------------------------------
def test_huge_case():
    rows, lens, classes = I.huge_case()
    assert int(lens[0]) == 2 ** 32 - 1 and sorted(classes) == [10, 2 ** 32 - 1]
    for fuzz, want in classes.items():
        assert S.reduce_rows(rows, lens, fuzz=fuzz)["row_class"].tolist() == want
    arcs = sorted(S.reduce_rows(rows, lens, fuzz=10)["kept_arcs"])
    assert (0, 2, 3_000_000_000, 0) in arcs and (0, 4, 2_000_000_000, 2) in arcs and (7, 3, 2_000_000_000, 5) in arcs
    assert (3_000_000_000 + 3_000_000_000) % 2 ** 32 <= 2_000_000_000 + 10                 # 32-bit sums would explain the long arc ...
    assert (2_000_000_000 + 2 ** 32 - 1) % 2 ** 32 < 3_000_000_000 + 3_000_000_000 <= 2_000_000_000 + 2 ** 32 - 1      # ... or a 32-bit bound keep it


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2047, 2048, 2049])
def test_tile_rows(n):
    rows, lens = I.tile_rows(np.random.default_rng(n), n)
    cls = S.reduce_rows(rows, lens)["row_class"]
    assert rows.shape == (n, 6) and all(cls[e] <= S.REDUCED for e in (1022, 1023, 1024, 2047, 2048) if e < n)
    assert set(range(6)) - {S.INTERNAL} <= set(cls.tolist())
