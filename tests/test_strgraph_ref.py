"""tests/strgraph_ref.py (the definition of hsk_overlaps_reduce in plain Python) held to rows written by hand, to the property that the kept
edges of an exact layout are the neighbouring live reads, and OverlapGraph.arcs (numpy, no GPU) held to the reference's arcs.
(A witness on the read of v or of x needs an arc between the two orientations of one read; SELF rows give no arcs, so such a witness
cannot be built from rows -- the rule is exercised on the function itself in tests/strgraph_test.cpp, and here through a SELF row.)"""
import itertools

import numpy as np
import pytest

from tests import strgraph_ref as S

K, R, I, AC, BC, DR, DU, SE = range(8)


def hand_chain():
    """three reads of 100 bases at 0, 40 and 80 of a line, as stored: (0, 1) and (1, 2) share 60 bases, (0, 2) shares 20"""
    rows = [S.make_row(0, 1, 0, 40, 100, 0, 60, 100, 100), S.make_row(0, 2, 0, 80, 100, 0, 20, 100, 100), S.make_row(1, 2, 0, 40, 100, 0, 60, 100, 100)]
    return np.array(rows, dtype=np.uint64), [100, 100, 100]


def hand_cases():
    """(name, rows, lens, fuzz, classes, contained): every case by hand; the GPU test runs the same list"""
    cases = []
    rows, lens = hand_chain()
    cases.append(("chain", rows, lens, 0, [K, R, K], [False] * 3))
    # read 1 stored reversed: its coordinates flip, both of its rows are on opposite strands
    rev = [S.make_row(0, 1, 1, 40, 100, 40, 100, 100, 100), S.make_row(0, 2, 0, 80, 100, 0, 20, 100, 100), S.make_row(1, 2, 1, 0, 60, 0, 60, 100, 100)]
    cases.append(("chain, read 1 reversed", np.array(rev, dtype=np.uint64), lens, 0, [K, R, K], [False] * 3))
    # reads 0 and 1 cover each other (e == 15): a goes, b stays; read 0's dovetail goes with it
    both = [S.make_row(0, 1, 0, 0, 100, 0, 100, 100, 100), S.make_row(0, 2, 0, 50, 100, 0, 50, 100, 100), S.make_row(1, 2, 0, 50, 100, 0, 50, 100, 100)]
    cases.append(("e == 15", np.array(both, dtype=np.uint64), lens, 10, [AC, DR, K], [True, False, False]))
    # read 2 [30, 100) inside read 1 [20, 150) inside read 0 [0, 200); read 3 [150, 300) dovetails with read 0 only
    nest = [S.make_row(0, 1, 0, 20, 150, 0, 130, 200, 130), S.make_row(0, 2, 0, 30, 100, 0, 70, 200, 70), S.make_row(1, 2, 0, 10, 80, 0, 70, 130, 70), S.make_row(0, 3, 0, 150, 200, 0, 50, 200, 150)]
    cases.append(("contained in contained", np.array(nest, dtype=np.uint64), [200, 130, 70, 150], 10, [BC, BC, BC, K], [False, True, True, False]))
    # the fuzz edge: 40 + 45 = 85 against L + 10 with L = 75 (reduced) and L = 74 (kept)
    for L, c in ((75, R), (74, K)):
        edge = [S.make_row(0, 1, 0, 40, 100, 0, 60, 100, 100), S.make_row(0, 2, 0, L, 100, 0, 100 - L, 100, 100), S.make_row(1, 2, 0, 45, 100, 0, 55, 100, 100)]
        cases.append(("fuzz edge L = %d" % L, np.array(edge, dtype=np.uint64), lens, 10, [K, c, K], [False] * 3))
    # duplicates: equal scores keep the lower index, else the larger score stays; the chain's result is that of its survivors
    d = hand_chain()[0]
    dup = np.array([d[0], d[0], d[1], d[2], d[2]], dtype=np.uint64)
    dup[4, 1] += np.uint64(5)
    cases.append(("duplicates", dup, lens, 0, [K, DU, R, DU, K], [False] * 3))
    # a row of a read with itself is SELF and gives no arc, whatever its shape; an INTERNAL row gives none either
    selfrow = np.array([S.make_row(0, 0, 0, 40, 100, 0, 60, 100, 100), S.make_row(0, 1, 0, 40, 100, 0, 60, 100, 100), S.make_row(0, 2, 0, 80, 100, 0, 20, 100, 100),
                        S.make_row(1, 2, 0, 40, 90, 5, 55, 100, 100)], dtype=np.uint64)
    cases.append(("self and internal", selfrow, lens, 10, [SE, K, K, I], [False] * 3))
    # a and b exchanged: the same arc twice from two rows that are no duplicates; both are edges
    swap = np.array([S.make_row(0, 1, 0, 40, 100, 0, 60, 100, 100), S.make_row(1, 0, 0, 0, 60, 40, 100, 100, 100)], dtype=np.uint64)
    cases.append(("exchanged", swap, lens, 10, [K, K], [False] * 3))
    return cases


@pytest.mark.parametrize("case", hand_cases(), ids=lambda c: c[0])
def test_hand_rows(case):
    name, rows, lens, fuzz, classes, contained = case
    ref = S.reduce_rows(rows, lens, fuzz=fuzz)
    assert ref["row_class"].tolist() == classes and ref["contained"].tolist() == contained
    assert np.array_equal(ref["kept"], rows[np.array(classes) == K])
    assert sum(ref["counts"].values()) == len(classes)


def test_chain_arcs_by_hand():
    rows, lens = hand_chain()
    ref = S.reduce_rows(rows, lens, fuzz=0)
    # 0 -> 2 (40 bases of read 0 in front), 2 -> 4 (40), and their complements 3 -> 1 and 5 -> 3; the arcs 0 -> 4 and 5 -> 1 (80) are out
    assert ref["kept_arcs"] == [(0, 2, 40, 0), (2, 4, 40, 1), (3, 1, 40, 0), (5, 3, 40, 1)] and ref["arcs"] == 6
    assert ref["degree"] == {0: 2, 2: 1, 3: 1, 5: 2} and S.expected_info(ref, 3, 2)["wave_vertices"] == 2 and S.expected_info(ref, 3, 0xFFFFFFFF)["wave_vertices"] == 0


@pytest.mark.parametrize("strands", list(itertools.product((0, 1), repeat=3)))
def test_chain_on_every_strand_combination(strands):
    rows = S.layout_rows([0, 40, 80], [100, 100, 100], strands, 10)
    assert S.row_pairs(rows) == [(0, 1), (0, 2), (1, 2)]
    if strands == (0, 0, 0):
        assert np.array_equal(rows, hand_chain()[0])     # layout_rows against the rows by hand
    if strands == (0, 1, 0):
        assert np.array_equal(rows, hand_cases()[1][1])
    assert [int(r[0]) >> 63 for r in rows] == [strands[0] ^ strands[1], strands[0] ^ strands[2], strands[1] ^ strands[2]]
    ref = S.reduce_rows(rows, [100, 100, 100], fuzz=0)
    assert ref["row_class"].tolist() == [K, R, K], ref["row_class"]      # the long arc goes, the two short ones stay
    for v, w, ln, row in ref["kept_arcs"]:
        assert ln == 40
        assert (v ^ 1, w ^ 1) != (v, w) and (w ^ 1, v ^ 1, 40, row) in ref["kept_arcs"]      # every arc with its complement


def test_refusals_of_the_reference():
    rows, lens = hand_chain()
    with pytest.raises(ValueError, match="not the lengths"):
        S.reduce_rows(rows, [100, 101, 100])
    with pytest.raises(ValueError, match="outside"):
        S.reduce_rows(rows, [100, 100])
    bad = rows.copy()
    bad[0, 4] = 2
    with pytest.raises(ValueError, match="not the lengths"):
        S.reduce_rows(bad, lens)


@pytest.mark.parametrize("seed", range(20))
def test_kept_edges_are_the_neighbouring_live_reads(seed):
    rng = np.random.default_rng(1000 + seed)
    starts, lens, strands = S.random_layout(rng, 120, 3000, 80, 200)
    rows = S.layout_rows(starts, lens, strands, 20)
    ref = S.reduce_rows(rows, lens, fuzz=0)
    kept = set(S.row_pairs(ref["kept"]))
    assert len(kept) == ref["kept"].shape[0] and kept == S.neighbour_pairs(starts, lens, ref["contained"], 20)
    assert ref["counts"]["reduced"] > 0 and ref["contained"].any()


def test_overlap_graph_arcs_against_the_reference():
    import hysortk_amd as H
    rng = np.random.default_rng(7)
    starts, lens, strands = S.random_layout(rng, 200, 4000, 80, 200)
    rows = S.layout_rows(starts, lens, strands, 20, jitter=3, rng=rng, rid_base=50)
    ref = S.reduce_rows(rows, lens, rid_base=50, fuzz=10)
    assert len({(int(r[0]) >> 63, int(r[4]) & 15) for r in ref["kept"]}) == 4          # every kind of dovetail among the edges
    g = H.OverlapGraph(H.Overlaps.from_rows(ref["kept"]), ref["row_class"], ref["contained"], {}, rid_base=50, nreads=len(lens))
    v, w, ln, row = g.arcs(lens)
    assert sorted(zip(v.tolist(), w.tolist(), ln.tolist(), row.tolist())) == ref["kept_arcs"] and len(g) == ref["kept"].shape[0]
    with pytest.raises(ValueError, match="no dovetail"):
        H.OverlapGraph(H.Overlaps.from_rows(rows), None, None, {}, rid_base=50).arcs(lens)
    assert (H.OverlapGraph.KEPT, H.OverlapGraph.REDUCED, H.OverlapGraph.INTERNAL, H.OverlapGraph.A_CONTAINED, H.OverlapGraph.B_CONTAINED, H.OverlapGraph.DROPPED_READ,
            H.OverlapGraph.DUPLICATE, H.OverlapGraph.SELF) == tuple(range(8)) and H.OverlapGraph.CLASS_NAMES == S.NAMES
