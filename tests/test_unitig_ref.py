"""tests/unitig_ref.py (the definition of hsk_overlaps_unitigs in plain Python) held to cases whose layout rows and unitig rows are typed
out by hand, and to the closed form on exact layouts: after the reduction with fuzz 0 the unitigs of reads on a line are the maximal runs
of neighbouring live reads."""
import numpy as np
import pytest

from tests import strgraph_ref as S
from tests import unitig_ref as U

NO = U.NO_LINK
BIG = (1 << 32) - 1


def _l(u, rank, v, offset, link):
    """a layout row by hand: v = 2 rid + s; link = (len, row) or NO"""
    return [u << 32 | rank, v, offset, NO if link == NO else link[0] << 32 | link[1]]


def hand_cases():
    """(name, rows, lens, contained, layout, table, counts): every case by hand, read ids from 0; the GPU test runs the same list"""
    z = np.zeros((0, 6), np.uint64)
    r = lambda *rows: np.array(rows, dtype=np.uint64).reshape(-1, 6)
    c = lambda unitigs, members, singletons, circular, longest, links, branch, live, rows, arcs: dict(zip(U.COUNTS, (unitigs, members, singletons, circular, longest, links, branch, live, rows, arcs)))
    cases = [("single read", z, [100], None, [_l(0, 0, 0, 0, NO)], [[0, 1, 100, 0]], c(1, 1, 1, 0, 1, 0, 0, 1, 0, 0))]
    # two reads of 100 and 120 bases, the four kinds of dovetail: who is in front, and on which strand read 1 lies next to a forward read 0
    two = c(1, 2, 0, 0, 2, 2, 0, 2, 1, 2)
    cases.append(("o 0 e 6", r(S.make_row(0, 1, 0, 40, 100, 0, 60, 100, 120)), [100, 120], None, [_l(0, 0, 0, 0, (40, 0)), _l(0, 1, 2, 40, NO)], [[0, 2, 160, 0]], two))
    cases.append(("o 0 e 9", r(S.make_row(0, 1, 0, 0, 60, 60, 120, 100, 120)), [100, 120], None, [_l(0, 0, 2, 0, (60, 0)), _l(0, 1, 0, 60, NO)], [[0, 2, 160, 0]], two))
    cases.append(("o 1 e 10", r(S.make_row(0, 1, 1, 40, 100, 60, 120, 100, 120)), [100, 120], None, [_l(0, 0, 0, 0, (40, 0)), _l(0, 1, 3, 40, NO)], [[0, 2, 160, 0]], two))
    cases.append(("o 1 e 5", r(S.make_row(0, 1, 1, 0, 60, 0, 60, 100, 120)), [100, 120], None, [_l(0, 0, 3, 0, (60, 0)), _l(0, 1, 0, 60, NO)], [[0, 2, 160, 0]], two))
    # vertex 0 has the out-arcs 0 -> 2 and 0 -> 4: nothing is joined
    three = [_l(0, 0, 0, 0, NO), _l(1, 0, 2, 0, NO), _l(2, 0, 4, 0, NO)], [[0, 1, 100, 0], [1, 1, 100, 0], [2, 1, 100, 0]], c(3, 3, 3, 0, 1, 0, 1, 3, 2, 4)
    cases.append(("fork", r(S.make_row(0, 1, 0, 40, 100, 0, 60, 100, 100), S.make_row(0, 2, 0, 50, 100, 0, 50, 100, 100)), [100] * 3, None) + three)
    # 0 -> 4 and 2 -> 4: vertex 5 has two out-arcs
    cases.append(("join", r(S.make_row(0, 2, 0, 40, 100, 0, 60, 100, 100), S.make_row(1, 2, 0, 50, 100, 0, 50, 100, 100)), [100] * 3, None) + three)
    # a and b exchanged: the arc 0 -> 2 twice, of 40 bases from row 0 and of 38 from row 1; row 1 represents it, and it is one link
    cases.append(("exchanged", r(S.make_row(0, 1, 0, 40, 100, 0, 60, 100, 100), S.make_row(1, 0, 0, 0, 62, 38, 100, 100, 100)), [100, 100], None,
                  [_l(0, 0, 0, 0, (38, 1)), _l(0, 1, 2, 38, NO)], [[0, 2, 138, 0]], c(1, 2, 0, 0, 2, 2, 0, 2, 2, 2)))
    # rings: read 1 (and 2) stored reversed, so the ring runs through the vertices 0, 3 (and 5); row r is the edge (r, r + 1 mod n)
    cases.append(("ring of 2", U.ring_rows(2, [0, 1], 100, 40), [100, 100], None, [_l(0, 0, 0, 0, (40, 0)), _l(0, 1, 3, 40, (40, 1))], [[0, 2, 80, 1]], c(1, 2, 0, 1, 2, 4, 0, 2, 2, 4)))
    cases.append(("ring of 3", U.ring_rows(3, [0, 1, 1], 100, 60), [100] * 3, None, [_l(0, 0, 0, 0, (60, 0)), _l(0, 1, 3, 60, (60, 1)), _l(0, 2, 5, 120, (60, 2))], [[0, 3, 180, 1]],
                  c(1, 3, 0, 1, 3, 6, 0, 3, 3, 6)))
    # read 1 is contained: it is no member, and its vertices are not live
    cases.append(("contained between", r(S.make_row(0, 2, 0, 40, 100, 0, 60, 100, 100)), [100, 50, 100], [False, True, False], [_l(0, 0, 0, 0, (40, 0)), _l(0, 1, 4, 40, NO)], [[0, 2, 140, 0]],
                  c(1, 2, 0, 0, 2, 2, 0, 2, 1, 2)))
    # three reads of 2^32 - 1 bases that share 295: the second link starts beyond 2^32
    step = BIG - 295
    cases.append(("near 2^32", r(S.make_row(0, 1, 0, step, BIG, 0, 295, BIG, BIG), S.make_row(1, 2, 0, step, BIG, 0, 295, BIG, BIG)), [BIG] * 3, None,
                  [_l(0, 0, 0, 0, (step, 0)), _l(0, 1, 2, step, (step, 1)), _l(0, 2, 4, 2 * step, NO)], [[0, 3, 2 * step + BIG, 0]], c(1, 3, 0, 0, 3, 4, 0, 3, 2, 4)))
    return cases


@pytest.mark.parametrize("case", hand_cases(), ids=lambda c: c[0])
def test_hand_cases(case):
    name, rows, lens, contained, layout, table, counts = case
    ref = U.unitigs(rows, lens, contained)
    assert ref["layout"].tolist() == layout and ref["table"].tolist() == table and ref["info"] == counts
    moved = rows.copy()
    moved[:, 0] += np.uint64(7 << 32 | 7)
    ref7 = U.unitigs(moved, lens, contained, rid_base=7)
    assert [[a, b - (7 << 1), c, d] for a, b, c, d in ref7["layout"].tolist()] == layout and ref7["table"].tolist() == table


def test_ring_rows_by_hand():
    # reads 0 and 1 as stored, 100 bases, 40 apart on a circle of 80: read 0's last 60 bases are read 1's first 60, and the other way round
    assert np.array_equal(U.ring_rows(2, [0, 0], 100, 40), np.array([S.make_row(0, 1, 0, 40, 100, 0, 60, 100, 100), S.make_row(0, 1, 0, 0, 60, 40, 100, 100, 100)], dtype=np.uint64))
    rows = U.ring_rows(5, [0, 1, 0, 1, 1], 100, 60, rid_base=3)
    assert S.row_pairs(rows, 3) == [(0, 1), (1, 2), (2, 3), (3, 4), (0, 4)] and [int(r[0]) >> 63 for r in rows] == [1, 1, 1, 0, 1]
    assert S.reduce_rows(rows, [100] * 5, rid_base=3, fuzz=0)["row_class"].tolist() == [S.KEPT] * 5


def test_offsets_beyond_32_bits():
    ref = U.unitigs(*hand_cases()[-1][1:4])
    assert int(ref["layout"][2, 2]) > 1 << 32 and int(ref["table"][0, 2]) == 3 * BIG - 2 * 295 > 1 << 33


def test_refusals_of_the_reference():
    rows, lens = hand_cases()[1][1], [100, 120]
    with pytest.raises(ValueError, match="not the lengths"):
        U.unitigs(rows, [101, 120])
    with pytest.raises(ValueError, match="outside"):
        U.unitigs(rows, [100])
    with pytest.raises(ValueError, match="1 of 1 rows name a read whose contained bit is set"):
        U.unitigs(rows, lens, [False, True])
    for bad in (S.make_row(0, 0, 0, 40, 100, 0, 60, 100, 100), S.make_row(0, 1, 0, 0, 100, 10, 110, 100, 120), S.make_row(0, 1, 0, 10, 90, 0, 80, 100, 120)):      # SELF, A_CONTAINED, INTERNAL
        with pytest.raises(ValueError, match="1 of 2 rows are no dovetails: this is not a list of string graph edges"):
            U.unitigs(np.array([rows[0], bad], dtype=np.uint64), lens)


@pytest.mark.parametrize("seed", range(12))
def test_unitigs_of_an_exact_layout_are_the_runs_of_neighbours(seed):
    rng = np.random.default_rng(2000 + seed)
    starts, lens, strands = S.random_layout(rng, 150, 6000, 80, 200)      # thin enough for coverage gaps
    red = S.reduce_rows(S.layout_rows(starts, lens, strands, 20), lens, fuzz=0)
    ref = U.unitigs(red["kept"], lens, red["contained"])
    runs = U.line_runs(starts, lens, red["contained"], 20)
    assert len(runs) > 1 and max(len(x) for x in runs) > 3
    got = []
    for first, reads, bases, circular in ref["table"].tolist():
        m = ref["layout"][first:first + reads]
        rid, rev, off = (m[:, 1] >> np.uint64(1)).astype(np.int64), (m[:, 1] & np.uint64(1)).astype(np.int64), m[:, 2].astype(np.int64)
        assert not circular and (m[:, 0] & np.uint64(0xFFFFFFFF)).tolist() == list(range(reads))
        # the smallest read is forward; the members lie in line order or against it, the offsets are the distances on the line
        flip = int(rev[0] != strands[rid[0]])
        assert rev[np.argmin(rid)] == 0 and np.array_equal(rev, strands[rid] ^ flip)
        pos = starts[rid] if not flip else -(starts[rid] + lens[rid])
        assert np.array_equal(off, pos - pos[0]) and bases == off[-1] + lens[rid[-1]]
        got.append(rid.tolist()[::-1] if flip else rid.tolist())
    assert sorted(got) == sorted(runs)
    info = ref["info"]
    assert info["unitigs"] == len(runs) and info["members"] == info["live_reads"] == int((~red["contained"]).sum()) and info["branch_vertices"] == 0
    assert info["links"] == 2 * (info["members"] - info["unitigs"]) == info["arcs"] and info["longest"] == max(len(x) for x in runs)
