"""tests/gapped_ref.py -- the definition of hsk_pair_diags_extend_gapped (include/hsk.h) base by base, which the GPU tests of the gapped
extension compare with -- held to rows written out by hand: insertions and deletions in either read, both orientations, a gap in the column
next to the seed, a gap that would end at the read's end, the two tie rules, a deletion of three bases that a band of two cannot cross; its
bulk form (all rows side by side, one antidiagonal per step) held to the row form on random rows with indels; and band 0 held to the
ungapped reference.  No GPU."""
import numpy as np
import pytest

from tests import extend_ref as X
from tests import gapped_ref as G
from tests.test_extend_ref import random_case

c = X.codes
SEED = "ACGT"


def _one(a, b, pa, pb, o=0, K=4, **kw):
    """the row without the cell count"""
    return G.extend_one(c(a), c(b), pa, pb, K, o, **kw)[:7]


def test_sides_written_out_by_hand():
    # five matches, a base that only x has, five matches: the gap costs one edit
    assert G.side(c("GGATCTCGATA"), c("GGATCCGATA"), band=1)[:4] == (9, 11, 10, 1)
    assert G.side(c("GGATCCGATA"), c("GGATCTCGATA"), band=1)[:4] == (9, 10, 11, 1)
    # band 0 has no gaps: the walk is the ungapped one and stops at 5 (T/C, then C/G, G/A, A/T, T/A)
    assert G.side(c("GGATCTCGATA"), c("GGATCCGATA"), band=0)[:4] == (5, 5, 5, 0)
    # the gap in the first column: a drop of 1, which xdrop 0 does not allow
    assert G.side(c("TGGATCCGA"), c("GGATCCGA"), band=1)[:4] == (7, 9, 8, 1)
    assert G.side(c("TGGATCCGA"), c("GGATCCGA"), band=1, xdrop=0) == (0, 0, 0, 0, 0)
    # a base behind y's end: the gap cell (6, 5) is live but raises nothing
    assert G.side(c("GGATCT"), c("GGATC"), band=3)[:4] == (5, 5, 5, 0)
    # fewer edits at equal score: one substitution (-2, one edit) against an insertion and a deletion (-1 -1, two edits)
    assert G.side(c("GGATACG"), c("GGACACG"), match=1, mismatch=2, gap=1, band=2)[:4] == (4, 7, 7, 1)
    # the smallest i: with gap 0 the cells (1, 2) and (2, 1) of antidiagonal 3 both hold (1, 1)
    assert G.side(c("AC"), c("CA"), match=1, mismatch=1, gap=0, band=1)[:4] == (1, 1, 2, 1)
    # cells: x = y = "A", band 1: (1,0) and (0,1) with (-1, 1), (1,1) with (1, 0); band 0: (1,1) alone
    assert G.side(c("A"), c("A"), band=1)[4] == 3 and G.side(c("A"), c("A"), band=0)[4] == 1
    # empty sides
    assert G.side([], c("ACG"), band=5, xdrop=7) == (0, 0, 0, 0, 3) and G.side([], [], band=5) == (0, 0, 0, 0, 0)


def test_rows_written_out_by_hand():
    right_a, right_b = "GGATCTCGATA", "GGATCCGATA"            # an insertion in A behind the seed
    left_a, left_b = "TTGCA", "TTGGCA"                        # an insertion in B in front of it: from the seed backwards AC|G|GTT against ACGTT
    a, b = left_a + SEED + right_a, left_b + SEED + right_b
    # same strand
    assert _one(a, b, 5, 6, band=1) == (4 + 9 + 4, 0, 20, 0, 20, 2, 15)
    assert _one(b, a, 6, 5, band=1) == (17, 0, 20, 0, 20, 2, 15)
    # opposite strands: B is the reverse complement, its seed at lb - pb - K
    rb = X.revcomp(b)
    assert _one(a, rb, 5, len(b) - 6 - 4, o=1, band=1) == (17, 0, 20, 0, 20, 2, 15)
    # only the right side has room in B (o = 1: B's low end is the right side)
    cut = X.revcomp(SEED + right_b)
    assert _one(a, cut, 5, len(cut) - 4, o=1, band=1) == (4 + 9, 5, 20, 0, 14, 1, 2 | 4 | 8)
    assert _one(a, SEED + right_b, 5, 0, o=0, band=1) == (13, 5, 20, 0, 14, 1, 2 | 4 | 8)
    # the gap in the column next to the seed, either side
    assert _one(SEED + "TGGATCCGA", SEED + "GGATCCGA", 0, 0, band=1) == (4 + 7, 0, 13, 0, 12, 1, 15)
    assert _one("AGCCTAGGT" + SEED, "AGCCTAGG" + SEED, 9, 8, band=1) == (4 + 7, 0, 13, 0, 12, 1, 15)
    # a gap that would end at the read's end is not taken
    assert _one(SEED + "GGATCT", SEED + "GGATC", 0, 0, band=3) == (9, 0, 9, 0, 9, 0, 1 | 4 | 8)
    # the tie rules in a row
    assert _one(SEED + "GGATACG", SEED + "GGACACG", 0, 0, match=1, mismatch=2, gap=1, band=2) == (8, 0, 11, 0, 11, 1, 15)
    assert _one(SEED + "AC", SEED + "CA", 0, 0, match=1, mismatch=1, gap=0, band=1) == (5, 0, 5, 0, 6, 1, 1 | 4 | 8)
    # N is A; a seed that is none
    assert _one(SEED + "N", SEED + "A", 0, 0) == (5, 0, 5, 0, 5, 0, 15)
    with pytest.raises(G.NotASeed):
        _one("ACGTA", "ACCTA", 0, 0)
    rows = [X.diag_row(10, 11, 0, 5, 6, support=3), X.diag_row(10, 12, 1, 5, len(b) - 10, support=9)]
    out, columns, cells = G.extend_rows(rows, [a, b, rb], 4, rid_base=10, band=1)
    assert out.tolist() == [[10 << 32 | 11, 17, 20, 20, 2 << 32 | 15, 3], [1 << 63 | 10 << 32 | 12, 17, 20, 20, 2 << 32 | 15, 9]] and columns == 40 and cells > 40
    assert G.extend_rows(rows, [a, b, rb], 4, rid_base=10, band=1, min_score=18)[0].shape == (0, 6)
    assert G.extend_rows(rows, [a, b, rb], 4, rid_base=10, band=1, min_length=20)[0].shape == (2, 6)


def test_a_deletion_of_three_bases_next_to_a_seed():
    """A = 150 bases of a genome, B the same without bases 100 .. 102, the seed at 60 (K = 31).  Left of the seed 60 columns match.  Right
    of it 9 match; the ungapped walk and a band of 2 cannot follow B; a band of 3 or more pays 3 and takes the other 47: 31 + 60 + 9 - 3 + 47."""
    g = "".join(np.random.default_rng(5).choice(list("ACGT"), 150))
    a, b = g, g[:100] + g[103:]
    ungapped = X.extend_one(c(a), c(b), 60, 60, 31, 0)
    assert ungapped[0] < 144 and ungapped[2] < 150
    assert _one(a, b, 60, 60, K=31, band=0) == ungapped
    narrow = _one(a, b, 60, 60, K=31, band=2)
    assert ungapped[0] <= narrow[0] < 144 and narrow[2] < 150
    for band in (3, 4, 15, 63):
        assert _one(a, b, 60, 60, K=31, band=band) == (144, 0, 150, 0, 147, 3, 15)
    rb = X.revcomp(b)
    assert _one(a, rb, 60, len(b) - 60 - 31, o=1, K=31, band=3) == (144, 0, 150, 0, 147, 3, 15)
    assert _one(b, a, 60, 60, K=31, band=3) == (144, 0, 147, 0, 150, 3, 15)


@pytest.mark.parametrize("score", [(1, 1, 7), (2, 3, 5), (1, 0, 0)])
def test_band_0_is_the_ungapped_call(score):
    rng = np.random.default_rng(99 + score[2])
    reads, rows = random_case(rng, 120, 500, 31, 31, 260, genome=1500, err=0.05)
    m, mm, xd = score
    want, wcols = X.extend_rows(rows, reads, 31, match=m, mismatch=mm, xdrop=xd)
    for gap in (0, 9):
        got, gcols, cells = G.extend_rows(rows, reads, 31, match=m, mismatch=mm, gap=gap, xdrop=xd, band=0)
        assert np.array_equal(got, want) and gcols == wcols and cells > 0
    got, gcols, bcells = G.extend_rows_bulk(rows, reads, 31, match=m, mismatch=mm, gap=9, xdrop=xd, band=0)
    assert np.array_equal(got, want) and gcols == wcols and bcells == cells


@pytest.mark.parametrize("K,score,band", [(31, (1, 1, 1, 7), 15), (31, (2, 3, 1, 5), 7), (51, (1, 0, 0, 4), 3), (5, (3, 2, 4, 11), 1), (31, (1, 1, 1, 7), 63)])
def test_bulk_form_equals_the_row_form(K, score, band):
    rng = np.random.default_rng(K * 7 + band)
    reads, rows = G.indel_case(rng, 120, 500, K, K + 9, 260, genome=1500, sub=0.03, indel=0.02)
    assert rows.shape[0] == 500 and 0 < int((rows[:, 0] >> np.uint64(63)).sum()) < rows.shape[0]
    m, mm, gp, xd = score
    want, wcols, wcells = G.extend_rows(rows, reads, K, match=m, mismatch=mm, gap=gp, xdrop=xd, band=band)
    got, gcols, gcells = G.extend_rows_bulk(rows, reads, K, match=m, mismatch=mm, gap=gp, xdrop=xd, band=band)
    assert np.array_equal(got, want) and gcols == wcols and gcells == wcells
    assert int((want[:, 4] >> np.uint64(32)).sum()) > 0
    spans_differ = ((want[:, 2] & np.uint64(0xFFFFFFFF)) - (want[:, 2] >> np.uint64(32))) != ((want[:, 3] & np.uint64(0xFFFFFFFF)) - (want[:, 3] >> np.uint64(32)))
    assert spans_differ.any()                                         # a gap was really crossed
    med = int(np.median(want[:, 1]))
    want, _, _ = G.extend_rows(rows, reads, K, match=m, mismatch=mm, gap=gp, xdrop=xd, band=band, min_score=med, min_length=K + 10)
    got, _, _ = G.extend_rows_bulk(rows, reads, K, match=m, mismatch=mm, gap=gp, xdrop=xd, band=band, min_score=med, min_length=K + 10)
    assert 0 < want.shape[0] < rows.shape[0] and np.array_equal(got, want)
