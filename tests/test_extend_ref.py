"""tests/extend_ref.py -- the definition of hsk_pair_diags_extend (include/hsk.h) base by base, which the GPU tests of the extension compare
with -- held to overlaps written out by hand, both orientations; its bulk form (all rows side by side, one column per step) held to the
row-by-row form on random overlaps; and Overlaps.kind(), which is host-side numpy, on rows built by hand.  No GPU."""
import numpy as np
import pytest

from tests import extend_ref as X


def test_overlaps_written_out_by_hand():
    c = X.codes
    # same strand, K = 4: three matching columns on either side, then a mismatch that is not taken
    #   A  T TTT ACGT GGG G        B  C TTT ACGT GGG A
    assert X.extend_one(c("TTTTACGTGGGG"), c("CTTTACGTGGGA"), 4, 4, 4, 0, 1, 1, 2) == (10, 1, 11, 1, 11, 0, 0)
    # one mismatch behind the first column of the right side: xdrop 1 goes on over it (drop 1), xdrop 0 stops there
    a, b = c("AAAAACGTCACC"), c("AAAAACGTCTCC")
    assert X.extend_one(a, b, 4, 4, 4, 0, 1, 1, 1) == (10, 0, 12, 0, 12, 1, 15)
    assert X.extend_one(a, b, 4, 4, 4, 0, 1, 1, 0) == (9, 0, 9, 0, 9, 0, 5)
    # a mismatch penalty of 0: the walk never drops, and the mismatch lies inside the overlap
    assert X.extend_one(a, b, 4, 4, 4, 0, 2, 0, 0) == (22, 0, 12, 0, 12, 1, 15)
    # opposite strands, K = 5: in A's direction B reads TG ACGTA CA against A = GG ACGTA CC; B itself is the reverse complement
    assert X.revcomp("TGACGTACA") == "TGTACGTCA"
    assert X.valid_range(9, 9, 2, 2, 5, 1) == (-2, 7)
    assert X.extend_one(c("GGACGTACC"), c("TGTACGTCA"), 2, 2, 5, 1, 1, 1, 7) == (7, 1, 8, 1, 8, 0, 0)
    # opposite strands, the seed at A's end and (in A's direction) at B's start: nothing to extend, a dovetail
    assert X.revcomp("ACGTAGGG") == "CCCTACGT"
    assert X.valid_range(10, 8, 5, 3, 5, 1) == (0, 5)
    assert X.extend_one(c("TTTTTACGTA"), c("CCCTACGT"), 5, 3, 5, 1, 1, 1, 7) == (5, 5, 10, 3, 8, 0, 2 | 8)
    # N is A
    assert X.extend_one(c("ACGTN"), c("ACGTA"), 0, 0, 4, 0) == (5, 0, 5, 0, 5, 0, 15)
    # a seed that is none
    with pytest.raises(X.NotASeed):
        X.extend_one(c("ACGTA"), c("ACCTA"), 0, 0, 4, 0)
    with pytest.raises(X.NotASeed):
        X.extend_one(c("ACGTA"), c("ACGTA"), 2, 0, 4, 0)


def test_rows_by_hand():
    reads = ["TTTTACGTGGGG", "CTTTACGTGGGA", "GGACGTACC", "TGTACGTCA"]
    rows = [X.diag_row(10, 11, 0, 4, 4, support=3)]
    out, columns = X.extend_rows(rows, reads, 4, rid_base=10, xdrop=2)
    assert out.tolist() == [[10 << 32 | 11, 10, 1 << 32 | 11, 1 << 32 | 11, 0, 3]] and columns == 10
    rows = [X.diag_row(12, 13, 1, 2, 2, support=9)]
    out, columns = X.extend_rows(rows, reads, 5, rid_base=10)
    assert out.tolist() == [[1 << 63 | 12 << 32 | 13, 7, 1 << 32 | 8, 1 << 32 | 8, 0, 9]] and columns == 7
    assert X.extend_rows(rows, reads, 5, rid_base=10, min_score=8)[0].shape == (0, 6)
    assert X.extend_rows(rows, reads, 5, rid_base=10, min_length=7)[0].shape == (1, 6)
    assert X.extend_rows(rows, reads, 5, rid_base=10, min_length=8)[0].shape == (0, 6)


def random_case(rng, nreads, nrows, K, lo, hi, genome=5000, err=0.03):
    """Ragged reads cut from a genome, both strands, with substitutions outside a protected seed per row: (reads, rows); every seed is
    valid by construction.  A row's reads overlap in the genome; the seed is a K-mer of the overlap, protected in both reads."""
    g = rng.integers(0, 4, genome)
    start = rng.integers(0, genome - hi, nreads)
    length = rng.integers(lo, hi + 1, nreads)
    strand = rng.integers(0, 2, nreads)
    order = np.argsort(start, kind="stable")
    start, length, strand = start[order], length[order], strand[order]
    fwd = [g[s:s + n].copy() for s, n in zip(start, length)]
    protect = [np.zeros(n, bool) for n in length]
    rows = []
    tries = 0
    while len(rows) < nrows and tries < 50 * nrows:
        tries += 1
        i = int(rng.integers(0, nreads - 1))
        j = int(rng.integers(i + 1, min(nreads, i + 40)))
        s0, s1 = max(start[i], start[j]), min(start[i] + length[i], start[j] + length[j])
        if s1 - s0 < K:
            continue
        gs = int(rng.integers(s0, s1 - K + 1))
        protect[i][gs - start[i]:gs - start[i] + K] = True
        protect[j][gs - start[j]:gs - start[j] + K] = True
        rows.append((i, j, gs))
    for r in range(nreads):
        hit = (rng.random(length[r]) < err) & ~protect[r]
        fwd[r][hit] = (fwd[r][hit] + rng.integers(1, 4, int(hit.sum()))) & 3
    reads = [(3 - f[::-1]) if s else f for f, s in zip(fwd, strand)]
    out = []
    for i, j, gs in rows:
        pi, pj = gs - start[i], gs - start[j]
        pa = length[i] - pi - K if strand[i] else pi
        pb = length[j] - pj - K if strand[j] else pj
        out.append(X.diag_row(i, j, int(strand[i] ^ strand[j]), int(pa), int(pb), support=int(rng.integers(1, 100))))
    out.sort(key=lambda r: (r[0] >> 63, r[0]))
    return ["".join("ACGT"[x] for x in r) for r in reads], np.array(out, dtype=np.uint64).reshape(-1, 6)


@pytest.mark.parametrize("K,score", [(31, (1, 1, 7)), (31, (2, 3, 0)), (51, (1, 0, 4)), (5, (3, 2, 11))])
def test_bulk_form_equals_the_row_by_row_form(K, score):
    rng = np.random.default_rng(K * 7 + score[2])
    reads, rows = random_case(rng, 150, 600, K, K, 260, genome=1500, err=0.05)
    assert rows.shape[0] > 300 and 0 < int((rows[:, 0] >> np.uint64(63)).sum()) < rows.shape[0]
    m, mm, xd = score
    want, wcols = X.extend_rows(rows, reads, K, match=m, mismatch=mm, xdrop=xd)
    got, gcols = X.extend_rows_bulk(rows, reads, K, match=m, mismatch=mm, xdrop=xd)
    assert np.array_equal(got, want) and gcols == wcols
    assert (int((want[:, 4] >> np.uint64(32)).sum()) > 0) == (xd > 0)      # overlaps with mismatches inside; with xdrop 0 the first mismatch ends a side
    med = int(np.median(want[:, 1]))
    want, _ = X.extend_rows(rows, reads, K, match=m, mismatch=mm, xdrop=xd, min_score=med, min_length=K + 10)
    got, _ = X.extend_rows_bulk(rows, reads, K, match=m, mismatch=mm, xdrop=xd, min_score=med, min_length=K + 10)
    assert 0 < want.shape[0] < rows.shape[0] and np.array_equal(got, want)


def test_kind_on_rows_built_by_hand():
    from hysortk_amd.api import Overlaps
    TOP = 1 << 63
    rows, want = [], []
    for o, ends, kind in [(0, 3, Overlaps.A_CONTAINED), (1, 3, Overlaps.A_CONTAINED), (0, 15, Overlaps.A_CONTAINED), (0, 12, Overlaps.B_CONTAINED), (1, 13, Overlaps.B_CONTAINED),
                          (0, 6, Overlaps.DOVETAIL), (0, 9, Overlaps.DOVETAIL), (0, 5, Overlaps.INTERNAL), (0, 10, Overlaps.INTERNAL), (1, 5, Overlaps.DOVETAIL), (1, 10, Overlaps.DOVETAIL),
                          (1, 6, Overlaps.INTERNAL), (1, 9, Overlaps.INTERNAL), (0, 0, Overlaps.INTERNAL), (1, 0, Overlaps.INTERNAL), (0, 1, Overlaps.INTERNAL), (1, 8, Overlaps.INTERNAL),
                          (0, 7, Overlaps.A_CONTAINED), (1, 14, Overlaps.B_CONTAINED)]:
        rows.append([o * TOP | 3 << 32 | 4, 40, 5 << 32 | 45, 7 << 32 | 47, 2 << 32 | ends, 6])
        want.append(kind)
    ov = Overlaps.from_rows(rows)
    assert ov.kind().tolist() == want
    assert len({Overlaps.INTERNAL, Overlaps.DOVETAIL, Overlaps.A_CONTAINED, Overlaps.B_CONTAINED}) == 4
    assert ov.a_lo.tolist() == [5] * len(rows) and ov.a_hi.tolist() == [45] * len(rows) and ov.b_lo[0] == 7 and ov.b_hi[0] == 47
    assert ov.mismatches[0] == 2 and ov.support[0] == 6 and ov.score[0] == 40 and ov.rid_a[0] == 3 and ov.rid_b[0] == 4
    assert ov.opposite.tolist() == [bool(r[0] >> 63) for r in rows] and np.array_equal(ov.rows(), np.array(rows, dtype=np.uint64))
    assert Overlaps.from_rows(np.zeros((0, 6), np.uint64)).kind().shape == (0,)
