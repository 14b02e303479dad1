"""The definition of hsk_pair_diags_extend (include/hsk.h), base by base on strings: the reference the GPU tests of the ungapped x-drop
extension compare with.  Nothing here looks at packed words, windows or runs; tests/test_extend_ref.py holds it to overlaps written out
by hand."""
import numpy as np

_CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 0, "a": 0, "c": 1, "g": 2, "t": 3, "n": 0}


def codes(seq):
    """base codes as the packed bytes hold them: N is A"""
    return [_CODE[ch] for ch in seq]


def revcomp(seq):
    return seq[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def column(a, b, pa, pb, K, o, t):
    """the two codes of column t"""
    return (a[pa + t], b[pb + t]) if not o else (a[pa + t], 3 - b[pb + K - 1 - t])


def valid_range(la, lb, pa, pb, K, o):
    if not o:
        return -min(pa, pb), min(la - pa, lb - pb)
    return max(-pa, pb + K - lb), min(la - pa, pb + K)


class NotASeed(ValueError):
    pass


def extend_one(a, b, pa, pb, K, o, match=1, mismatch=1, xdrop=7):
    """a, b: lists of base codes.  Returns (score, a_lo, a_hi, b_lo, b_hi, mismatches, ends); NotASeed if the seed does not fit or its K
    columns do not all match."""
    la, lb = len(a), len(b)
    if pa + K > la or pb + K > lb:
        raise NotASeed("the seed does not fit its reads")
    t_lo, t_hi = valid_range(la, lb, pa, pb, K, o)
    assert t_lo <= 0 and t_hi >= K
    for t in range(K):
        x, y = column(a, b, pa, pb, K, o, t)
        if x != y:
            raise NotASeed("the seed's columns do not all match")
    s = best = 0
    end = K
    for t in range(K, t_hi):
        x, y = column(a, b, pa, pb, K, o, t)
        s += match if x == y else -mismatch
        if s > best:
            best, end = s, t + 1
        if best - s > xdrop:
            break
    best_r = best
    s = best = 0
    begin = 0
    for t in range(-1, t_lo - 1, -1):
        x, y = column(a, b, pa, pb, K, o, t)
        s += match if x == y else -mismatch
        if s > best:
            best, begin = s, t
        if best - s > xdrop:
            break
    score = K * match + best_r + best
    mm = 0
    for t in range(begin, end):
        x, y = column(a, b, pa, pb, K, o, t)
        mm += x != y
    a_lo, a_hi = pa + begin, pa + end
    if not o:
        b_lo, b_hi = pb + begin, pb + end
    else:
        b_lo, b_hi = pb + K - end, pb + K - begin
    ends = (a_lo == 0) | (a_hi == la) << 1 | (b_lo == 0) << 2 | (b_hi == lb) << 3
    return score, a_lo, a_hi, b_lo, b_hi, mm, ends


def extend_rows(rows, reads, K, rid_base=0, match=1, mismatch=1, xdrop=7, min_score=0, min_length=0):
    """rows: [n, 6] uint64 diagonal rows { key, shared, bin, support, first, last }; reads: a list of strings or of code lists.  Returns the
    [m, 6] uint64 overlap rows { key, score, a_lo << 32 | a_hi, b_lo << 32 | b_hi, mismatches << 32 | ends, support } that survive the
    filter, in the input's order, and the sum of the lengths before the filter."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 6)
    cs = [codes(r) if isinstance(r, str) else r for r in reads]
    out, columns = [], 0
    for key, _, _, support, first, _ in rows.tolist():
        o = key >> 63
        ra, rb = ((key >> 32) & 0x7FFFFFFF) - rid_base, (key & 0xFFFFFFFF) - rid_base
        score, a_lo, a_hi, b_lo, b_hi, mm, ends = extend_one(cs[ra], cs[rb], first >> 32, first & 0xFFFFFFFF, K, o, match, mismatch, xdrop)
        columns += a_hi - a_lo
        if score >= min_score and a_hi - a_lo >= min_length:
            out.append([key, score, a_lo << 32 | a_hi, b_lo << 32 | b_hi, mm << 32 | ends, support])
    return np.array(out, dtype=np.uint64).reshape(-1, 6), columns


def code_matrix(reads):
    """(codes [nreads, longest] uint8 padded with 0, lengths) of a list of strings or code lists"""
    cs = [codes(r) if isinstance(r, str) else r for r in reads]
    lens = np.array([len(c) for c in cs], dtype=np.int64)
    m = np.zeros((len(cs), max(1, int(lens.max()) if len(cs) else 1)), dtype=np.int64)
    for i, c in enumerate(cs):
        m[i, :len(c)] = c
    return m, lens


def extend_rows_bulk(rows, reads, K, rid_base=0, match=1, mismatch=1, xdrop=7, min_score=0, min_length=0):
    """extend_rows for many rows: the same walk, one column per step, all rows of the list side by side in numpy (a row leaves the step
    loop where extend_one breaks).  reads: a list of strings or code lists, or the (matrix, lengths) of code_matrix.  The mismatches of
    an overlap are those seen when `best` was last raised: the columns behind the last raise are not part of the overlap.
    tests/test_extend_ref.py compares it with extend_rows."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 6)
    M, lens = reads if isinstance(reads, tuple) else code_matrix(reads)
    key, support, first = rows[:, 0], rows[:, 3], rows[:, 4]
    o = (key >> np.uint64(63)).astype(np.int64)
    ra = ((key >> np.uint64(32)) & np.uint64(0x7FFFFFFF)).astype(np.int64) - rid_base
    rb = (key & np.uint64(0xFFFFFFFF)).astype(np.int64) - rid_base
    pa, pb = (first >> np.uint64(32)).astype(np.int64), (first & np.uint64(0xFFFFFFFF)).astype(np.int64)
    la, lb = lens[ra], lens[rb]
    if ((pa + K > la) | (pb + K > lb)).any():
        raise NotASeed("a seed does not fit its reads")
    t_lo = np.where(o == 0, -np.minimum(pa, pb), np.maximum(-pa, pb + K - lb))
    t_hi = np.where(o == 0, np.minimum(la - pa, lb - pb), np.minimum(la - pa, pb + K))

    def col(idx, t):
        x = M[ra[idx], pa[idx] + t]
        y = np.where(o[idx] == 0, M[rb[idx], np.where(o[idx] == 0, pb[idx] + t, 0)], 3 - M[rb[idx], np.where(o[idx] == 1, pb[idx] + K - 1 - t, 0)])
        return x == y

    every = np.arange(rows.shape[0])
    for t in range(K):
        if not col(every, t).all():
            raise NotASeed("a seed's columns do not all match")

    def side(ts, inside, taken):
        n = rows.shape[0]
        s, best, seen, mm = (np.zeros(n, np.int64) for _ in range(4))
        edge = np.zeros(n, np.int64)                     # columns taken at best
        active = np.ones(n, bool)
        for t in ts:
            idx = np.flatnonzero(active & inside(t))
            if not idx.size:
                break
            eq = col(idx, t)
            s[idx] += np.where(eq, match, -mismatch)
            seen[idx] += ~eq
            up = idx[s[idx] > best[idx]]
            best[up], edge[up], mm[up] = s[up], taken(t), seen[up]
            active[idx[best[idx] - s[idx] > xdrop]] = False
            active &= inside(t)
        return best, edge, mm

    if rows.shape[0]:
        best_r, right, mm_r = side(range(K, int(t_hi.max())), lambda t: t < t_hi, lambda t: t + 1 - K)
        best_l, left, mm_l = side(range(-1, int(t_lo.min()) - 1, -1), lambda t: t >= t_lo, lambda t: -t)
    else:
        best_r = right = mm_r = best_l = left = mm_l = np.zeros(0, np.int64)
    begin, end = -left, K + right
    score = K * match + best_r + best_l
    a_lo, a_hi = pa + begin, pa + end
    b_lo, b_hi = np.where(o == 0, pb + begin, pb + K - end), np.where(o == 0, pb + end, pb + K - begin)
    ends = (a_lo == 0) * 1 + (a_hi == la) * 2 + (b_lo == 0) * 4 + (b_hi == lb) * 8
    out = np.stack([key, score.astype(np.uint64), (a_lo << 32 | a_hi).astype(np.uint64), (b_lo << 32 | b_hi).astype(np.uint64),
                    ((mm_r + mm_l) << 32 | ends).astype(np.uint64), support], axis=1)
    keep = (score >= min_score) & (a_hi - a_lo >= min_length)
    return out[keep], int((a_hi - a_lo).sum())


def diag_row(rid_a, rid_b, o, pa, pb, support=1, shared=None, bin=0):
    """a diagonal row by hand: `first` is the seed (pa, pb); last = first"""
    first = pa << 32 | pb
    return [o << 63 | rid_a << 32 | rid_b, support if shared is None else shared, bin, support, first, first]
