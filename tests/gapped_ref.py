"""The definition of hsk_pair_diags_extend_gapped (include/hsk.h), base by base on code lists: the reference the GPU tests of the banded,
gapped x-drop extension compare with.  side() walks one side with its cells in dictionaries, one antidiagonal at a time, and knows nothing of
packed words, windows, lanes or packed (score, edits) pairs; extend_rows_bulk is the same walk for many rows side by side in numpy, held
to the row form by tests/test_gapped_ref.py, which also holds side() to rows written out by hand.  indel_case makes reads with
substitutions, insertions and deletions whose seeds are tracked through the indels."""
import numpy as np

from tests import extend_ref as X
from tests.extend_ref import NotASeed, codes, diag_row, revcomp  # noqa: F401  (what the tests of the gapped call use beside this module)

MAX_SPAN = 1 << 22


def side(x, y, match=1, mismatch=1, gap=1, xdrop=7, band=15):
    """x, y: the side's two base sequences as code lists (x[0] is x_1).  Returns (best, i*, j*, e*, cells)."""
    na, nb = len(x), len(y)
    best, bi, bj, be, cells = 0, 0, 0, 0, 0
    prev2, prev = {}, {0: (0, 0)}                        # the cells of antidiagonals d - 2 and d - 1 by i: (s, e)
    dead = 0
    for d in range(1, na + nb + 1):
        cur = {}
        for i in range(max(0, d - nb), min(na, d) + 1):
            j = d - i
            if abs(i - j) > band:
                continue
            cands = []
            if i - 1 in prev2:                           # (i-1, j-1)
                s, e = prev2[i - 1]
                cands.append((s + match, e) if x[i - 1] == y[j - 1] else (s - mismatch, e + 1))
            if i - 1 in prev:                            # (i-1, j)
                s, e = prev[i - 1]
                cands.append((s - gap, e + 1))
            if i in prev:                                # (i, j-1)
                s, e = prev[i]
                cands.append((s - gap, e + 1))
            if not cands:
                continue
            s, e = min(cands, key=lambda c: (-c[0], c[1]))
            if best - s > xdrop:
                continue
            cur[i] = (s, e)
        cells += len(cur)
        if cur:
            dead = 0
            i = min(cur, key=lambda t: (-cur[t][0], cur[t][1], t))
            if cur[i][0] > best:
                best, bi, bj, be = cur[i][0], i, d - i, cur[i][1]
        else:
            dead += 1
            if dead == 2:
                break
        prev2, prev = prev, cur
    return best, bi, bj, be, cells


def sides(a, b, pa, pb, K, o):
    """the table of include/hsk.h: ((x, y) of the right side, (x, y) of the left side)"""
    if not o:
        return (a[pa + K:], b[pb + K:]), (a[:pa][::-1], b[:pb][::-1])
    return (a[pa + K:], [3 - c for c in b[:pb][::-1]]), (a[:pa][::-1], [3 - c for c in b[pb + K:]])


def extend_one(a, b, pa, pb, K, o, match=1, mismatch=1, gap=1, xdrop=7, band=15):
    """a, b: lists of base codes.  Returns (score, a_lo, a_hi, b_lo, b_hi, edits, ends, cells); NotASeed as extend_ref.extend_one."""
    la, lb = len(a), len(b)
    if pa + K > la or pb + K > lb:
        raise NotASeed("the seed does not fit its reads")
    for t in range(K):
        x, y = X.column(a, b, pa, pb, K, o, t)
        if x != y:
            raise NotASeed("the seed's columns do not all match")
    if la + lb >= MAX_SPAN:
        raise ValueError("la + lb >= 2^22")
    (xr, yr), (xl, yl) = sides(a, b, pa, pb, K, o)
    br, ir, jr, er, cr = side(xr, yr, match, mismatch, gap, xdrop, band)
    bl, il, jl, el, cl = side(xl, yl, match, mismatch, gap, xdrop, band)
    a_lo, a_hi = pa - il, pa + K + ir
    b_lo, b_hi = (pb - jl, pb + K + jr) if not o else (pb - jr, pb + K + jl)
    ends = (a_lo == 0) | (a_hi == la) << 1 | (b_lo == 0) << 2 | (b_hi == lb) << 3
    return K * match + br + bl, a_lo, a_hi, b_lo, b_hi, er + el, ends, cr + cl


def extend_rows(rows, reads, K, rid_base=0, match=1, mismatch=1, gap=1, xdrop=7, band=15, min_score=0, min_length=0):
    """rows: [n, 6] uint64 diagonal rows; reads: a list of strings or of code lists.  Returns (the [m, 6] uint64 overlap rows that survive the
    filter, in the input's order; the sum of a_hi - a_lo before the filter; the live cells of all rows)."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 6)
    cs = [codes(r) if isinstance(r, str) else list(r) for r in reads]
    out, columns, cells = [], 0, 0
    for key, _, _, support, first, _ in rows.tolist():
        o = key >> 63
        ra, rb = ((key >> 32) & 0x7FFFFFFF) - rid_base, (key & 0xFFFFFFFF) - rid_base
        score, a_lo, a_hi, b_lo, b_hi, ed, ends, nc = extend_one(cs[ra], cs[rb], first >> 32, first & 0xFFFFFFFF, K, o, match, mismatch, gap, xdrop, band)
        columns += a_hi - a_lo
        cells += nc
        if score >= min_score and a_hi - a_lo >= min_length:
            out.append([key, score, a_lo << 32 | a_hi, b_lo << 32 | b_hi, ed << 32 | ends, support])
    return np.array(out, dtype=np.uint64).reshape(-1, 6), columns, cells


_NEG = -(1 << 36)                                        # a dead cell's score in the bulk form
_EB = 1 << 24                                            # key = s * _EB + (_EB - 1 - e): the larger key is the better pair (e < 2^22)


def _bulk_side(xs, ys, na, nb, match, mismatch, gap, xdrop, band):
    """xs[r, i] = x_i of row r for 1 <= i <= na[r] (column 0 and the padding: anything), ys likewise.  One antidiagonal per step, the cells of
    diagonal k = i - j in column k + band.  Returns best, i*, j*, e*, cells: one int64 array each."""
    n, W = na.shape[0], 2 * band + 1
    k = np.arange(-band, band + 1)
    dead_key = _NEG * _EB
    prev2 = np.full((n, W), dead_key, np.int64)
    prev = prev2.copy()
    prev[:, band] = _EB - 1                              # (0, 0): s = 0, e = 0
    best, bi, bj, be, cells, dead = (np.zeros(n, np.int64) for _ in range(6))
    active = (na + nb) > 0
    every = np.arange(n)
    pad = np.full((n, 1), dead_key, np.int64)
    for d in range(1, int((na + nb).max()) + 1 if n else 0):
        if not active.any():
            break
        i, j = (d + k) >> 1, (d - k) >> 1
        here = ((d + k) % 2 == 0) & (i >= 0) & (j >= 0)
        exists = here[None, :] & (i[None, :] <= na[:, None]) & (j[None, :] <= nb[:, None]) & active[:, None]
        eq = xs[:, np.clip(i, 0, xs.shape[1] - 1)] == ys[:, np.clip(j, 0, ys.shape[1] - 1)]
        cand = np.where(eq, prev2 + match * _EB, prev2 - mismatch * _EB - 1)
        up = np.concatenate([pad, prev[:, :-1]], axis=1)                 # (i-1, j): diagonal k - 1
        left = np.concatenate([prev[:, 1:], pad], axis=1)                # (i, j-1): diagonal k + 1
        cand = np.maximum(cand, np.maximum(up, left) - gap * _EB - 1)
        s = cand >> 24
        live = exists & (cand > dead_key // 2) & (best[:, None] - s <= xdrop)
        cur = np.where(live, cand, dead_key)
        cells += live.sum(axis=1)
        t = cur.argmax(axis=1)                           # the first of the largest: the smallest i
        top = cur[every, t]
        anyl = top > dead_key // 2
        ts = top >> 24
        up_ = anyl & (ts > best)
        best[up_], bi[up_], be[up_] = ts[up_], i[t[up_]], (_EB - 1) - (top[up_] & (_EB - 1))
        bj[up_] = d - bi[up_]
        dead = np.where(anyl, 0, dead + 1)
        active &= (dead < 2) & (d < na + nb)
        prev2, prev = prev, cur
    return best, bi, bj, be, cells


def extend_rows_bulk(rows, reads, K, rid_base=0, match=1, mismatch=1, gap=1, xdrop=7, band=15, min_score=0, min_length=0):
    """extend_rows for many rows, all rows side by side in numpy.  reads: a list of strings or code lists, or the (matrix, lengths) of
    extend_ref.code_matrix.  tests/test_gapped_ref.py compares it with extend_rows."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 6)
    M, lens = reads if isinstance(reads, tuple) else X.code_matrix(reads)
    n = rows.shape[0]
    if not n:
        return np.zeros((0, 6), np.uint64), 0, 0
    key, support, first = rows[:, 0], rows[:, 3], rows[:, 4]
    o = (key >> np.uint64(63)).astype(np.int64)
    ra = ((key >> np.uint64(32)) & np.uint64(0x7FFFFFFF)).astype(np.int64) - rid_base
    rb = (key & np.uint64(0xFFFFFFFF)).astype(np.int64) - rid_base
    pa, pb = (first >> np.uint64(32)).astype(np.int64), (first & np.uint64(0xFFFFFFFF)).astype(np.int64)
    la, lb = lens[ra], lens[rb]
    if ((pa + K > la) | (pb + K > lb)).any():
        raise NotASeed("a seed does not fit its reads")
    for t in range(K):
        y = np.where(o == 0, M[rb, np.where(o == 0, pb + t, 0)], 3 - M[rb, np.where(o == 1, pb + K - 1 - t, 0)])
        if not (M[ra, pa + t] == y).all():
            raise NotASeed("a seed's columns do not all match")
    if ((la + lb) >= MAX_SPAN).any():
        raise ValueError("la + lb >= 2^22")
    L = M.shape[1]

    def seq(r, p0, step, comp, count):
        """[n, max(count) + 1]: column i holds base p0 + step * i of read r (complemented), for 1 <= i <= count"""
        idx = p0[:, None] + step[:, None] * np.arange(int(count.max()) + 1)[None, :]
        v = M[r[:, None], np.clip(idx, 0, L - 1)]
        return np.where(comp[:, None] == 1, 3 - v, v)

    one, zero = np.ones(n, np.int64), np.zeros(n, np.int64)
    res = []
    for right in (True, False):
        na = la - pa - K if right else pa
        xs = seq(ra, pa + K - 1 if right else pa, one if right else -one, zero, na)
        onwards = (o == 0) == right
        nb = np.where(onwards, lb - pb - K, pb)
        ys = seq(rb, np.where(onwards, pb + K - 1, pb), np.where(onwards, 1, -1), o, nb)
        res.append(_bulk_side(xs, ys, na, nb, match, mismatch, gap, xdrop, band))
    (br, ir, jr, er, cr), (bl, il, jl, el, cl) = res
    score = K * match + br + bl
    a_lo, a_hi = pa - il, pa + K + ir
    b_lo, b_hi = np.where(o == 0, pb - jl, pb - jr), np.where(o == 0, pb + K + jr, pb + K + jl)
    ends = (a_lo == 0) * 1 + (a_hi == la) * 2 + (b_lo == 0) * 4 + (b_hi == lb) * 8
    out = np.stack([key, score.astype(np.uint64), (a_lo << 32 | a_hi).astype(np.uint64), (b_lo << 32 | b_hi).astype(np.uint64),
                    ((er + el) << 32 | ends).astype(np.uint64), support], axis=1)
    keep = (score >= min_score) & (a_hi - a_lo >= min_length)
    return out[keep], int((a_hi - a_lo).sum()), int((cr + cl).sum())


def mutate(fwd, protect, rng, sub, indel):
    """A copy of the code array `fwd` with substitutions (rate sub) and indels (rate indel, half insertions in front of a base and half
    deletions) at the positions that are not protected; and where[p] = the place of base p in the copy (-1: deleted)."""
    out, where = [], np.full(len(fwd), -1, np.int64)
    u = rng.random(len(fwd))
    fresh = rng.integers(0, 4, len(fwd))
    other = rng.integers(1, 4, len(fwd))
    for p, c in enumerate(fwd.tolist()):
        if not protect[p]:
            if u[p] < indel / 2:
                continue                                 # deleted
            if u[p] < indel:
                out.append(int(fresh[p]))                # an insertion in front of it
            elif u[p] < indel + sub:
                c = (c + int(other[p])) & 3
        where[p] = len(out)
        out.append(c)
    return np.array(out, dtype=np.int64), where


def indel_case(rng, nreads, nrows, K, lo, hi, genome=5000, sub=0.02, indel=0.01, near=40, share=0.0):
    """Ragged reads cut from a genome, both strands, with substitutions and indels outside a protected seed per row: (reads, rows).  A row's
    reads overlap in the genome; the seed is a K-mer of the overlap, protected in both reads and found again in each through the read's
    indels, so every seed is valid by construction.  lo .. hi bound a read's span in the genome; indels move its length by a few bases.
    share: a row's reads overlap in at least this part of the longer one (long overlaps meet indels; a K-mer's worth of overlap does not)."""
    g = rng.integers(0, 4, genome)
    start = np.sort(rng.integers(0, genome - hi, nreads))
    length = rng.integers(lo, hi + 1, nreads)
    strand = rng.integers(0, 2, nreads)
    protect = [np.zeros(n, bool) for n in length]
    picks, tries = [], 0
    while len(picks) < nrows and tries < 50 * nrows:
        tries += 1
        i = int(rng.integers(0, nreads - 1))
        j = int(rng.integers(i + 1, min(nreads, i + near)))
        s0, s1 = max(start[i], start[j]), min(start[i] + length[i], start[j] + length[j])
        if s1 - s0 < K or s1 - s0 < share * max(length[i], length[j]):
            continue
        gs = int(rng.integers(s0, s1 - K + 1))
        protect[i][gs - start[i]:gs - start[i] + K] = True
        protect[j][gs - start[j]:gs - start[j] + K] = True
        picks.append((i, j, gs))
    fwd, where = [], []
    for r in range(nreads):
        f, w = mutate(g[start[r]:start[r] + length[r]], protect[r], rng, sub, indel)
        fwd.append(f)
        where.append(w)
    reads = [(3 - f[::-1]) if s else f for f, s in zip(fwd, strand)]
    out = []
    for i, j, gs in picks:
        pi, pj = int(where[i][gs - start[i]]), int(where[j][gs - start[j]])
        pa = len(fwd[i]) - pi - K if strand[i] else pi
        pb = len(fwd[j]) - pj - K if strand[j] else pj
        out.append(diag_row(i, j, int(strand[i] ^ strand[j]), int(pa), int(pb), support=int(rng.integers(1, 100))))
    out.sort(key=lambda r: (r[0] >> 63, r[0]))
    return ["".join("ACGT"[x] for x in r) for r in reads], np.array(out, dtype=np.uint64).reshape(-1, 6)
