"""The definition of hsk_overlaps_reduce (include/hsk.h) in plain Python: the class of every row, the contained reads, the arcs of the
surviving dovetails and the one round of transitive reduction, with dictionaries and lists and nothing clever -- what the kernels, the
shared header (hysortk_amd/csrc/hsk_strgraph.h) and OverlapGraph.arcs are held to.  tests/test_strgraph_ref.py holds this file to rows written
by hand.  layout_rows makes exact overlap rows from a layout of reads on a line, so that a test needs lengths only."""
import numpy as np

KEPT, REDUCED, INTERNAL, A_CONTAINED, B_CONTAINED, DROPPED_READ, DUPLICATE, SELF = range(8)
NAMES = ("kept", "reduced", "internal", "a_contained", "b_contained", "dropped_read", "duplicate", "self")
DOVETAILS = {(0, 6), (0, 9), (1, 10), (1, 5)}
DEFAULT_FUZZ = 10


def make_row(rid_a, rid_b, o, a_lo, a_hi, b_lo, b_hi, la, lb, score=None, support=1, mismatches=0):
    """one row of the C ABI, its ends bits from the coordinates"""
    ends = (1 if a_lo == 0 else 0) | (2 if a_hi == la else 0) | (4 if b_lo == 0 else 0) | (8 if b_hi == lb else 0)
    return [(o << 63) | (rid_a << 32) | rid_b, (a_hi - a_lo) if score is None else score, (a_lo << 32) | a_hi, (b_lo << 32) | b_hi, (mismatches << 32) | ends, support]


def fields(row, lens, rid_base=0):
    key, score, w2, w3, w4 = (int(x) for x in row[:5])
    f = dict(key=key, score=score, o=key >> 63, rid_a=(key >> 32) & 0x7FFFFFFF, rid_b=key & 0xFFFFFFFF, a_lo=w2 >> 32, a_hi=w2 & 0xFFFFFFFF, b_lo=w3 >> 32, b_hi=w3 & 0xFFFFFFFF, e=w4 & 15)
    f["a"], f["b"] = f["rid_a"] - rid_base, f["rid_b"] - rid_base
    if not (0 <= f["a"] < len(lens) and 0 <= f["b"] < len(lens)):
        raise ValueError("a row names a read outside the reads")
    f["la"], f["lb"] = int(lens[f["a"]]), int(lens[f["b"]])
    ok = f["a_lo"] < f["a_hi"] <= f["la"] and f["b_lo"] < f["b_hi"] <= f["lb"]
    want = (1 if f["a_lo"] == 0 else 0) | (2 if f["a_hi"] == f["la"] else 0) | (4 if f["b_lo"] == 0 else 0) | (8 if f["b_hi"] == f["lb"] else 0)
    if not ok or want != f["e"]:
        raise ValueError("these are not the lengths of the reads the rows were computed from")
    return f


def own_class(f):
    """the class a row has by itself: the first rule that applies; a dovetail is KEPT until the list says otherwise"""
    if f["rid_a"] == f["rid_b"]:
        return SELF
    if f["e"] & 3 == 3:
        return A_CONTAINED
    if f["e"] & 12 == 12:
        return B_CONTAINED
    return KEPT if (f["o"], f["e"]) in DOVETAILS else INTERNAL


def row_arcs(f):
    """the two arcs (v, w, len) of a dovetail: the table of include/hsk.h, line by line"""
    a, b, la, lb = f["a"], f["b"], f["la"], f["lb"]
    oe = (f["o"], f["e"])
    if oe == (0, 6):
        return [(2 * a, 2 * b, f["a_lo"]), (2 * b + 1, 2 * a + 1, lb - f["b_hi"])]
    if oe == (0, 9):
        return [(2 * b, 2 * a, f["b_lo"]), (2 * a + 1, 2 * b + 1, la - f["a_hi"])]
    if oe == (1, 10):
        return [(2 * a, 2 * b + 1, f["a_lo"]), (2 * b, 2 * a + 1, f["b_lo"])]
    if oe == (1, 5):
        return [(2 * b + 1, 2 * a, lb - f["b_hi"]), (2 * a + 1, 2 * b, la - f["a_hi"])]
    raise ValueError("no dovetail")


def reduce_rows(rows, lens, rid_base=0, fuzz=DEFAULT_FUZZ):
    """dict: row_class (uint8 per row), kept (the KEPT rows in order), contained (bool per read), counts (rows per class by name), arcs
    (live arcs of G), degree (arc records per vertex, duplicates included: what max_degree and wave_vertices count), kept_arcs (sorted
    (v, w, len, index among the kept rows))"""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 6)
    n = rows.shape[0]
    F = [fields(r, lens, rid_base) for r in rows]
    cls = [own_class(f) for f in F]
    contained = [False] * len(lens)
    for f, c in zip(F, cls):
        if c == A_CONTAINED:
            contained[f["a"]] = True
        if c == B_CONTAINED:
            contained[f["b"]] = True
    for i, f in enumerate(F):
        if cls[i] == KEPT and (contained[f["a"]] or contained[f["b"]]):
            cls[i] = DROPPED_READ
    degree = {}
    for i, f in enumerate(F):
        if cls[i] == KEPT:
            for v, w, ln in row_arcs(f):
                degree[v] = degree.get(v, 0) + 1
    groups = {}
    for i, f in enumerate(F):
        if cls[i] == KEPT:
            groups.setdefault((f["key"], f["e"]), []).append(i)
    for members in groups.values():
        best = max(members, key=lambda i: (F[i]["score"], -i))
        for i in members:
            if i != best:
                cls[i] = DUPLICATE
    out = {}                                              # v -> [(w, len)]
    shortest = {}                                         # (w, x) -> the shortest live arc (two rows with a and b exchanged can give one arc twice)
    arcs = []                                             # (v, x, len, row)
    for i, f in enumerate(F):
        if cls[i] == KEPT:
            for v, w, ln in row_arcs(f):
                out.setdefault(v, []).append((w, ln))
                shortest[(v, w)] = min(ln, shortest.get((v, w), ln))
                arcs.append((v, w, ln, i))
    reduced = set()
    for v, x, L, i in arcs:
        for w, l1 in out[v]:
            if w >> 1 == v >> 1 or w >> 1 == x >> 1:
                continue
            l2 = shortest.get((w, x))
            if l2 is not None and l1 + l2 <= L + fuzz:
                reduced.add(i)
                break
    for i in reduced:
        cls[i] = REDUCED
    cls = np.array(cls, dtype=np.uint8)
    kept_index = {i: k for k, i in enumerate(np.flatnonzero(cls == KEPT).tolist())}
    kept_arcs = sorted((v, x, L, kept_index[i]) for v, x, L, i in arcs if cls[i] == KEPT)
    counts = {name: int((cls == c).sum()) for c, name in enumerate(NAMES)}
    return dict(row_class=cls, kept=rows[cls == KEPT], contained=np.array(contained, dtype=bool), counts=counts, arcs=len(arcs), degree=degree, kept_arcs=kept_arcs)


def expected_info(ref, n, wave_degree):
    """the counts of the call's info from a reference result; wave_degree: the threshold the call reports (0xFFFFFFFF: no vertex)"""
    deg = list(ref["degree"].values())
    info = dict(ref["counts"], input_rows=n, contained_reads=int(ref["contained"].sum()), arcs=ref["arcs"], max_degree=max(deg, default=0),
                wave_vertices=0 if wave_degree == 0xFFFFFFFF else sum(1 for d in deg if d >= wave_degree))
    return info


def layout_rows(starts, lens, strands, min_ov, jitter=0, rng=None, rid_base=0):
    """Exact overlap rows of reads laid on a line: read r covers [starts[r], starts[r] + lens[r]) and is stored reversed if strands[r].
    One row per pair of reads that share at least min_ov bases, a = the smaller index: the shared interval in each read's own
    coordinates (flipped for strand 1), o = strand_a ^ strand_b, ends from the coordinates, score = the shared bases.  jitter: every
    coordinate that does not touch an end of its read moves by up to +-jitter bases (what indels do to an overlap's ends) and stays
    inside the read.  [n, 6] uint64, ordered by (a, b)."""
    starts, lens, strands = (np.asarray(x, dtype=np.int64) for x in (starts, lens, strands))
    n = starts.size
    order = np.argsort(starts, kind="stable")
    s, e = starts[order], starts[order] + lens[order]
    last = np.searchsorted(s, e - min_ov, side="right")      # partners j > i (sorted) start at or before e_i - min_ov
    cnt = np.maximum(last - (np.arange(n) + 1), 0)
    I = np.repeat(np.arange(n), cnt)
    J = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt) + I + 1
    lo, hi = s[J], np.minimum(e[I], e[J])
    ok = hi - lo >= min_ov
    I, J, lo, hi = I[ok], J[ok], lo[ok], hi[ok]
    ri, rj = order[I], order[J]
    a, b = np.minimum(ri, rj), np.maximum(ri, rj)

    def own(r):
        fwd_lo, fwd_hi = lo - starts[r], hi - starts[r]
        r_lo = np.where(strands[r] == 1, lens[r] - fwd_hi, fwd_lo)
        r_hi = np.where(strands[r] == 1, lens[r] - fwd_lo, fwd_hi)
        if jitter:
            d_lo, d_hi = rng.integers(-jitter, jitter + 1, r_lo.size), rng.integers(-jitter, jitter + 1, r_lo.size)
            n_lo = np.where(r_lo == 0, 0, np.clip(r_lo + d_lo, 1, lens[r] - 2))
            n_hi = np.where(r_hi == lens[r], lens[r], np.clip(r_hi + d_hi, 2, lens[r] - 1))
            bad = n_lo >= n_hi
            r_lo, r_hi = np.where(bad, r_lo, n_lo), np.where(bad, r_hi, n_hi)
        return r_lo, r_hi

    a_lo, a_hi = own(a)
    b_lo, b_hi = own(b)
    o = strands[a] ^ strands[b]
    ends = (a_lo == 0) * 1 | (a_hi == lens[a]) * 2 | (b_lo == 0) * 4 | (b_hi == lens[b]) * 8
    u = np.uint64
    rows = np.stack([(o.astype(u) << u(63)) | ((a + rid_base).astype(u) << u(32)) | (b + rid_base).astype(u), (hi - lo).astype(u), (a_lo.astype(u) << u(32)) | a_hi.astype(u),
                     (b_lo.astype(u) << u(32)) | b_hi.astype(u), ends.astype(u), np.ones(a.size, u)], axis=1)
    return rows[np.lexsort((b, a))]


def random_layout(rng, nreads, genome, len_lo, len_hi):
    """(starts, lens, strands) of reads scattered over a line of `genome` bases"""
    lens = rng.integers(len_lo, len_hi + 1, nreads)
    starts = rng.integers(0, genome - lens + 1)
    return starts, lens, rng.integers(0, 2, nreads)


def neighbour_pairs(starts, lens, contained, min_ov):
    """the pairs {r, r'} of reads that are neighbours among the non-contained reads in the order of the line and share min_ov bases"""
    live = [r for r in np.argsort(starts, kind="stable").tolist() if not contained[r]]
    live.sort(key=lambda r: (starts[r], starts[r] + lens[r]))
    return {(min(p, q), max(p, q)) for p, q in zip(live, live[1:]) if starts[p] + lens[p] - starts[q] >= min_ov}


def row_pairs(rows, rid_base=0):
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 6)
    return [(int((k >> np.uint64(32)) & np.uint64(0x7FFFFFFF)) - rid_base, int(k & np.uint64(0xFFFFFFFF)) - rid_base) for k in rows[:, 0]]
