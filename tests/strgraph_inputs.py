"""Overlap rows fabricated arc by arc, for the tests of hsk_overlaps_reduce that need a graph of a given shape and not a layout of reads
on a line: arc_row is the arc table of include/hsk.h read backwards, hub_graph a list with two vertices of more than RD_CHUNK out-arcs
whose every row has a class known by design.  No GPU code here; tests/test_strgraph_inputs.py holds this file to the plain-Python
definition (tests/strgraph_ref.py), tests/test_gpu_overlaps_reduce_hubs.py runs the lists through the kernels."""
import numpy as np

from tests import strgraph_ref as S

CHUNK = 1024                                              # RD_CHUNK of hysortk_amd/csrc/hsk_reduce.h
GRID = 1 << 14                                            # the most workgroups reduce_wave_kernel is launched with
DEG_A, DEG_B = 2 * CHUNK + 37, CHUNK + 1                  # records of out(A) and out(B), dead ones and repeated keys included
POOL_LEN = 1000
HUB_SEED = 5                                              # the list that both test files build


def arc_row(v, w, length, lens, exchanged=False, score=None, rid_base=0, reach=None):
    """The six-word row of which v -> w (`length` bases of v in front of the overlap) is one of the two arcs; the other one is its
    complement w^1 -> v^1.  v = 2 p + s and w = 2 q + s' are oriented reads, lens the lengths of all reads.  The row has a = p, b = q,
    or a = q, b = p with `exchanged`.  reach: how far the overlap goes into q, strictly inside it (default: as far as it goes into p, where
    q is long enough); it is the free coordinate of the row, and lens[q] - reach the length of the complement arc."""
    p, sv, q, sw = v >> 1, v & 1, w >> 1, w & 1
    lp, lq = int(lens[p]), int(lens[q])
    if reach is None:
        reach = min(lp - length, lq - 1)
    if not (p != q and 0 < length < lp and 0 < reach < lq):
        raise ValueError("no dovetail has this arc")
    p_lo, p_hi = (length, lp) if sv == 0 else (0, lp - length)          # a suffix of v: the end of p, or its start if v is the reverse complement
    q_lo, q_hi = (0, reach) if sw == 0 else (lq - reach, lq)            # a prefix of w
    o = sv ^ sw
    if exchanged:
        return S.make_row(q + rid_base, p + rid_base, o, q_lo, q_hi, p_lo, p_hi, lq, lp, score=score)
    return S.make_row(p + rid_base, q + rid_base, o, p_lo, p_hi, q_lo, q_hi, lp, lq, score=score)


def _background(rng, nreads, genome, internal):
    """reads scattered over a line, their exact overlaps with jittered ends, and a few rows that stop inside both reads"""
    starts, lens, strands = S.random_layout(rng, nreads, genome, 200, 300)
    rows = S.layout_rows(starts, lens, strands, 30, jitter=3, rng=rng)
    taken = set(S.row_pairs(rows))
    extra = []
    while len(extra) < internal:
        a, b = sorted(rng.choice(nreads, 2, replace=False).tolist())
        if (a, b) in taken:
            continue
        taken.add((a, b))
        extra.append(S.make_row(a, b, int(rng.integers(0, 2)), 5, int(lens[a]) - 5, 7, int(lens[b]) - 7, int(lens[a]), int(lens[b])))
    return lens, np.concatenate([rows, np.array(extra, dtype=np.uint64).reshape(-1, 6)])


class _Hub:
    """the rows around one vertex h: `entries` are short lists of (row, kind, designed class) whose order among themselves is kept"""

    def __init__(self, rng, lens, fuzz, h, reads):
        self.rng, self.lens, self.fuzz, self.h = rng, lens, fuzz, h
        reads = np.sort(np.asarray(reads))
        self.x = 2 * reads + rng.integers(0, 2, reads.size)             # the targets, sorted: vertex ids follow read ids
        self.L = rng.integers(200, 900, reads.size)
        self.kind = np.array(["none", "exact", "over"])[rng.integers(0, 3, reads.size)]
        self.special = np.zeros(reads.size, bool)                       # targets with a second record: never the w of a designed witness
        self.entries, self.losers = [], []

    def row(self, v, w, length, exchanged=None, score=None):
        exchanged = bool(self.rng.integers(0, 2)) if exchanged is None else exchanged
        return arc_row(int(v), int(w), int(length), self.lens, exchanged=exchanged, score=score, reach=int(self.rng.integers(100, 200))), exchanged

    def witness(self, j, total, room=1):
        """(i, l2): a target i without a second record and the length of x_i -> x_j with L_i + l2 == total; l2 >= room"""
        ok = np.flatnonzero(~self.special & (self.L <= total - room) & (np.arange(self.L.size) != j))
        i = int(self.rng.choice(ok))
        return i, int(total - self.L[i])

    def plain(self, j):
        """target j with one record: no witness (KEPT), a witness at exactly L + fuzz (REDUCED) or one base too long (KEPT)"""
        kind = str(self.kind[j])
        self.entries.append([(self.row(self.h, self.x[j], self.L[j])[0], kind, S.REDUCED if kind == "exact" else S.KEPT)])
        if kind != "none":
            i, l2 = self.witness(j, self.L[j] + self.fuzz + (kind == "over"))
            self.entries.append([(self.row(self.x[i], self.x[j], l2)[0], "witness", S.KEPT)])

    def pair(self, variant, winner, loser):
        """[winner, loser] in the order and with the scores of one of three variants: the larger score at the larger index, equal
        scores (the lower index stays), the larger score at the lower index"""
        (wrow, wkind, wcls), (lrow, lkind) = winner, loser
        wrow, lrow = list(wrow), list(lrow)
        wrow[1], lrow[1] = 500, (495, 500, 495)[variant % 3]
        w, l = (wrow, wkind, wcls), (lrow, lkind, S.DUPLICATE)
        entry = [l, w] if variant % 3 == 0 else [w, l]
        self.entries.append(entry)
        return entry.index(w), entry.index(l)

    def loser_target(self, j, variant):
        """h -> x_j twice with equal (key, ends): the loser's arc is much longer and has an exact witness, the winner has none"""
        far = int(self.L[j] + self.rng.integers(50, 100))
        win, ex = self.row(self.h, self.x[j], self.L[j])
        lose, _ = self.row(self.h, self.x[j], far, exchanged=ex)
        iw, il = self.pair(variant, (win, "none", S.KEPT), (lose, "dup_target"))
        e = len(self.entries) - 1
        self.losers.append(dict(kind="dup_target", loser=(e, il), winner=(e, iw), then={(e, il): S.REDUCED, (e, iw): S.DUPLICATE}))
        i, l2 = self.witness(j, far + self.fuzz)
        self.entries.append([(self.row(self.x[i], self.x[j], l2)[0], "witness", S.KEPT)])

    def loser_witness(self, j, variant):
        """target j with a witness one base too long, and a copy of that witness row that is short enough and loses"""
        self.entries.append([(self.row(self.h, self.x[j], self.L[j])[0], "over", S.KEPT)])
        t = len(self.entries) - 1
        i, l2 = self.witness(j, self.L[j] + self.fuzz + 1, room=31)
        win, ex = self.row(self.x[i], self.x[j], l2)
        lose, _ = self.row(self.x[i], self.x[j], l2 - int(self.rng.integers(1, 30)), exchanged=ex)
        iw, il = self.pair(variant, (win, "witness", S.KEPT), (lose, "dup_witness"))
        e = len(self.entries) - 1
        self.losers.append(dict(kind="dup_witness", loser=(e, il), winner=(e, iw), then={(e, il): S.KEPT, (e, iw): S.DUPLICATE, (t, 0): S.REDUCED}))

    def edge(self, j, original_long, second):
        """Target j with two records of one key, laid across a chunk edge by the caller's choice of j: arcs of L and L + 40 and one witness
        that explains the longer arc exactly and the shorter not at all.  second "exchanged": the second row has a and b the other way
        round, both rows are live; "copy": it is a copy that loses (the longer arc, so the witness explains a dead record only)."""
        short, far = int(self.L[j]), int(self.L[j]) + 40
        one, _ = self.row(self.h, self.x[j], far if original_long else short, exchanged=False)
        if second == "exchanged":
            two, _ = self.row(self.h, self.x[j], short if original_long else far, exchanged=True)
            a, b = ("edge_long", S.REDUCED), ("edge_short", S.KEPT)
            self.entries.append([(one,) + (a if original_long else b), (two,) + (b if original_long else a)])
        else:
            two, _ = self.row(self.h, self.x[j], far, exchanged=False)
            one, two = list(one), list(two)
            one[1], two[1] = 500, 495
            self.entries.append([(one, "edge_short", S.KEPT), (two, "edge_dup", S.DUPLICATE)])
            e = len(self.entries) - 1
            self.losers.append(dict(kind="edge_dup", loser=(e, 1), winner=(e, 0), then={(e, 1): S.REDUCED, (e, 0): S.DUPLICATE}))
        i, l2 = self.witness(j, far + self.fuzz)
        self.entries.append([(self.row(self.x[i], self.x[j], l2)[0], "witness", S.KEPT)])


def hub_graph(rng, background=9000, genome=450000, fuzz=S.DEFAULT_FUZZ, dup_targets=40, dup_witnesses=40):
    """(rows, lens, plan): a background of `background` reads laid on a line (coverage about 5, ends jittered by 3 bases, every class
    0 - 5), and behind it a pool of reads of POOL_LEN bases that no background row names.  Pool read 0 is hub A: one of its vertices has
    DEG_A = 2 * CHUNK + 37 records to distinct pool reads, three chunks of the wave path.  Pool read 8192 is hub B, same strand, DEG_B =
    CHUNK + 1 records: its vertex is GRID behind A's, so the workgroup that treats A treats B next.  Every target x_j of a hub has a
    random length L_j in [200, 900) and one of three designs: no witness (KEPT), one row x_i -> x_j with L_i + l2 == L_j + fuzz (REDUCED),
    one with L_i + l2 == L_j + fuzz + 1 (KEPT).  Strands and the order of a and b are random, so every branch of the arc table feeds a
    hub.  On hub A, behind rank 1100 of its sorted run: copies that lose against a row of equal (key, ends) -- as a target whose much
    longer arc has an exact witness, and as a witness that would be short enough -- under all three score orders.  Across A's chunk edges
    (records 1023 | 1024 and 2047 | 2048) lie two exchanged rows of one arc with a witness for the longer of them only, across B's edge a
    row and its losing copy.  The complement arcs never reduce anything: every overlap reaches less than 200 bases into its target.

    plan: fuzz, hub_a / hub_b (the vertices), index / cls / kind (one entry per designed row: its index in rows, its designed class and
    what it is), on_a (the row belongs to hub A), edges ((hub vertex, target vertex, first position in the sorted out(hub))), losers
    (loser and winner as row indices, and `then`: row index -> class once the loser's score is raised above the winner's)."""
    lens_bg, rows_bg = _background(rng, background, genome, 60)
    nreads = background + GRID // 2 + 1
    lens = np.concatenate([lens_bg, np.full(nreads - background, POOL_LEN)])
    s = int(rng.integers(0, 2))
    pool = rng.permutation(np.arange(background + 1, background + GRID // 2))
    n_a, n_b = DEG_A - 2 - dup_targets, DEG_B - 1
    A = _Hub(rng, lens, fuzz, 2 * background + s, pool[:n_a])
    B = _Hub(rng, lens, fuzz, 2 * (background + GRID // 2) + s, pool[n_a:n_a + n_b])

    # hub A: the run's positions.  One record per target below rank 1023; that target has two; 30 of the copies that lose as a target
    # lie between it and the second edge's target, whose first record is therefore number 2047, and 10 behind it.
    e1, below = CHUNK - 1, dup_targets * 3 // 4
    e2 = 2 * CHUNK - 1 - 1 - below
    dt = np.concatenate([rng.choice(np.arange(1101, e2), below, replace=False), rng.choice(np.arange(e2 + 1, n_a - 1), dup_targets - below, replace=False)])
    A.special[[e1, e2]] = True
    A.special[dt] = True
    A.kind[dt] = "none"
    A.kind[n_a - 1] = "exact"                             # the last record of the run: the largest target of the last chunk
    over = np.flatnonzero((A.kind == "over") & ~A.special & (np.arange(n_a) > 1100) & (A.L >= 300))      # (room for a witness that can lose 30 bases)
    dw = rng.choice(over, dup_witnesses, replace=False)
    for j in range(n_a):
        if j == e1 or j == e2:
            A.edge(j, original_long=(j == e2), second="exchanged")
        elif j in dt:
            A.loser_target(j, int(np.flatnonzero(dt == j)[0]))
        elif j in dw:
            A.loser_witness(j, int(np.flatnonzero(dw == j)[0]))
        else:
            A.plain(j)
    B.special[n_b - 1] = True
    for j in range(n_b):
        if j == n_b - 1:
            B.edge(j, original_long=False, second="copy")
        else:
            B.plain(j)

    # the designed rows in a random order of their entries, behind the background
    rows, index, cls, kind, on_a, where = [], [], [], [], [], {}
    units = [(hub, e) for hub in (A, B) for e in range(len(hub.entries))]
    for u in rng.permutation(len(units)):
        hub, e = units[u]
        for k, (row, what, c) in enumerate(hub.entries[e]):
            where[(id(hub), e, k)] = rows_bg.shape[0] + len(rows)
            index.append(rows_bg.shape[0] + len(rows)); cls.append(c); kind.append(what); on_a.append(hub is A)
            rows.append(row)
    losers = []
    for hub in (A, B):
        for l in hub.losers:
            at = lambda ek: where[(id(hub), ek[0], ek[1])]
            losers.append(dict(kind=l["kind"], loser=at(l["loser"]), winner=at(l["winner"]), then={at(ek): c for ek, c in l["then"].items()}))
    plan = dict(fuzz=fuzz, hub_a=A.h, hub_b=B.h, index=np.array(index), cls=np.array(cls, dtype=np.uint8), kind=np.array(kind), on_a=np.array(on_a), losers=losers,
                edges=[(A.h, int(A.x[e1]), CHUNK - 1), (A.h, int(A.x[e2]), 2 * CHUNK - 1), (B.h, int(B.x[n_b - 1]), CHUNK - 1)])
    return np.concatenate([rows_bg, np.array(rows, dtype=np.uint64)]), lens, plan


def raise_losers(rows, plan):
    """the list with every designed loser's score above its winner's, and the classes the designed rows then have"""
    out = np.array(rows, dtype=np.uint64)
    cls = dict(zip(plan["index"].tolist(), plan["cls"].tolist()))
    for l in plan["losers"]:
        out[l["loser"], 1] = out[l["winner"], 1] + np.uint64(7)
        cls.update(l["then"])
    return out, np.array([cls[i] for i in plan["index"].tolist()], dtype=np.uint8)


def huge_case():
    """(rows, lens, {fuzz: classes}): five reads of 2^32 - 1 bases and two triangles v -> w -> x, v -> x with short arcs of 3e9 and a
    long arc of 2e9.  The sum 6e9 needs 33 bits: kept in 32 it is 1 705 032 704 and would explain the long arc at fuzz 10; at fuzz
    2^32 - 1 the bound L + fuzz is 6 294 967 295 and the long arc is explained, kept in 32 bits it is 1 999 999 999 and it would not be.
    The first triangle is on the forward strands of reads 0, 1, 2, a before b; the second on the reverse complements of reads 3, 4, 1,
    two of its rows exchanged."""
    top = 0xFFFFFFFF
    lens = np.full(5, top, dtype=np.uint64)
    short, far = 3_000_000_000, 2_000_000_000
    rows = [arc_row(0, 2, short, lens, reach=1000), arc_row(2, 4, short, lens, reach=1000), arc_row(0, 4, far, lens, reach=1000),
            arc_row(7, 9, short, lens, exchanged=True, reach=1000), arc_row(9, 3, short, lens, reach=1000), arc_row(7, 3, far, lens, exchanged=True, reach=1000)]
    K, R = S.KEPT, S.REDUCED
    return np.array(rows, dtype=np.uint64), lens, {10: [K, K, K, K, K, K], top: [K, K, R, K, K, R]}


def tile_rows(rng, n, reads=300, genome=15000, edges=(1022, 1023, 1024, 2047, 2048)):
    """(rows, lens) with exactly n rows: the overlaps of `reads` reads laid on a line (ends jittered by 3 bases), repeated on fresh reads
    until there are n rows and cut there, and ordered so that the rows on both sides of the edges of the 1024-row tiles (`edges`, where n
    reaches that far) are dovetails between live reads -- rows that give arcs and are kept or reduced, not rows that drop out early."""
    starts, lens, strands = S.random_layout(rng, reads, genome, 200, 300)
    one = S.layout_rows(starts, lens, strands, 30, jitter=3, rng=rng)
    copies = -(-n // one.shape[0])
    rows = np.concatenate([S.layout_rows(starts, lens, strands, 30, jitter=3, rng=rng, rid_base=k * reads) for k in range(copies)])[:n]
    lens = np.tile(lens, copies)
    cls = S.reduce_rows(rows, lens)["row_class"]
    live = [int(i) for i in np.flatnonzero(cls <= S.REDUCED) if int(i) not in edges]
    for e in edges:
        if e < n and cls[e] > S.REDUCED:                  # (a permutation of the rows permutes their classes: no two rows here have one key)
            j = min(live, key=lambda i: abs(i - e))
            live.remove(j)
            rows[[e, j]] = rows[[j, e]]
    return rows, lens
