"""The definition of hsk_overlaps_unitigs (include/hsk.h) in plain Python: the out-arcs of every vertex, the links, and the chains walked
one link at a time, with dictionaries and lists and nothing clever -- what the kernels and the shared header
(hysortk_amd/csrc/hsk_unitig.h) are held to.  tests/test_unitig_ref.py holds this file to layouts typed out by hand.  ring_rows makes the
edges of reads laid around a circle, next to strgraph_ref.layout_rows for reads on a line."""
import numpy as np

from tests import strgraph_ref as S

NO_LINK = (1 << 64) - 1
COUNTS = ("unitigs", "members", "singletons", "circular", "longest", "links", "branch_vertices", "live_reads", "input_rows", "arcs")


def unitigs(rows, lens, contained=None, rid_base=0):
    """dict: layout ([members, 4] uint64), table ([unitigs, 4] uint64), info (the counts of the call, without rounds and times)"""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 6)
    n, nreads = rows.shape[0], len(lens)
    contained = [False] * nreads if contained is None else [bool(x) for x in contained]
    F = [S.fields(r, lens, rid_base) for r in rows]       # (raises for a read outside the reads and for lengths that disagree)
    bad = sum(1 for f in F if S.own_class(f) != S.KEPT)
    if bad:
        raise ValueError("%d of %d rows are no dovetails: this is not a list of string graph edges" % (bad, n))
    bad = sum(1 for f in F if contained[f["a"]] or contained[f["b"]])
    if bad:
        raise ValueError("%d of %d rows name a read whose contained bit is set" % (bad, n))
    rep = {}                                              # (v, w) -> (len, row) of the arc's representative
    for i, f in enumerate(F):
        for v, w, ln in S.row_arcs(f):
            rep[(v, w)] = min(rep.get((v, w), (ln, i)), (ln, i))
    out = {}
    for v, w in rep:
        out.setdefault(v, set()).add(w)
    deg = lambda v: len(out.get(v, ()))
    succ, pred = {}, {}
    for v, ws in out.items():
        if len(ws) == 1:
            w = next(iter(ws))
            if deg(w ^ 1) == 1:
                succ[v], pred[w] = w, v
    live = [2 * r + s for r in range(nreads) if not contained[r] for s in (0, 1)]
    seen, chains = set(), []
    for v in live:                                        # in increasing order: the first vertex not seen is the smallest of its pair of chains
        if v in seen:
            continue
        assert v % 2 == 0
        h, circular = v, False
        while h in pred:
            h = pred[h]
            if h == v:
                circular = True
                break
        chain, x = [h], h
        while x in succ and succ[x] != h:
            x = succ[x]
            chain.append(x)
        for x in chain:
            assert x not in seen and x ^ 1 not in seen
            seen.add(x)
            seen.add(x ^ 1)
        chains.append((h, circular, chain))
    chains.sort()
    layout, table = [], []
    for u, (h, circular, chain) in enumerate(chains):
        first, offset = len(layout), 0
        for rank, x in enumerate(chain):
            link = NO_LINK
            if x in succ:
                ln, row = rep[(x, succ[x])]
                link = ln << 32 | row
            layout.append([u << 32 | rank, ((x >> 1) + rid_base) << 1 | (x & 1), offset, link])
            if x in succ:
                offset += ln
        last = chain[-1]
        bases = offset if circular else layout[-1][2] + int(lens[last >> 1])
        table.append([first, len(chain), bases, 1 if circular else 0])
    sizes = [t[1] for t in table]
    info = dict(unitigs=len(table), members=len(layout), singletons=sum(1 for s in sizes if s == 1), circular=sum(t[3] for t in table), longest=max(sizes, default=0),
                links=len(succ), branch_vertices=sum(1 for v in live if deg(v) > 1), live_reads=len(live) // 2, input_rows=n, arcs=len(rep))
    return dict(layout=np.array(layout, dtype=np.uint64).reshape(-1, 4), table=np.array(table, dtype=np.uint64).reshape(-1, 4), info=info)


def ring_rows(n, strands, L, step, rid_base=0):
    """The edges of n reads of L bases laid around a circle of n * step bases, read r at r * step and stored reversed if strands[r]: one
    exact dovetail row per neighbouring pair (r, r + 1 mod n), of L - step shared bases, a = the smaller index.  [n, 6] uint64, in the
    order of r (a ring of 2 has two rows of the same two reads, a ring of 1 would be a SELF row: n >= 2)."""
    assert n >= 2 and 0 < step < L
    rows = []
    for i in range(n):
        j = (i + 1) % n
        lo, hi = min(i, j), max(i, j)
        r = S.layout_rows([0, step] if i == lo else [step, 0], [L, L], [strands[lo], strands[hi]], 1)[0].copy()
        o = int(r[0]) >> 63
        r[0] = np.uint64(o << 63 | (lo + rid_base) << 32 | (hi + rid_base))
        rows.append(r)
    return np.array(rows, dtype=np.uint64).reshape(-1, 6)


def line_runs(starts, lens, contained, min_ov):
    """the closed form on an exact layout without stray rows: the maximal runs of live reads, in the order of the line, in which every
    two neighbours share min_ov bases (strgraph_ref.neighbour_pairs); one list of reads per run"""
    live = [r for r in np.argsort(starts, kind="stable").tolist() if not contained[r]]
    live.sort(key=lambda r: (starts[r], starts[r] + lens[r]))
    pairs = S.neighbour_pairs(starts, lens, contained, min_ov)
    runs = []
    for p in live:
        if runs and (min(runs[-1][-1], p), max(runs[-1][-1], p)) in pairs:
            runs[-1].append(p)
        else:
            runs.append([p])
    return runs
