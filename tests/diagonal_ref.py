"""The oriented read pairs by diagonal, by their definition (include/hsk.h: hsk_result_pair_diagonals), in numpy on the CPU oracle's EXTENSION
result.  The records are those of tests/oriented_ref.py's oriented_reference() -- key o << 63 | rid_a << 32 | rid_b, value pos_a << 32 |
pos_b, pairs inside one read dropped and counted -- with their values kept; every record gets D = pos_a - pos_b + 2^32 (o = 0) or
pos_a + pos_b (o = 1) and the bin D // W, and the records are grouped by (key, bin).  Everything is integers and compared exactly."""
import numpy as np

from tests.test_gpu_pairs import _triu

U32 = np.uint64(0xFFFFFFFF)
BIAS = 1 << 32


def records(o, strand, task_lo=0, task_hi=None):
    """(keys, values, records, self_records): the records of the task range as oriented_reference() takes them, unsorted; `records` counts
    the same-read pairs too."""
    nt = len(o.task_off) - 1
    a, b = int(o.task_off[task_lo]), int(o.task_off[nt if task_hi is None else task_hi])
    cnt = o.cnt[a:b].astype(np.int64)
    rid = o.rid.astype(np.int64).astype(np.uint64) & U32
    pos = o.pos.astype(np.uint64)
    sb = strand.astype(np.uint64)
    ks, vs, total = [], [], 0
    ent = a + np.flatnonzero(cnt >= 2)
    for c in np.unique(o.cnt[ent]):                       # all entries of one count at a time: the same (i, j) for each of them
        p0 = o.payoff[ent[o.cnt[ent] == c]].astype(np.int64)[:, None]
        i, j = _triu(int(c))
        si, sj = (p0 + i[None, :]).ravel(), (p0 + j[None, :]).ravel()
        ra, rb, pa, pb = rid[si], rid[sj], pos[si], pos[sj]
        orient = sb[si] ^ sb[sj]
        sw = ra > rb
        ra, rb, pa, pb = np.where(sw, rb, ra), np.where(sw, ra, rb), np.where(sw, pb, pa), np.where(sw, pa, pb)
        keep = ra != rb
        total += si.size
        ks.append(((orient << np.uint64(63)) | (ra << np.uint64(32)) | rb)[keep]); vs.append(((pa << np.uint64(32)) | pb)[keep])
    k = np.concatenate(ks) if ks else np.zeros(0, np.uint64)
    v = np.concatenate(vs) if vs else np.zeros(0, np.uint64)
    return k, v, total, total - int(k.size)


def bins_of(k, v, W):
    """The bin of every record (uint64)."""
    pa, pb = (v >> np.uint64(32)).astype(np.int64), (v & U32).astype(np.int64)
    D = np.where((k >> np.uint64(63)) != 0, pa + pb, pa - pb + BIAS)
    assert np.all(D >= 0)
    return (D // int(W)).astype(np.uint64)


def select(allb, min_support=1):
    """The list by best bin from the all-bins rows (ascending (key, bin), min_support = 1): a plain loop over the keys."""
    out = []
    if allb.shape[0]:
        start = np.flatnonzero(np.concatenate([[True], allb[1:, 0] != allb[:-1, 0]]))
        for s, e in zip(start, np.concatenate([start[1:], [allb.shape[0]]])):
            grp = allb[s:e]
            best = 0
            for q in range(1, grp.shape[0]):              # larger support; the rows are in ascending bin, so a later equal support loses
                if int(grp[q, 3]) > int(grp[best, 3]):
                    best = q
            row = grp[best].copy()
            row[1] = grp[:, 3].sum(dtype=np.uint64)
            if int(row[3]) >= min_support:
                out.append(row)
    return np.array(out, dtype=np.uint64).reshape(-1, 6)


def diagonal_reference(o, strand, W, task_lo=0, task_hi=None, min_support=1, recs=None):
    """dict: all_bins ([n, 6] uint64 { key, support, bin, support, first, last } in ascending (key, bin), rows below min_support dropped),
    best ([m, 6] { key, shared, bin, support, first, last } in ascending key, min_support applied after the selection), records,
    self_records, keys, bins (both before min_support)."""
    k, v, total, self_records = recs if recs is not None else records(o, strand, task_lo, task_hi)      # (recs: records() of the same range, computed once)
    b = bins_of(k, v, W)
    order = np.lexsort((v, b, k))
    k, v, b = k[order], v[order], b[order]
    if k.size:
        new = np.concatenate([[True], (k[1:] != k[:-1]) | (b[1:] != b[:-1])])
        start = np.flatnonzero(new)
        end = np.concatenate([start[1:], [k.size]])
        sup = (end - start).astype(np.uint64)
        allb = np.stack([k[start], sup, b[start], sup, v[start], v[end - 1]], axis=1)
    else:
        allb = np.zeros((0, 6), np.uint64)
    return dict(all_bins=allb[allb[:, 3] >= np.uint64(min_support)], best=select(allb, min_support), records=total, self_records=self_records,
                keys=int(np.unique(k).size), bins=int(allb.shape[0]))
