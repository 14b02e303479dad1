"""One comparison for every EXTENSION result list of the GPU tests: all entries and all payloads against the oracle's, never a sample."""
import collections

import numpy as np

Want = collections.namedtuple("Want", "task_off keys cnt hist triples total_kmers")


def entry_triples(cnt, payload_off, rid, pos):
    """(entry, rid, pos) of every payload of a list, each an array, in ascending order: the payload SETS (the order inside one entry is free)"""
    cnt = np.asarray(cnt).astype(np.int64)
    po = np.asarray(payload_off).astype(np.int64)[:len(cnt)]
    sel = np.repeat(po - (np.cumsum(cnt) - cnt), cnt) + np.arange(int(cnt.sum()), dtype=np.int64)
    entry = np.repeat(np.arange(len(cnt), dtype=np.int64), cnt)
    r, p = np.asarray(rid)[sel].astype(np.int64), np.asarray(pos)[sel].astype(np.int64)
    order = np.lexsort(((r << 32) | p, entry))                # (0 <= rid < 2^31, pos < 2^32: one 63-bit key per payload)
    return entry[order].astype(np.int32), r[order], p[order].astype(np.uint32)


def oracle_want(ores):
    from oracle import hsk_oracle as O
    return Want(ores.task_off, ores.keys, ores.cnt, O.histogram_text(ores.cnt), entry_triples(ores.cnt, ores.payoff, ores.rid, ores.pos), ores.stats["total_kmers"])


def assert_list_equals(res, want, tag=None):
    """every entry of an EXTENSION result (KmerList, or anything with its arrays) against `want` (oracle_want)"""
    import hysortk_amd as H
    assert np.array_equal(res.task_off, want.task_off), tag
    assert res.kmers.shape == want.keys.shape and np.array_equal(res.kmers, want.keys), tag
    assert np.array_equal(res.cnt, want.cnt), tag
    if res.histo is not None:
        assert H.histogram_text(res.histo) == want.hist, tag
    n = len(res.cnt)
    if n == 0 and res.payload_off is None:                   # (an empty list comes back without payload arrays)
        return
    cnt, po =res.cnt.astype(np.int64), res.payload_off.astype(np.int64)[:n]
    assert len(res.pos) == len(res.rid) and (po >= 0).all() and (po + cnt <= len(res.pos)).all(), tag       # every range inside the arrays ...
    order = np.argsort(po, kind="stable")
    order = order[cnt[order] > 0]
    assert (po[order][1:] >= (po + cnt)[order][:-1]).all(), tag                                              # ... and no two of them share a slot
    got = entry_triples(res.cnt, res.payload_off, res.rid, res.pos)
    for g, w, what in zip(got, want.triples, ("entry", "rid", "pos")):
        assert g.shape == w.shape, (tag, what)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (tag, what, "%d of %d payloads differ; the first: entry %d, (rid, pos) = (%d, %d), the oracle's (%d, %d)" % (
            bad.size, g.size, got[0][bad[0]], got[1][bad[0]], got[2][bad[0]], want.triples[1][bad[0]], want.triples[2][bad[0]]))
