"""The strand of a k-mer occurrence and the read pairs split by relative strand, by their definitions (include/hsk.h: hsk_result_strands,
hsk_result_pairs_oriented), in numpy on the CPU oracle's EXTENSION result.  The strand of an oracle payload (rid, pos) is 1 iff the read's K
bases at pos -- upper-cased, N read as A -- differ from the entry's k-mer; the oriented rows are the rows of tests/test_gpu_pairs.py's
reference() with o << 63 OR-ed into the key before grouping.  Everything is integers."""
import numpy as np

from tests.test_gpu_pairs import _triu

U32 = np.uint64(0xFFFFFFFF)
_CODE = np.zeros(256, dtype=np.uint8)                     # A / N / anything else -> 0 (the tests' reads hold ACGTN only)
for _ch, _c in (("C", 1), ("G", 2), ("T", 3)):
    _CODE[ord(_ch)] = _CODE[ord(_ch.lower())] = _c


def entry_codes(keys, K):
    """[n, K] base codes of the entries' k-mers (base i in word i / 32 at shift 2 (31 - i % 32))."""
    keys = np.asarray(keys, dtype=np.uint64)
    cols = [((keys[:, j // 32] >> np.uint64(2 * (31 - j % 32))) & np.uint64(3)).astype(np.uint8) for j in range(K)]
    return np.stack(cols, axis=1) if keys.shape[0] else np.zeros((0, K), np.uint8)


def payload_strands(o, seqs, K, rid_base):
    """(strand per oracle payload index -- False where no entry owns the index --, owner mask, palindrome mask): numpy bool arrays of len(o.pos)."""
    codes = [_CODE[np.frombuffer(s.encode(), dtype=np.uint8)] for s in seqs]
    start = np.concatenate([[0], np.cumsum([c.size for c in codes])]).astype(np.int64)
    flat = np.concatenate(codes) if codes else np.zeros(0, np.uint8)
    P = int(o.pos.size)
    strand, owned, pal = np.zeros(P, bool), np.zeros(P, bool), np.zeros(P, bool)
    cnt = o.cnt.astype(np.int64)
    if not cnt.size:
        return strand, owned, pal
    slot = np.repeat(o.payoff[:-1].astype(np.int64), cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    ent = np.repeat(np.arange(cnt.size), cnt)
    r = o.rid[slot].astype(np.int64) - rid_base
    assert r.min() >= 0 and r.max() < len(seqs)
    p = o.pos[slot].astype(np.int64)
    assert np.all(p + K <= (start[r + 1] - start[r]))
    bases = flat[(start[r] + p)[:, None] + np.arange(K)[None, :]]
    ec = entry_codes(o.keys, K)
    fwd = np.all(bases == ec[ent], axis=1)
    rev = np.all((3 - bases[:, ::-1]) == ec[ent], axis=1)
    assert np.all(fwd | rev), "the oracle's payload does not spell its entry"
    strand[slot], owned[slot], pal[slot] = ~fwd, True, fwd & rev
    return strand, owned, pal


def strand_lookup(o, seqs, K, rid_base):
    """Sorted keys rid << 32 | pos of the owned oracle payloads and their strands: what a device slot's (rid, pos) is looked up in."""
    strand, owned, pal = payload_strands(o, seqs, K, rid_base)
    key = ((o.rid.astype(np.int64).astype(np.uint64) & U32) << np.uint64(32)) | o.pos.astype(np.uint64)
    key, st = key[owned], strand[owned]
    order = np.argsort(key, kind="stable")
    key, st = key[order], st[order]
    assert np.all(key[1:] != key[:-1])                    # a position of a read holds one k-mer
    return key, st, int(owned.sum()), int(strand.sum()), int(pal.sum())


def task_bits(fetched, lookup):
    """The bits hsk_result_strands must give for a task, from the task's own arrays (DeviceResult.fetch: the order of the payload inside an entry is
    the device's) and strand_lookup: (bool array of npay, number of gap slots)."""
    key, st = lookup[0], lookup[1]
    npay = int(fetched["npay"])
    bits, owned = np.zeros(npay, bool), np.zeros(npay, bool)
    cnt = fetched["cnt"].astype(np.int64)
    if cnt.size:
        first = fetched["payload_off"].astype(np.int64) - int(fetched["payload_base"])
        slot = np.repeat(first, cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        k = ((fetched["rid"][slot].astype(np.int64).astype(np.uint64) & U32) << np.uint64(32)) | fetched["pos"][slot].astype(np.uint64)
        at = np.searchsorted(key, k)
        assert np.all(at < key.size) and np.all(key[np.minimum(at, key.size - 1)] == k), "a device payload the oracle does not have"
        bits[slot], owned[slot] = st[at], True
    return bits, int((~owned).sum())


def oriented_reference(o, strand, task_lo=0, task_hi=None, min_shared=1):
    """reference() of tests/test_gpu_pairs.py with the relative strand in bit 63 of the key: (rows [n, 4] uint64, records, self_records, keys).
    strand: payload_strands(...)[0]."""
    nt = len(o.task_off) - 1
    a, b = int(o.task_off[task_lo]), int(o.task_off[nt if task_hi is None else task_hi])
    cnt = o.cnt[a:b].astype(np.int64)
    rid = o.rid.astype(np.int64).astype(np.uint64) & U32
    pos = o.pos.astype(np.uint64)
    sb = strand.astype(np.uint64)
    ks, vs, records = [], [], 0
    for e in a + np.flatnonzero(cnt >= 2):
        c, p0 = int(o.cnt[e]), int(o.payoff[e])
        i, j = _triu(c)
        ra, rb, pa, pb = rid[p0 + i], rid[p0 + j], pos[p0 + i], pos[p0 + j]
        orient = sb[p0 + i] ^ sb[p0 + j]
        sw = ra > rb
        ra, rb, pa, pb = np.where(sw, rb, ra), np.where(sw, ra, rb), np.where(sw, pb, pa), np.where(sw, pa, pb)
        keep = ra != rb
        records += i.size
        ks.append(((orient << np.uint64(63)) | (ra << np.uint64(32)) | rb)[keep]); vs.append(((pa << np.uint64(32)) | pb)[keep])
    k = np.concatenate(ks) if ks else np.zeros(0, np.uint64)
    v = np.concatenate(vs) if vs else np.zeros(0, np.uint64)
    order = np.lexsort((v, k))
    k, v = k[order], v[order]
    uk, start, shared = np.unique(k, return_index=True, return_counts=True)
    rows = np.stack([uk, shared.astype(np.uint64), v[start], v[start + shared - 1]], axis=1) if uk.size else np.zeros((0, 4), np.uint64)
    return rows[rows[:, 1] >= np.uint64(min_shared)], records, records - int(k.size), int(uk.size)
