"""The EXTENSION result by its definition, with no minimizers, supermers or tasks in it: every position of every read with at least K bases
gives one instance (canonical k-mer, read id, position); canonical = min(s, revcomp(s)) as strings after upper-casing and N -> A (what
DnaSeq::compress packs); a k-mer stays if the number of its instances lies in [L, U].  numpy only, keys of any number of words in the layout of
oracle.string_to_words (base i in word i / 32 at bit 2 (31 - i % 32), word 0 first).  It pins the oracle on the inputs of
tests/ragged_inputs.py (tests/test_ext_brute_force.py), and tests/test_gpu_ext_ragged.py holds the GPU's unfiltered lists to it."""
import numpy as np

_CODE = np.zeros(256, dtype=np.uint8)
for _ch, _c in (("C", 1), ("c", 1), ("G", 2), ("g", 2), ("T", 3), ("t", 3)):      # A, a, N, n -> 0
    _CODE[ord(_ch)] = _c


def instances(seqs, K, rid_base=0):
    """(keys uint64 [n, nw], rid int64 [n], pos int64 [n]) of every k-mer instance, in read order"""
    nw = (K + 31) // 32
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    first = np.concatenate(([0], np.cumsum(lens)[:-1])) if len(seqs) else np.zeros(0, np.int64)
    codes = _CODE[np.frombuffer("".join(seqs).encode(), dtype=np.uint8)].astype(np.uint64)
    per = np.maximum(lens - K + 1, 0)
    n = int(per.sum())
    rid = np.repeat(np.arange(len(seqs), dtype=np.int64), per)
    pos = np.arange(n, dtype=np.int64) - np.repeat(np.cumsum(per) - per, per)
    at = np.repeat(first, per) + pos
    fw = np.zeros((n, nw), dtype=np.uint64)
    rc = np.zeros((n, nw), dtype=np.uint64)
    for i in range(K):
        sh = np.uint64(2 * (31 - i % 32))
        fw[:, i // 32] |= codes[at + i] << sh
        rc[:, i // 32] |= (np.uint64(3) - codes[at + (K - 1 - i)]) << sh
    less = np.zeros(n, dtype=bool)                             # rc < fw, word 0 the most significant (= the strings' order)
    same = np.ones(n, dtype=bool)
    for j in range(nw):
        less |= same & (rc[:, j] < fw[:, j])
        same &= rc[:, j] == fw[:, j]
    keys = np.where(less[:, None], rc, fw)
    return keys, rid + int(rid_base), pos


def sort_triples(keys, rid, pos):
    """the rows in ascending (key words from word 0, rid, pos)"""
    keys = np.asarray(keys, dtype=np.uint64)
    keys = keys.reshape(len(rid), keys.shape[-1] if keys.ndim == 2 else 1)
    rid, pos = np.asarray(rid).astype(np.int64), np.asarray(pos).astype(np.int64)
    order = np.lexsort((pos, rid) + tuple(keys[:, j] for j in range(keys.shape[1] - 1, -1, -1)))
    return keys[order], rid[order], pos[order]


def triples(seqs, K, L=1, U=None, rid_base=0):
    """the sorted (keys, rid, pos) of the k-mers with L <= instances <= U (U = None: no upper limit)"""
    return kept(sort_triples(*instances(seqs, K, rid_base)), L, U)


def kept(sorted_rows, L=1, U=None):
    """the filter on sorted rows of ALL instances (sort_triples(*instances(...)): sorted once, filtered as often as needed)"""
    keys, rid, pos = sorted_rows
    n = len(rid)
    if n == 0:
        return keys, rid, pos
    start = np.flatnonzero(np.concatenate(([True], (keys[1:] != keys[:-1]).any(axis=1))))
    size = np.diff(np.concatenate((start, [n])))
    keep = size >= L
    if U is not None:
        keep &= size <= U
    sel = np.repeat(keep, size)
    return keys[sel], rid[sel], pos[sel]


def result_triples(keys, cnt, payload_off, rid, pos):
    """the same rows from a result list (entry i owns cnt[i] payloads from payload_off[i]), sorted alike"""
    cnt = np.asarray(cnt).astype(np.int64)
    po = np.asarray(payload_off).astype(np.int64)[:len(cnt)]
    sel = np.repeat(po - (np.cumsum(cnt) - cnt), cnt) + np.arange(int(cnt.sum()), dtype=np.int64)
    return sort_triples(np.repeat(np.asarray(keys, dtype=np.uint64), cnt, axis=0), np.asarray(rid)[sel], np.asarray(pos)[sel])
