"""Host-side mirror of the reference's public interface (include/hysortk.hpp:10-16) on top of the
C ABI of libhsk.so.  Same names, argument meaning and error behaviour as the reference:

    read_dna_buffer(fasta_fname, comm)        reference src/hysortk.cpp:18-33
    kmer_count(mydna, comm)                   reference src/hysortk.cpp:36-96
    print_kmer_histogram(kmerlist, comm)      reference src/hysortk.cpp:98-136
    write_output_file(kmerlist, outdir, comm) reference src/hysortk.cpp:138-164
    DnaBuffer / DnaSeq                        reference include/dnabuffer.hpp:14, include/dnaseq.hpp:33
    KmerList (= KmerListS)                    reference include/kmer.hpp:368-410

The reference's compile-time macros (KMER_SIZE, MINIMIZER_SIZE, LOWER/UPPER_KMER_FREQ, EXTENSION,
Makefile:1-46) are keyword arguments with the Makefile's defaults.  `comm` is a torch.distributed
process group wrapper (hysortk_amd.dist.Comm) or None for one process; every function is
collective over it, like the reference over its MPI_Comm.  All computation happens in libhsk.so
on the GPU; this module only moves buffers and formats text.
"""
import ctypes as C
import os
import sys

import numpy as np

from . import _lib

# reference include/dnaseq.hpp:138-157: A/a/N/n -> 0, C/c -> 1, G/g -> 2, T/t -> 3, other -> 4
_CODETAB = np.full(256, 4, dtype=np.uint8)
for _ch, _c in (("A", 0), ("a", 0), ("N", 0), ("n", 0), ("C", 1), ("c", 1), ("G", 2), ("g", 2), ("T", 3), ("t", 3)):
    _CODETAB[ord(_ch)] = _c


class HskError(RuntimeError):
    """Raised where the reference throws std::runtime_error / aborts."""

    def __init__(self, status, detail=""):
        self.status = status
        msg = _lib.load().hsk_strerror(status).decode()
        super().__init__(msg + (": " + detail if detail else ""))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


_PINNED = {}


def pinned_empty(n, dtype=np.uint8):
    """numpy array of n elements in pinned host memory (hsk_host_alloc): a DnaBuffer held in such arrays is read by the GPU
    in place (hsk_count's zero-copy ingest).  Release with pinned_free()."""
    dt = np.dtype(dtype)
    nbytes = max(int(n) * dt.itemsize, 1)
    p = _lib.load().hsk_host_alloc(nbytes)
    if not p:
        raise MemoryError("hsk_host_alloc(%d) failed" % nbytes)
    arr = np.frombuffer((C.c_uint8 * nbytes).from_address(p), dtype=dt, count=int(n))
    _PINNED[arr.ctypes.data] = p
    return arr


def pinned_free(arr):
    p = _PINNED.pop(arr.ctypes.data, None)
    if p:
        _lib.load().hsk_host_free(p)


def pack_sequence(seq):
    """2-bit packs one read exactly like DnaSeq::compress (reference src/dnaseq.cpp:9-31): base i in
    byte i/4 at shift 6-2*(i%4); tail bits zero; a non-ACGTN byte yields code 4 whose shifted value
    (truncated to 8 bits) is OR-ed in, as in the reference."""
    raw = np.frombuffer(seq.encode() if isinstance(seq, str) else bytes(seq), dtype=np.uint8)
    n = raw.size
    nb = (n + 3) // 4
    codes = np.zeros(nb * 4, dtype=np.uint16)
    codes[:n] = _CODETAB[raw]
    codes = codes.reshape(nb, 4)
    sh = np.array([6, 4, 2, 0], dtype=np.uint16)
    return (np.bitwise_or.reduce((codes << sh) & 0xFF, axis=1)).astype(np.uint8)


class DnaSeq:
    """Non-owning view of one packed read (reference include/dnaseq.hpp:33)."""

    def __init__(self, length, mem):
        self._len, self._mem = int(length), mem

    def size(self):
        return self._len

    def numbytes(self):
        return (self._len + 3) // 4

    def data(self):
        return self._mem

    def __getitem__(self, i):
        return int(self._mem[i // 4] >> (6 - 2 * (i % 4))) & 3

    def ascii(self):
        b = np.asarray(self._mem[: self.numbytes()], dtype=np.uint8)
        codes = np.stack([(b >> 6) & 3, (b >> 4) & 3, (b >> 2) & 3, b & 3], axis=1).reshape(-1)[: self._len]
        return np.frombuffer(b"ACGT", dtype=np.uint8)[codes].tobytes().decode()


class DnaBuffer:
    """Owning contiguous 2-bit buffer + read index (reference include/dnabuffer.hpp:14).
    Every read starts on a byte boundary (src/dnabuffer.cpp:24-31)."""

    def __init__(self, bufsize=0):
        self._chunks = []
        self._lens = []
        self._buf = None
        self._off = None
        self._bufsize = bufsize

    @classmethod
    def from_arrays(cls, packed, read_off, read_len):
        b = cls()
        b._buf = np.ascontiguousarray(packed, dtype=np.uint8)
        b._off = np.ascontiguousarray(read_off, dtype=np.uint64)
        b._lens = list(np.asarray(read_len, dtype=np.uint32))
        return b

    @classmethod
    def from_sequences(cls, seqs):
        b = cls()
        for s in seqs:
            b.push_back(s)
        return b

    def push_back(self, s, length=None):
        if length is not None:
            s = s[:length]
        self._chunks.append(pack_sequence(s))
        self._lens.append(len(s))
        self._buf = None

    def _finalize(self):
        if self._buf is None:
            self._buf = np.concatenate(self._chunks) if self._chunks else np.zeros(0, dtype=np.uint8)
            nb = np.array([c.size for c in self._chunks], dtype=np.uint64)
            self._off = np.zeros(len(self._chunks), dtype=np.uint64)
            if len(self._chunks):
                self._off[1:] = np.cumsum(nb)[:-1]
        return self._buf

    def size(self):
        return len(self._lens)

    __len__ = size

    def getbufsize(self):
        return int(self._finalize().size)

    def __getitem__(self, i):
        buf = self._finalize()
        o = int(self._off[i])
        return DnaSeq(self._lens[i], buf[o:o + (int(self._lens[i]) + 3) // 4])

    def arrays(self):
        buf = self._finalize()
        return buf, self._off, np.asarray(self._lens, dtype=np.uint32)


class KmerList:
    """KmerListS (reference include/kmer.hpp:410): parallel arrays instead of a vector of structs.
    kmers[i] are the TKmer words (longs[0..nw)), cnt[i] the count; with EXTENSION entry i owns
    pos/rid[payload_off[i]:payload_off[i]+cnt[i]] (KmerListEntryS::pos / ::rid); see payload(i)."""

    def __init__(self, k, kmers, cnt, task_off, payload_off=None, pos=None, rid=None, histo=None, info=None):
        self.k = k
        self.kmers, self.cnt, self.task_off = kmers, cnt, task_off
        self.payload_off, self.pos, self.rid = payload_off, pos, rid
        self.histo = histo
        self.info = info or {}

    def __len__(self):
        return int(self.cnt.size)

    def payload(self, i):
        """(pos, rid) arrays of entry i (EXTENSION)."""
        a = int(self.payload_off[i]); b = a + int(self.cnt[i])
        return self.pos[a:b], self.rid[a:b]

    def kmer_string(self, i):
        w = self.kmers[i]
        return "".join("ACGT"[(int(w[j // 32]) >> (2 * (31 - j % 32))) & 3] for j in range(self.k))

    def strings(self):
        n = len(self)
        lut = np.frombuffer(b"ACGT", dtype=np.uint8)
        cols = [lut[((self.kmers[:, j // 32] >> np.uint64(2 * (31 - j % 32))) & np.uint64(3)).astype(np.int64)] for j in range(self.k)]
        arr = np.stack(cols, axis=1) if n else np.zeros((0, self.k), dtype=np.uint8)
        return [r.tobytes().decode() for r in arr]


class ReadPairs:
    """The read pairs that share k-mers (hsk_result_pairs, include/hsk.h): one row per pair of reads rid_a < rid_b (unsigned) with
    `shared` common k-mer occurrence pairs; first_pos_* / last_pos_* are the smallest / largest (pos_a, pos_b) among them.  Rows are
    in ascending (rid_a, rid_b).  With on_device the rows stay in HBM: rows_dev (n rows of four uint64 words { rid_a << 32 | rid_b,
    shared, first, last }) and n; close() gives them back to the context.  There is no strand -- unless the list is oriented
    (hsk_result_pairs_oriented, DeviceResult.pairs(strands=...)): bit 63 of the key is then the relative strand of the two occurrences,
    `opposite` is that bit as a bool array and rid_a is the key's upper half without it; a read pair has up to two rows, all same-strand
    rows first.  fold() gives the unoriented list."""

    def __init__(self, key, shared, first, last, info=None, rows_dev=None, n=None, owner=None, oriented=False):
        self.key, self.shared, self.first, self.last = (np.ascontiguousarray(x, dtype=np.uint64) for x in (key, shared, first, last))
        lo = np.uint64(0xFFFFFFFF)
        self.oriented = bool(oriented)
        self.rid_a, self.rid_b = (self.key >> np.uint64(32)).astype(np.uint32), (self.key & lo).astype(np.uint32)
        self.opposite = None
        if self.oriented:                        # (an unoriented list may have bit 31 of rid_a set: read ids are unsigned 32-bit numbers there)
            self.opposite = (self.key >> np.uint64(63)).astype(bool)
            self.rid_a = self.rid_a & np.uint32(0x7FFFFFFF)
        self.first_pos_a, self.first_pos_b = (self.first >> np.uint64(32)).astype(np.uint32), (self.first & lo).astype(np.uint32)
        self.last_pos_a, self.last_pos_b = (self.last >> np.uint64(32)).astype(np.uint32), (self.last & lo).astype(np.uint32)
        self.info = info or {}
        self.rows_dev = rows_dev
        self.n = int(self.key.size) if n is None else int(n)
        self._owner = owner                      # (ctx, hsk_pairs) of rows that live on the device

    def __len__(self):
        return self.n

    def rows(self):
        """[n, 4] uint64: { key, shared, first, last }, the C ABI's layout."""
        return np.stack([self.key, self.shared, self.first, self.last], axis=1) if self.key.size else np.zeros((0, 4), np.uint64)

    @classmethod
    def from_rows(cls, rows, **kw):
        rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 4)
        return cls(rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], **kw)

    @staticmethod
    def combine(parts, min_shared=1, ctx=None, on_device=False):
        """The list of the union of disjoint task ranges, or of the ranks of a several-GPU run, from their lists: rows with equal keys
        join -- shared adds up, first is the minimum, last the maximum -- and min_shared is applied afterwards.  The parts must have
        been computed with min_shared=1.  Without ctx: on the host, in numpy (the parts' rows must be on the host).  With a Context:
        hsk_pairs_merge on its GPU -- parts whose rows are on the device are read there, host rows are uploaded, and on_device=True
        leaves the result in HBM as DeviceResult.pairs does.  Oriented parts give an oriented list (bit 63 is part of the key); oriented
        and unoriented parts do not combine (ValueError)."""
        parts = list(parts)
        flags = {bool(p.oriented) for p in parts}
        if len(flags) > 1:
            raise ValueError("oriented and unoriented read pair lists do not combine: fold() the oriented ones first")
        oriented = bool(flags) and flags.pop()
        if ctx is not None:
            return ReadPairs._combine_device(parts, min_shared, ctx, on_device, oriented)
        rows = [p.rows() for p in parts if len(p)]
        if not rows:
            return ReadPairs.from_rows(np.zeros((0, 4), np.uint64), oriented=oriented)
        r = np.concatenate(rows)
        r = r[np.argsort(r[:, 0], kind="stable")]
        start = np.flatnonzero(np.concatenate([[True], r[1:, 0] != r[:-1, 0]]))
        out = np.stack([r[start, 0], np.add.reduceat(r[:, 1], start), np.minimum.reduceat(r[:, 2], start), np.maximum.reduceat(r[:, 3], start)], axis=1)
        info = {k: sum(int(p.info.get(k, 0)) for p in parts) for k in ("records", "self_records")}
        info["keys"] = int(out.shape[0])
        return ReadPairs.from_rows(out[out[:, 1] >= np.uint64(min_shared)], info=info, oriented=oriented)

    def fold(self, min_shared=1):
        """The unoriented list of an oriented one, on the host (the folding property, include/hsk.h): bit 63 of every key cleared, rows
        with equal keys joined -- shared adds up, first is the minimum, last the maximum -- and min_shared applied afterwards: the list
        DeviceResult.pairs gives without strands for the same task range (from an oriented list computed with min_shared=1)."""
        if not self.oriented:
            raise ValueError("fold() is for an oriented list")
        r = self.rows().copy()
        r[:, 0] &= np.uint64(0x7FFFFFFFFFFFFFFF)
        info = {k: v for k, v in self.info.items() if k in ("records", "self_records")}
        return ReadPairs.combine([ReadPairs.from_rows(r, info=info)], min_shared=min_shared)

    @staticmethod
    def _combine_device(parts, min_shared, ctx, on_device, oriented=False):
        structs, keep = [], []
        for p in parts:
            s = _lib.Pairs()
            s.n = len(p)
            s.records, s.self_records = int(p.info.get("records", 0)), int(p.info.get("self_records", 0))
            if len(p) and p.rows_dev:
                s.rows_dev = p.rows_dev
            elif len(p):
                r = np.ascontiguousarray(p.rows(), dtype=np.uint64)
                keep.append(r)
                s.rows = r.ctypes.data_as(C.POINTER(C.c_uint64))
            structs.append(s)
        arr = (C.POINTER(_lib.Pairs) * max(len(structs), 1))(*[C.pointer(s) for s in structs])
        pr = _lib.Pairs()
        ctx._check(ctx.lib.hsk_pairs_merge(ctx.h, arr, len(structs), min_shared, 1 if on_device else 0, C.byref(pr)))
        return ReadPairs._wrap(ctx, pr, on_device, oriented=oriented)

    @staticmethod
    def _wrap(ctx, pr, on_device, extra=None, oriented=False):
        """A ReadPairs from a filled hsk_pairs: the rows copied to numpy and the struct freed, or (on_device) left in HBM and owned."""
        info = dict(records=int(pr.records), self_records=int(pr.self_records), keys=int(pr.keys), sort_passes=int(pr.sort_passes),
                    ms_expand=pr.ms_expand, ms_sort=pr.ms_sort, ms_reduce=pr.ms_reduce, ms_d2h=pr.ms_d2h, ms_total=pr.ms_total)
        info.update(extra or {})
        n = int(pr.n)
        if on_device:
            z = np.zeros(0, np.uint64)
            return ReadPairs(z, z, z, z, info=info, rows_dev=pr.rows_dev, n=n, owner=(ctx, pr), oriented=oriented)
        rows = np.ctypeslib.as_array(pr.rows, shape=(n * 4,)).reshape(n, 4).copy() if n else np.zeros((0, 4), np.uint64)
        ctx.lib.hsk_pairs_free(ctx.h, C.byref(pr))
        return ReadPairs.from_rows(rows, info=info, oriented=oriented)

    def close(self):
        if self._owner is not None:
            ctx, pr = self._owner
            if getattr(ctx, "h", None):
                ctx.lib.hsk_pairs_free(ctx.h, C.byref(pr))
            self._owner, self.rows_dev = None, None

    def __del__(self):
        try:
            self.close()                 # (rows left on the device go back while the context is alive; after hsk_destroy there is nothing to free)
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class PairDiagonals:
    """The oriented read pairs by diagonal (hsk_result_pair_diagonals, include/hsk.h): rows { key, shared, bin, support, first, last } with
    key = o << 63 | rid_a << 32 | rid_b.  A record's diagonal number is D = pos_a - pos_b + 2^32 on the same strand (o = 0) and pos_a + pos_b
    on opposite strands (o = 1), its bin D // diag_bin.  all_bins=False: one row per key -- the bin with the most records (the smallest such
    bin on a tie), `support` its records, `shared` the records of the key over all bins, first_pos_* / last_pos_* the smallest / largest
    (pos_a, pos_b) of that bin only.  all_bins=True: one row per (key, bin), ascending, shared == support.  With on_device the rows stay in
    HBM (rows_dev: n rows of six uint64 words; close() gives them back).  select() and combine() work on all-bins lists, on the host or, with
    a Context, on its GPU."""

    COLS = 6

    def __init__(self, key, shared, bin, support, first, last, diag_bin=None, all_bins=False, info=None, rows_dev=None, n=None, owner=None):
        self.key, self.shared, self.bin, self.support, self.first, self.last = (np.ascontiguousarray(x, dtype=np.uint64) for x in (key, shared, bin, support, first, last))
        lo = np.uint64(0xFFFFFFFF)
        self.diag_bin = None if diag_bin is None else int(diag_bin)
        self.all_bins = bool(all_bins)
        self.opposite = (self.key >> np.uint64(63)).astype(bool)
        self.rid_a, self.rid_b = ((self.key >> np.uint64(32)) & np.uint64(0x7FFFFFFF)).astype(np.uint32), (self.key & lo).astype(np.uint32)
        self.first_pos_a, self.first_pos_b = (self.first >> np.uint64(32)).astype(np.uint32), (self.first & lo).astype(np.uint32)
        self.last_pos_a, self.last_pos_b = (self.last >> np.uint64(32)).astype(np.uint32), (self.last & lo).astype(np.uint32)
        self.info = info or {}
        self.rows_dev = rows_dev
        self.n = int(self.key.size) if n is None else int(n)
        self._owner = owner                      # (ctx, hsk_pair_diags) of rows that live on the device

    def __len__(self):
        return self.n

    def rows(self):
        """[n, 6] uint64: { key, shared, bin, support, first, last }, the C ABI's layout."""
        return np.stack([self.key, self.shared, self.bin, self.support, self.first, self.last], axis=1) if self.key.size else np.zeros((0, 6), np.uint64)

    @classmethod
    def from_rows(cls, rows, **kw):
        rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 6)
        return cls(*(rows[:, i] for i in range(6)), **kw)

    def diagonal(self):
        """(lo, hi), two int64 arrays: the range a row's bin covers -- of pos_a - pos_b (signed) for a same-strand row, of pos_a + pos_b for an
        opposite-strand row.  Needs diag_bin."""
        if self.diag_bin is None:
            raise ValueError("diagonal() needs the bin width: give diag_bin to from_rows()")
        w = self.diag_bin
        lo = self.bin.astype(np.int64) * w - np.where(self.opposite, 0, 1 << 32)
        return lo, lo + (w - 1)

    def select(self, min_support=1, ctx=None, on_device=False):
        """The selection property (include/hsk.h): the list by best bin of an all-bins list that was computed with min_support=1 -- per
        key shared is the sum of support, the row with the largest support is kept (the smallest bin on a tie), and min_support is
        applied afterwards.  Without ctx: on the host, in numpy.  With a Context: hsk_pair_diags_merge of this one list on its GPU (rows
        in HBM are read there; on_device=True leaves the result there)."""
        if not self.all_bins:
            raise ValueError("select() is for an all-bins list")
        if ctx is not None:
            return PairDiagonals._combine_device([self], ctx, False, min_support, on_device, self.diag_bin)
        r = self.rows()
        info = dict(self.info)
        if not r.shape[0]:
            return PairDiagonals.from_rows(r, diag_bin=self.diag_bin, all_bins=False, info=info)
        start = np.flatnonzero(np.concatenate([[True], r[1:, 0] != r[:-1, 0]]))
        shared = np.add.reduceat(r[:, 3], start)
        grp = np.cumsum(np.concatenate([[False], r[1:, 0] != r[:-1, 0]]))
        # rows are in ascending (key, bin): the first row of a key that reaches the key's largest support is the one with the smallest bin
        top = np.maximum.reduceat(r[:, 3], start)
        is_top = r[:, 3] == top[grp]
        idx = np.arange(r.shape[0])
        pick = np.minimum.reduceat(np.where(is_top, idx, r.shape[0]), start)
        out = r[pick].copy()
        out[:, 1] = shared
        info["keys"] = int(start.size)
        return PairDiagonals.from_rows(out[out[:, 3] >= np.uint64(min_support)], diag_bin=self.diag_bin, all_bins=False, info=info)

    @staticmethod
    def combine(parts, ctx=None, all_bins=True, min_support=1, on_device=False):
        """The several-list contract: the all-bins list of the union of disjoint task ranges, or of the ranks of a several-GPU run, from
        their all-bins lists (computed with min_support=1, same diag_bin): rows with equal (key, bin) join -- support and shared add up,
        first is the minimum, last the maximum.  Best-bin lists do not combine (ValueError): select() the joined list.  Without ctx: on
        the host, in numpy (the parts' rows must be on the host).  With a Context: hsk_pair_diags_merge on its GPU -- parts whose rows
        are on the device are read there, host rows are uploaded, min_support is applied after the join, all_bins=False runs the
        selection on the joined list, and on_device=True leaves the result in HBM."""
        parts = list(parts)
        if any(not p.all_bins for p in parts):
            raise ValueError("lists by best bin do not combine: combine the all-bins lists, then select()")
        widths = {p.diag_bin for p in parts}
        if len(widths) > 1:
            raise ValueError("lists of different diag_bin do not combine")
        w = widths.pop() if widths else None
        if ctx is not None:
            return PairDiagonals._combine_device(parts, ctx, all_bins, min_support, on_device, w)
        if not all_bins or min_support != 1 or on_device:
            raise ValueError("all_bins=False, min_support and on_device are for the device join: give a ctx, or select() the joined list")
        info = {k: sum(int(p.info.get(k, 0)) for p in parts) for k in ("records", "self_records")}
        rows = [p.rows() for p in parts if len(p)]
        if not rows:
            info.update(keys=0, bins=0)
            return PairDiagonals.from_rows(np.zeros((0, 6), np.uint64), diag_bin=w, all_bins=True, info=info)
        r = np.concatenate(rows)
        r = r[np.lexsort((r[:, 2], r[:, 0]))]
        new = np.concatenate([[True], (r[1:, 0] != r[:-1, 0]) | (r[1:, 2] != r[:-1, 2])])
        start = np.flatnonzero(new)
        sup = np.add.reduceat(r[:, 3], start)
        out = np.stack([r[start, 0], sup, r[start, 2], sup, np.minimum.reduceat(r[:, 4], start), np.maximum.reduceat(r[:, 5], start)], axis=1)
        info.update(keys=int(np.unique(out[:, 0]).size), bins=int(out.shape[0]))
        return PairDiagonals.from_rows(out, diag_bin=w, all_bins=True, info=info)

    @staticmethod
    def _combine_device(parts, ctx, all_bins, min_support, on_device, diag_bin):
        structs, keep = [], []
        for p in parts:
            s = _lib.PairDiags()
            s.n = len(p)
            s.records, s.self_records = int(p.info.get("records", 0)), int(p.info.get("self_records", 0))
            if len(p) and p.rows_dev:
                s.rows_dev = p.rows_dev
            elif len(p):
                r = np.ascontiguousarray(p.rows(), dtype=np.uint64)
                keep.append(r)
                s.rows = r.ctypes.data_as(C.POINTER(C.c_uint64))
            structs.append(s)
        arr = (C.POINTER(_lib.PairDiags) * max(len(structs), 1))(*[C.pointer(s) for s in structs])
        pd = _lib.PairDiags()
        ctx._check(ctx.lib.hsk_pair_diags_merge(ctx.h, arr, len(structs), int(min_support), 1 if all_bins else 0, 1 if on_device else 0, C.byref(pd)))
        return PairDiagonals._wrap(ctx, pd, on_device, diag_bin, bool(all_bins))

    def extend(self, ctx, reads, rid_base=None, match=1, mismatch=1, xdrop=7, min_score=0, min_length=0, wave_span=0, on_device=False):
        """hsk_pair_diags_extend: the seed of every row (`first`) extended in both directions, ungapped, with an x-drop stop, over the reads
        in HBM -- one overlap row per row of this list (best-bin or all-bins; rows in HBM are read there, host rows are uploaded).  reads: a
        DeviceDna (read where it lies), a DnaBuffer or a (packed, off, lens) tuple of host arrays (uploaded for the call), as
        DeviceResult.strands takes them; rid_base: the id of read 0 (default: the buffer's first_read_id, else 0).  match in 1 .. 2^15,
        mismatch (a penalty) in 0 .. 2^15, xdrop in 0 .. 2^31 - 1; min_score / min_length drop rows after the extension; wave_span: rows
        whose span is at least this many columns are extended by a whole wavefront (0: the library's default, 1: all, 0xFFFFFFFF: none; the
        rows are the same).  Returns an Overlaps (on_device=True: its rows stay in HBM; close() it before the context goes)."""
        opts = _lib.ExtendOpts()
        opts.match, opts.mismatch, opts.xdrop, opts.min_score, opts.min_length, opts.wave_span = int(match), int(mismatch), int(xdrop), int(min_score), int(min_length), int(wave_span)
        return self._extend_call(ctx, ctx.lib.hsk_pair_diags_extend, reads, rid_base, opts, on_device)

    def extend_gapped(self, ctx, reads, rid_base=None, match=1, mismatch=1, gap=1, xdrop=7, band=15, min_score=0, min_length=0, group=0, on_device=False):
        """hsk_pair_diags_extend_gapped: the seed of every row extended in both directions inside a band of diagonals -- cell by cell over
        the antidiagonals, with match / mismatch / gap scores and an x-drop stop (include/hsk.h has the definition) --, so that the overlap
        follows the reads across insertions and deletions.  Rows, reads, rid_base, min_score, min_length and on_device as in extend().
        match in 1 .. 255, mismatch and gap (penalties) in 0 .. 255, xdrop in 0 .. 2^31 - 1, band in 0 .. 63 (band 0 gives extend()'s rows);
        group: the lanes that take one row, 0 (the smallest that holds the band) or 8, 16, 32, 64 with band <= group - 1 -- the rows are the
        same.  Reads with la + lb >= 2^22 are refused.  Returns an Overlaps: `edits` counts substitutions and gap bases, info["cells"] the
        live cells of all rows."""
        opts = _lib.GappedOpts()
        opts.match, opts.mismatch, opts.gap, opts.xdrop, opts.band = int(match), int(mismatch), int(gap), int(xdrop), int(band)
        opts.min_score, opts.min_length, opts.group = int(min_score), int(min_length), int(group)
        return self._extend_call(ctx, ctx.lib.hsk_pair_diags_extend_gapped, reads, rid_base, opts, on_device)

    def _extend_call(self, ctx, fn, reads, rid_base, opts, on_device):
        """what extend() and extend_gapped() share: the rows where they lie, the reads where they lie, the call, the Overlaps"""
        pd = _lib.PairDiags()
        pd.n = len(self)
        keep = None
        if len(self) and self.rows_dev:
            pd.rows_dev = self.rows_dev
        elif len(self):
            keep = np.ascontiguousarray(self.rows(), dtype=np.uint64)
            pd.rows = keep.ctypes.data_as(C.POINTER(C.c_uint64))
        ov = _lib.Overlaps()
        if isinstance(reads, DeviceDna):
            base = reads.first_read_id if rid_base is None else rid_base
            rc = fn(ctx.h, C.byref(pd), reads.dp, reads.nbytes, reads.do, reads.dl, reads.nreads, base, 1, C.byref(opts), 1 if on_device else 0, C.byref(ov))
        else:
            base = getattr(reads, "first_read_id", 0) if rid_base is None else rid_base
            packed, off, lens = reads.arrays() if isinstance(reads, DnaBuffer) else reads
            packed = np.ascontiguousarray(packed, dtype=np.uint8)
            off = np.ascontiguousarray(off, dtype=np.uint64)
            lens = np.ascontiguousarray(lens, dtype=np.uint32)
            rc = fn(ctx.h, C.byref(pd), _p(packed), packed.size, _p(off), _p(lens), lens.size, base, 0, C.byref(opts), 1 if on_device else 0, C.byref(ov))
        ctx._check(rc)
        return Overlaps._wrap(ctx, ov, on_device)

    @staticmethod
    def _wrap(ctx, pd, on_device, diag_bin, all_bins, extra=None):
        """A PairDiagonals from a filled hsk_pair_diags: the rows copied to numpy and the struct freed, or (on_device) left in HBM and owned."""
        info = dict(records=int(pd.records), self_records=int(pd.self_records), keys=int(pd.keys), bins=int(pd.bins), sort_passes=int(pd.sort_passes),
                    ms_expand=pd.ms_expand, ms_sort=pd.ms_sort, ms_reduce=pd.ms_reduce, ms_d2h=pd.ms_d2h, ms_total=pd.ms_total)
        info.update(extra or {})
        n = int(pd.n)
        if on_device:
            z = np.zeros(0, np.uint64)
            return PairDiagonals(z, z, z, z, z, z, diag_bin=diag_bin, all_bins=all_bins, info=info, rows_dev=pd.rows_dev, n=n, owner=(ctx, pd))
        rows = np.ctypeslib.as_array(pd.rows, shape=(n * 6,)).reshape(n, 6).copy() if n else np.zeros((0, 6), np.uint64)
        ctx.lib.hsk_pair_diags_free(ctx.h, C.byref(pd))
        return PairDiagonals.from_rows(rows, diag_bin=diag_bin, all_bins=all_bins, info=info)

    def close(self):
        if self._owner is not None:
            ctx, pd = self._owner
            if getattr(ctx, "h", None):
                ctx.lib.hsk_pair_diags_free(ctx.h, C.byref(pd))
            self._owner, self.rows_dev = None, None

    def __del__(self):
        try:
            self.close()                 # (rows left on the device go back while the context is alive; after hsk_destroy there is nothing to free)
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Overlaps:
    """The x-drop overlaps of a list of diagonal rows, ungapped (hsk_pair_diags_extend, include/hsk.h) or banded and gapped
    (hsk_pair_diags_extend_gapped: `edits` is `mismatches`, info["cells"] the live cells): rows { key, score, a_lo << 32 | a_hi,
    b_lo << 32 | b_hi, mismatches << 32 | ends, support } with key = o << 63 | rid_a << 32 | rid_b.  [a_lo, a_hi) and [b_lo, b_hi) are
    forward read coordinates, half-open; ends has bit 0 a_lo == 0, bit 1 a_hi == len(a), bit 2 b_lo == 0, bit 3 b_hi == len(b).  info has
    input_rows, dropped, columns, wave_rows and the ms_* of the call.  With on_device the rows stay in HBM (rows_dev: n rows of six uint64
    words; close() gives them back)."""

    COLS = 6
    INTERNAL, DOVETAIL, A_CONTAINED, B_CONTAINED = 0, 1, 2, 3

    def __init__(self, key, score, a, b, mm_ends, support, info=None, rows_dev=None, n=None, owner=None):
        self.key, self.score, self._a, self._b, self._me, self.support = (np.ascontiguousarray(x, dtype=np.uint64) for x in (key, score, a, b, mm_ends, support))
        lo = np.uint64(0xFFFFFFFF)
        self.a_lo, self.a_hi = (self._a >> np.uint64(32)).astype(np.uint32), (self._a & lo).astype(np.uint32)
        self.b_lo, self.b_hi = (self._b >> np.uint64(32)).astype(np.uint32), (self._b & lo).astype(np.uint32)
        self.mismatches, self.ends = (self._me >> np.uint64(32)).astype(np.uint32), (self._me & lo).astype(np.uint32)
        self.edits = self.mismatches             # (the gapped call's name for the same word: substitutions and gap bases)
        self.opposite = (self.key >> np.uint64(63)).astype(bool)
        self.rid_a, self.rid_b = ((self.key >> np.uint64(32)) & np.uint64(0x7FFFFFFF)).astype(np.uint32), (self.key & lo).astype(np.uint32)
        self.info = info or {}
        self.rows_dev = rows_dev
        self.n = int(self.key.size) if n is None else int(n)
        self._owner = owner                      # (ctx, hsk_overlaps) of rows that live on the device

    def __len__(self):
        return self.n

    def rows(self):
        """[n, 6] uint64, the C ABI's layout."""
        return np.stack([self.key, self.score, self._a, self._b, self._me, self.support], axis=1) if self.key.size else np.zeros((0, 6), np.uint64)

    @classmethod
    def from_rows(cls, rows, **kw):
        rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 6)
        return cls(*(rows[:, i] for i in range(6)), **kw)

    def kind(self):
        """One small integer per row, what an overlapper asks next: A_CONTAINED -- the overlap is all of read A (ends has bits 0 and 1);
        B_CONTAINED -- all of read B (bits 2 and 3) and not the former; DOVETAIL -- the side of the low columns reached a read's end and so did
        the side of the high columns (same strand: bit 0 or 2, and bit 1 or 3; opposite strands, where B runs backwards: bit 0 or 3, and
        bit 1 or 2); INTERNAL -- a local match that stops inside both reads on some side."""
        e = self.ends
        b = [(e >> np.uint32(i)) & np.uint32(1) != 0 for i in range(4)]
        low = np.where(self.opposite, b[0] | b[3], b[0] | b[2])
        high = np.where(self.opposite, b[1] | b[2], b[1] | b[3])
        k = np.where(low & high, self.DOVETAIL, self.INTERNAL)
        k = np.where(b[2] & b[3], self.B_CONTAINED, k)
        k = np.where(b[0] & b[1], self.A_CONTAINED, k)
        return k.astype(np.uint8)

    def reduce(self, ctx, reads, rid_base=None, fuzz=10, wave_degree=0, on_device=False):
        """hsk_overlaps_reduce: the string graph of this list (include/hsk.h has the definition) -- the reads that lie inside another read
        go out, the dovetails become arcs between read ends, every arc that two shorter arcs explain is marked; what is left are the
        edges.  Rows in HBM are read there, host rows are uploaded.  reads: only the lengths are used -- a DeviceDna (read where they lie), a
        DnaBuffer, a (packed, off, lens) tuple or a bare array of lengths; rid_base: the id of read 0 (default: the buffer's first_read_id,
        else 0).  fuzz: the bases by which the two short arcs may exceed the long one -- what it has to cover is the indel drift along one
        overlap; wave_degree: vertices with at least this many out-arcs are reduced by a whole workgroup (0: the library's default, 1: all,
        0xFFFFFFFF: none; the result is the same).  Returns an OverlapGraph (on_device=True: everything stays in HBM; close() it before the
        context goes)."""
        ov = _lib.Overlaps()
        ov.n = len(self)
        keep = None
        if len(self) and self.rows_dev:
            ov.rows_dev = self.rows_dev
        elif len(self):
            keep = np.ascontiguousarray(self.rows(), dtype=np.uint64)
            ov.rows = keep.ctypes.data_as(C.POINTER(C.c_uint64))
        opts = _lib.ReduceOpts(fuzz=int(fuzz), wave_degree=int(wave_degree))
        rd = _lib.Reduced()
        if isinstance(reads, DeviceDna):
            base = reads.first_read_id if rid_base is None else rid_base
            rc = ctx.lib.hsk_overlaps_reduce(ctx.h, C.byref(ov), reads.dl, reads.nreads, base, 1, C.byref(opts), 1 if on_device else 0, C.byref(rd))
        else:
            base = getattr(reads, "first_read_id", 0) if rid_base is None else rid_base
            lens = reads.arrays()[2] if isinstance(reads, DnaBuffer) else (reads[2] if isinstance(reads, tuple) else reads)
            lens = np.ascontiguousarray(lens, dtype=np.uint32)
            rc = ctx.lib.hsk_overlaps_reduce(ctx.h, C.byref(ov), _p(lens), lens.size, base, 0, C.byref(opts), 1 if on_device else 0, C.byref(rd))
        ctx._check(rc)
        return OverlapGraph._wrap(ctx, rd, on_device, int(base))

    @staticmethod
    def _wrap(ctx, ov, on_device):
        """An Overlaps from a filled hsk_overlaps: the rows copied to numpy and the struct freed, or (on_device) left in HBM and owned."""
        info = dict(input_rows=int(ov.input_rows), dropped=int(ov.dropped), columns=int(ov.columns), wave_rows=int(ov.wave_rows), cells=int(ov.cells),
                    ms_extend=ov.ms_extend, ms_d2h=ov.ms_d2h, ms_total=ov.ms_total)
        n = int(ov.n)
        if on_device:
            z = np.zeros(0, np.uint64)
            return Overlaps(z, z, z, z, z, z, info=info, rows_dev=ov.rows_dev, n=n, owner=(ctx, ov))
        rows = np.ctypeslib.as_array(ov.rows, shape=(n * 6,)).reshape(n, 6).copy() if n else np.zeros((0, 6), np.uint64)
        ctx.lib.hsk_overlaps_free(ctx.h, C.byref(ov))
        return Overlaps.from_rows(rows, info=info)

    def close(self):
        if self._owner is not None:
            ctx, ov = self._owner
            if getattr(ctx, "h", None):
                ctx.lib.hsk_overlaps_free(ctx.h, C.byref(ov))
            self._owner, self.rows_dev = None, None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class OverlapGraph:
    """The string graph of a list of overlap rows (hsk_overlaps_reduce, include/hsk.h): `edges` -- an Overlaps with the KEPT rows in the
    input's order --, `row_class` -- one of the class constants per input row --, `contained` -- one bool per read --, and info:
    input_rows, rows per class under the classes' names in lower case, contained_reads, arcs, wave_vertices, max_degree, wave_degree (the
    threshold that was used) and the ms_* of the call.  With on_device all three stay in HBM: edges.rows_dev, row_class_dev (input_rows
    bytes) and contained_dev ((nreads + 31) // 32 uint32 words, read r is bit r % 32 of word r // 32); row_class and contained are then
    None, host_copy() fetches them, close() gives everything back."""

    KEPT, REDUCED, INTERNAL, A_CONTAINED, B_CONTAINED, DROPPED_READ, DUPLICATE, SELF = range(8)
    CLASS_NAMES = ("kept", "reduced", "internal", "a_contained", "b_contained", "dropped_read", "duplicate", "self")

    def __init__(self, edges, row_class, contained, info, rid_base=0, nreads=0, row_class_dev=None, contained_dev=None, owner=None):
        self.edges, self.row_class, self.contained, self.info = edges, row_class, contained, info
        self.rid_base, self.nreads = int(rid_base), int(nreads)
        self.row_class_dev, self.contained_dev = row_class_dev, contained_dev
        self._owner = owner                      # (ctx, hsk_reduced) of a graph that lives on the device

    def __len__(self):
        return len(self.edges)

    @staticmethod
    def unpack_contained(words, nreads):
        """one bool per read from the bit words of the C ABI"""
        return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")[:nreads].astype(bool)

    @staticmethod
    def _wrap(ctx, rd, on_device, rid_base):
        info = dict(input_rows=int(rd.input_rows), contained_reads=int(rd.contained_reads), arcs=int(rd.arcs), wave_vertices=int(rd.wave_vertices), max_degree=int(rd.max_degree),
                    wave_degree=int(rd.wave_degree), ms_classify=rd.ms_classify, ms_sort=rd.ms_sort, ms_reduce=rd.ms_reduce, ms_d2h=rd.ms_d2h, ms_total=rd.ms_total)
        info.update({name: int(rd.class_rows[i]) for i, name in enumerate(OverlapGraph.CLASS_NAMES)})
        n, rows_in, nreads = int(rd.n), int(rd.input_rows), int(rd.nreads)
        if on_device:
            z = np.zeros(0, np.uint64)
            edges = Overlaps(z, z, z, z, z, z, rows_dev=rd.rows_dev, n=n)      # (the rows belong to the graph)
            return OverlapGraph(edges, None, None, info, rid_base, nreads, row_class_dev=rd.row_class_dev, contained_dev=rd.contained_dev, owner=(ctx, rd))
        rows = np.ctypeslib.as_array(rd.rows, shape=(n * 6,)).reshape(n, 6).copy() if n else np.zeros((0, 6), np.uint64)
        cls = np.ctypeslib.as_array(rd.row_class, shape=(rows_in,)).copy() if rows_in else np.zeros(0, np.uint8)
        words = np.ctypeslib.as_array(rd.contained, shape=((nreads + 31) // 32,)).copy() if nreads else np.zeros(0, np.uint32)
        ctx.lib.hsk_reduced_free(ctx.h, C.byref(rd))
        return OverlapGraph(Overlaps.from_rows(rows), cls, OverlapGraph.unpack_contained(words, nreads), info, rid_base, nreads)

    def host_copy(self):
        """(row_class, contained) of a graph in HBM, fetched"""
        if self._owner is None:
            return self.row_class, self.contained
        ctx = self._owner[0]
        n = self.info["input_rows"]
        cls = ctx.d2h(self.row_class_dev, n) if n else np.zeros(0, np.uint8)
        words = ctx.d2h(self.contained_dev, 4 * ((self.nreads + 31) // 32)).view(np.uint32) if self.nreads else np.zeros(0, np.uint32)
        return cls, OverlapGraph.unpack_contained(words, self.nreads)

    def arcs(self, lens, rid_base=None):
        """(v, w, len, row) of the kept edges on the host, two arcs per edge (the table of include/hsk.h; numpy, needs no GPU): v = 2 r + s
        with r counted from rid_base (default: the call's), s = 1 the reverse complement; an arc v -> w says that a suffix of v overlaps
        a prefix of w, len is the number of bases of v in front of the overlap; row is the edge's index.  What a client walks."""
        e = self.edges
        base = self.rid_base if rid_base is None else int(rid_base)
        lens = np.asarray(lens, dtype=np.int64)
        a, b = e.rid_a.astype(np.int64) - base, e.rid_b.astype(np.int64) - base
        la, lb = lens[a], lens[b]
        a_lo, a_hi, b_lo, b_hi = (x.astype(np.int64) for x in (e.a_lo, e.a_hi, e.b_lo, e.b_hi))
        o, en = e.opposite.astype(np.int64), (e.ends & np.uint32(15)).astype(np.int64)
        good = np.where(o == 0, (en == 6) | (en == 9), (en == 10) | (en == 5))
        if not good.all():
            raise ValueError("row %d of the edges is no dovetail" % int(np.flatnonzero(~good)[0]))
        first = (en == 6) | (en == 10)           # a_hi == la: a is in front
        sb = o                                   # the orientation of b next to a forward a
        v1 = np.where(first, 2 * a, 2 * b + sb)
        w1 = np.where(first, 2 * b + sb, 2 * a)
        l1 = np.where(first, a_lo, np.where(o == 0, b_lo, lb - b_hi))
        l2 = np.where(first, np.where(o == 0, lb - b_hi, b_lo), la - a_hi)
        row = np.arange(len(a), dtype=np.int64)
        return np.concatenate([v1, w1 ^ 1]), np.concatenate([w1, v1 ^ 1]), np.concatenate([l1, l2]), np.concatenate([row, row])

    @staticmethod
    def pack_contained(contained):
        """the bit words of the C ABI from one bool per read"""
        bits = np.packbits(np.asarray(contained, dtype=bool), bitorder="little")
        return np.concatenate([bits, np.zeros(-bits.size % 4, np.uint8)]).view("<u4").astype(np.uint32)

    def unitigs(self, ctx, reads, rid_base=None, on_device=False):
        """hsk_overlaps_unitigs: the maximal non-branching paths of this graph's edges (include/hsk.h has the definition), one of each
        complement pair, with every member read's orientation and position -- list ranking in HBM, not a walk.  A graph in HBM gives its
        rows and its contained bits where they lie, a host graph uploads its rows and its packed bits.  reads: as Overlaps.reduce takes
        them (only the lengths are used); rid_base: default the graph's.  Returns a Unitigs (on_device=True: both row lists stay in HBM;
        close() it before the context goes)."""
        e = self.edges
        ov = _lib.Overlaps()
        ov.n = len(e)
        keep = bits = None
        if len(e) and e.rows_dev:
            ov.rows_dev = e.rows_dev
        elif len(e):
            keep = np.ascontiguousarray(e.rows(), dtype=np.uint64)
            ov.rows = keep.ctypes.data_as(C.POINTER(C.c_uint64))
        if isinstance(reads, DeviceDna):
            lens, plens, nreads, lens_dev = None, reads.dl, int(reads.nreads), 1
        else:
            lens = reads.arrays()[2] if isinstance(reads, DnaBuffer) else (reads[2] if isinstance(reads, tuple) else reads)
            lens = np.ascontiguousarray(lens, dtype=np.uint32)
            plens, nreads, lens_dev = _p(lens), int(lens.size), 0
        if nreads != self.nreads:
            raise ValueError("the graph was reduced over %d reads, lengths of %d were given" % (self.nreads, nreads))
        if self.contained_dev:
            con, con_dev = self.contained_dev, 1
        else:                                    # (no bits at all: no read is contained)
            bits = np.ascontiguousarray(OverlapGraph.pack_contained(np.zeros(nreads, bool) if self.contained is None else self.contained))
            con, con_dev = (_p(bits) if bits.size else None), 0
        base = self.rid_base if rid_base is None else rid_base
        opts = _lib.UnitigOpts()
        ut = _lib.Unitigs()
        rc = ctx.lib.hsk_overlaps_unitigs(ctx.h, C.byref(ov), con, con_dev, plens, nreads, base, lens_dev, C.byref(opts), 1 if on_device else 0, C.byref(ut))
        ctx._check(rc)
        return Unitigs._wrap(ctx, ut, on_device)

    def close(self):
        if self._owner is not None:
            ctx, rd = self._owner
            if getattr(ctx, "h", None):
                ctx.lib.hsk_reduced_free(ctx.h, C.byref(rd))
            self._owner, self.row_class_dev, self.contained_dev = None, None, None
            self.edges.rows_dev = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Unitigs:
    """The unitigs of a string graph (hsk_overlaps_unitigs, include/hsk.h).  Per member, ordered by (unitig, rank): unitig, rank, rid (the
    absolute read id), reverse (bool: the member is the read's reverse complement), offset (the unitig coordinate of the oriented read's
    first base), link_len and link_row (the link to the next member: its len and the index of its row in the graph's edges; NO_LINK in
    both for the last member of a path; the last member of a cycle links back to rank 0).  Per unitig: first (its first layout row),
    reads, bases, circular.  info: unitigs, members, singletons, circular, longest, links, branch_vertices, live_reads, input_rows, arcs,
    rounds and the ms_* of the call.  With on_device the two row lists stay in HBM (rows_dev: members rows, table_dev: unitigs rows, four
    uint64 words each; the per-member and per-unitig arrays are then empty; close() gives them back)."""

    NO_LINK = 0xFFFFFFFF

    def __init__(self, rows, table, info, rows_dev=None, table_dev=None, owner=None):
        rows, table = (np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 4) for x in (rows, table))
        lo, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
        self._rows, self._table = rows, table
        self.unitig, self.rank = (rows[:, 0] >> s32).astype(np.uint32), (rows[:, 0] & lo).astype(np.uint32)
        self.rid, self.reverse = (rows[:, 1] >> np.uint64(1)).astype(np.uint32), (rows[:, 1] & np.uint64(1)).astype(bool)
        self.offset = rows[:, 2].copy()
        self.link_len, self.link_row = (rows[:, 3] >> s32).astype(np.uint32), (rows[:, 3] & lo).astype(np.uint32)
        self.first, self.reads, self.bases, self.circular = table[:, 0].copy(), table[:, 1].copy(), table[:, 2].copy(), table[:, 3] != 0
        self.info = info
        self.rows_dev, self.table_dev = rows_dev, table_dev
        self._owner = owner                      # (ctx, hsk_unitigs) of lists that live on the device

    def __len__(self):
        return int(self.info["unitigs"])

    def rows(self):
        """[members, 4] uint64, the layout rows in the C ABI's layout"""
        return self._rows

    def table(self):
        """[unitigs, 4] uint64, the unitig rows in the C ABI's layout"""
        return self._table

    def members(self, u):
        """(rid, reverse, offset) of unitig u's members in the order of their ranks"""
        s = slice(int(self.first[u]), int(self.first[u]) + int(self.reads[u]))
        return self.rid[s], self.reverse[s], self.offset[s]

    @staticmethod
    def _wrap(ctx, ut, on_device):
        info = {k: int(getattr(ut, k)) for k in ("unitigs", "members", "singletons", "circular", "longest", "links", "branch_vertices", "live_reads", "input_rows", "arcs", "rounds")}
        info.update({k: getattr(ut, k) for k in ("ms_arcs", "ms_sort", "ms_rank", "ms_emit", "ms_d2h", "ms_total")})
        m, u = int(ut.members), int(ut.unitigs)
        z = np.zeros((0, 4), np.uint64)
        if on_device:
            return Unitigs(z, z, info, rows_dev=ut.rows_dev, table_dev=ut.table_dev, owner=(ctx, ut))
        rows = np.ctypeslib.as_array(ut.rows, shape=(m * 4,)).reshape(m, 4).copy() if m else z
        table = np.ctypeslib.as_array(ut.table, shape=(u * 4,)).reshape(u, 4).copy() if u else z
        ctx.lib.hsk_unitigs_free(ctx.h, C.byref(ut))
        return Unitigs(rows, table, info)

    def host_copy(self):
        """(layout rows, unitig rows) of lists in HBM, fetched"""
        if self._owner is None:
            return self._rows, self._table
        ctx = self._owner[0]
        m, u = self.info["members"], self.info["unitigs"]
        z = np.zeros((0, 4), np.uint64)
        return (ctx.d2h(self.rows_dev, m * 32).view(np.uint64).reshape(m, 4) if m else z), (ctx.d2h(self.table_dev, u * 32).view(np.uint64).reshape(u, 4) if u else z)

    def close(self):
        if self._owner is not None:
            ctx, ut = self._owner
            if getattr(ctx, "h", None):
                ctx.lib.hsk_unitigs_free(ctx.h, C.byref(ut))
            self._owner, self.rows_dev, self.table_dev = None, None, None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Strands:
    """The strand bits of a resident EXTENSION result (hsk_result_strands, include/hsk.h): one bit per payload slot, in HBM.  info has
    ntasks, payloads, reverse, palindromes and ms_total; task_bits(t) copies task t's bits to the host.  close() gives the arrays back
    to the context (before the context goes)."""

    def __init__(self, ctx, st):
        self.ctx, self.st = ctx, st
        self.info = dict(ntasks=int(st.ntasks), payloads=int(st.payloads), reverse=int(st.reverse), palindromes=int(st.palindromes), ms_total=st.ms_total)

    def task(self, t):
        """(device address of task t's bit words or None, number of its payload slots)"""
        bits, npay = C.c_void_p(), C.c_uint64()
        self.ctx._check(self.ctx.lib.hsk_strands_task(C.byref(self.st), t, C.byref(bits), C.byref(npay)))
        return bits.value, int(npay.value)

    def task_bits(self, t):
        """numpy bool array of npay: the strand of every payload slot of task t (False for the gaps of filtered k-mers)."""
        bits, npay = self.task(t)
        if not npay:
            return np.zeros(0, dtype=bool)
        words = self.ctx.d2h(bits, (npay + 63) // 64 * 8)
        return np.unpackbits(words, bitorder="little")[:npay].astype(bool)

    def close(self):
        if self.st is not None:
            if getattr(self.ctx, "h", None):
                self.ctx.lib.hsk_strands_free(self.ctx.h, C.byref(self.st))
            self.st = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class DeviceResult:
    """A k-mer list that stays in HBM (HSK_FLAG_KEEP_DEVICE).  task(t) gives the device addresses of task t's entries and,
    with EXTENSION, its CSR payload (payload_off / pos / rid); fetch(t) copies them to numpy arrays; pairs() turns the payload
    into the list of read pairs that share k-mers without leaving the GPU."""

    def __init__(self, ctx, res):
        self.ctx, self.res = ctx, res
        self.ntasks, self.nw, self.n = int(res.ntasks), int(res.nw), int(res.n)
        self.task_off = np.ctypeslib.as_array(res.task_off, shape=(self.ntasks + 1,)).copy()

    def task(self, t):
        e, po, pos, rid = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        n, npay, base = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self.ctx._check(self.ctx.lib.hsk_result_device_task(C.byref(self.res), t, C.byref(e), C.byref(n), C.byref(po), C.byref(pos), C.byref(rid), C.byref(npay), C.byref(base)))
        return dict(entries=e.value, n=int(n.value), payload_off=po.value, pos=pos.value, rid=rid.value, npay=int(npay.value), payload_base=int(base.value))

    def fetch(self, t):
        d = self.task(t)
        out = dict(n=d["n"], npay=d["npay"], payload_base=d["payload_base"])
        ent = self.ctx.d2h(d["entries"], d["n"] * (self.nw + 1) * 8).view(np.uint64).reshape(d["n"], self.nw + 1) if d["n"] else np.zeros((0, self.nw + 1), np.uint64)
        out["kmers"], out["cnt"] = ent[:, :self.nw].copy(), ent[:, self.nw].copy()
        if d["payload_off"] and d["n"]:
            out["payload_off"] = self.ctx.d2h(d["payload_off"], d["n"] * 8).view(np.uint64)
        if d["pos"] and d["npay"]:
            out["pos"] = self.ctx.d2h(d["pos"], d["npay"] * 4).view(np.uint32)
            out["rid"] = self.ctx.d2h(d["rid"], d["npay"] * 4).view(np.int32)
        return out

    def strands(self, reads, rid_base=None):
        """hsk_result_strands: the strand of every payload slot of the result, recovered from the reads it was counted from -- a
        DeviceDna (read where it lies in HBM), a DnaBuffer or a (packed, off, lens) tuple of host arrays (uploaded for the call).
        rid_base: the id of read 0, as it was given to the count (default: the buffer's first_read_id, else 0).  Returns a Strands;
        close() it before the context goes."""
        st = _lib.Strands()
        if isinstance(reads, DeviceDna):
            base = reads.first_read_id if rid_base is None else rid_base
            rc = self.ctx.lib.hsk_result_strands(self.ctx.h, C.byref(self.res), reads.dp, reads.nbytes, reads.do, reads.dl, reads.nreads, base, 1, C.byref(st))
        else:
            base = getattr(reads, "first_read_id", 0) if rid_base is None else rid_base
            packed, off, lens = reads.arrays() if isinstance(reads, DnaBuffer) else reads
            packed = np.ascontiguousarray(packed, dtype=np.uint8)
            off = np.ascontiguousarray(off, dtype=np.uint64)
            lens = np.ascontiguousarray(lens, dtype=np.uint32)
            rc = self.ctx.lib.hsk_result_strands(self.ctx.h, C.byref(self.res), _p(packed), packed.size, _p(off), _p(lens), lens.size, base, 0, C.byref(st))
        self.ctx._check(rc)
        return Strands(self.ctx, st)

    def pairs(self, task_lo=0, task_hi=None, min_shared=1, on_device=False, max_records=None, strands=None):
        """hsk_result_pairs over tasks [task_lo, task_hi) (default: all): the read pairs that share at least min_shared k-mer
        occurrence pairs, as a ReadPairs.  on_device=True leaves the rows in HBM (ReadPairs.rows_dev, .n; close() it before the
        context goes).  max_records=N: hsk_result_pairs_sliced -- the same list, from at most N records expanded at a time (0: the
        library chooses from the device memory that is left); info then has slices, peak_records, merges, merged_rows and ms_merge.
        strands=Strands (of this result): hsk_result_pairs_oriented -- the rows split by the relative strand of the two occurrences, an
        oriented ReadPairs (max_records=None: the single pass)."""
        pr = _lib.Pairs()
        hi = self.ntasks if task_hi is None else task_hi
        if strands is not None:
            sl = _lib.PairsSlices()
            budget = 0xFFFFFFFFFFFFFFFF if max_records is None else int(max_records)
            self.ctx._check(self.ctx.lib.hsk_result_pairs_oriented(self.ctx.h, C.byref(self.res), C.byref(strands.st), task_lo, hi, min_shared, 1 if on_device else 0,
                                                                   budget, C.byref(pr), C.byref(sl)))
            extra = dict(slices=int(sl.slices), peak_records=int(sl.peak_records), merges=int(sl.merges), merged_rows=int(sl.merged_rows), ms_merge=sl.ms_merge)
            return ReadPairs._wrap(self.ctx, pr, on_device, extra, oriented=True)
        if max_records is None:
            self.ctx._check(self.ctx.lib.hsk_result_pairs(self.ctx.h, C.byref(self.res), task_lo, hi, min_shared, 1 if on_device else 0, C.byref(pr)))
            return ReadPairs._wrap(self.ctx, pr, on_device)
        sl = _lib.PairsSlices()
        self.ctx._check(self.ctx.lib.hsk_result_pairs_sliced(self.ctx.h, C.byref(self.res), task_lo, hi, min_shared, 1 if on_device else 0, int(max_records),
                                                             C.byref(pr), C.byref(sl)))
        extra = dict(slices=int(sl.slices), peak_records=int(sl.peak_records), merges=int(sl.merges), merged_rows=int(sl.merged_rows), ms_merge=sl.ms_merge)
        return ReadPairs._wrap(self.ctx, pr, on_device, extra)

    def pair_diagonals(self, strands, diag_bin, task_lo=0, task_hi=None, min_support=1, all_bins=False, on_device=False, max_records=None):
        """hsk_result_pair_diagonals over tasks [task_lo, task_hi) (default: all): the records of pairs(strands=...) binned by diagonal
        (bins of diag_bin diagonals), as a PairDiagonals -- per oriented read pair the bin with the most records (all_bins=False), or every
        (pair, bin) (all_bins=True: what disjoint task ranges and ranks combine through, PairDiagonals.combine and .select).  strands: the
        Strands of this result.  on_device=True leaves the rows in HBM (close() it before the context goes).  max_records=N:
        hsk_result_pair_diagonals_sliced -- the same list, from at most N records expanded at a time (0: the library chooses from the
        device memory that is left); info then has slices, peak_records, merges, merged_rows and ms_merge."""
        pd = _lib.PairDiags()
        hi = self.ntasks if task_hi is None else task_hi
        if max_records is not None:
            sl = _lib.PairsSlices()
            self.ctx._check(self.ctx.lib.hsk_result_pair_diagonals_sliced(self.ctx.h, C.byref(self.res), C.byref(strands.st) if strands is not None else None, task_lo, hi,
                                                                          int(diag_bin), int(min_support), 1 if all_bins else 0, 1 if on_device else 0, int(max_records),
                                                                          C.byref(pd), C.byref(sl)))
            extra = dict(slices=int(sl.slices), peak_records=int(sl.peak_records), merges=int(sl.merges), merged_rows=int(sl.merged_rows), ms_merge=sl.ms_merge)
            return PairDiagonals._wrap(self.ctx, pd, on_device, int(diag_bin), bool(all_bins), extra)
        self.ctx._check(self.ctx.lib.hsk_result_pair_diagonals(self.ctx.h, C.byref(self.res), C.byref(strands.st) if strands is not None else None, task_lo, hi,
                                                               int(diag_bin), int(min_support), 1 if all_bins else 0, 1 if on_device else 0, C.byref(pd)))
        return PairDiagonals._wrap(self.ctx, pd, on_device, int(diag_bin), bool(all_bins))

    def close(self):
        if self.res is not None:
            self.ctx.lib.hsk_result_free(self.ctx.h, C.byref(self.res))
            self.res = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Context:
    """One hsk_ctx (one process, one GPU)."""

    def __init__(self, K=31, M=17, L=15, U=40, EXT=0, ntasks=0, device=0, plain_dispatcher=0, radix_bits=8, profile=False, keep_device=False,
                 plan=None, tuning=None, plain_classifier=False, unbalanced_ratio=None):
        """plan: None (two prefix passes + LDS aggregation, the library's choice), "no_aggregation" (HSK_FLAG_NO_AGGREGATION) or
        "full_sort" (HSK_FLAG_FULL_SORT: the reference's algorithm, LSD over all key bytes + merge-count over the sorted array).
        plain_classifier (HSK_FLAG_PLAIN_CLASSIFIER): no task is a heavy hitter; unbalanced_ratio (hsk_config::unbalanced_ratio): a task
        is one when its global k-mer count exceeds this many times the mean (the library's default when None)."""
        self.lib = _lib.load()
        cfg = _lib.Config()
        self.lib.hsk_config_default(C.byref(cfg))
        cfg.kmer_size, cfg.minimizer_size, cfg.lower_freq, cfg.upper_freq = K, M, L, U
        cfg.extension, cfg.ntasks, cfg.device, cfg.plain_dispatcher, cfg.radix_bits = EXT, ntasks, device, plain_dispatcher, radix_bits
        cfg.flags = (_lib.FLAG_PROFILE if profile else 0) | (_lib.FLAG_KEEP_DEVICE if keep_device else 0) | \
            (_lib.FLAG_PLAIN_CLASSIFIER if plain_classifier else 0) | \
            {None: 0, "no_aggregation": _lib.FLAG_NO_AGGREGATION, "full_sort": _lib.FLAG_FULL_SORT, "no_combine": _lib.FLAG_NO_COMBINE}[plan]
        if unbalanced_ratio is not None:
            cfg.unbalanced_ratio = float(unbalanced_ratio)
        # tuning: dict or "name=value,..." (hsk_config::tuning): forced paths for tests and a few measured thresholds, per context
        if isinstance(tuning, dict):
            tuning = ",".join("%s=%d" % (k, int(v)) for k, v in tuning.items())
        cfg.tuning = tuning.encode() if tuning else None
        self.keep_device = bool(keep_device)
        self.cfg = cfg
        self.K, self.EXT = K, EXT
        self.nw = (K + 31) // 32
        h = C.c_void_p()
        rc = self.lib.hsk_init(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise HskError(rc)
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.hsk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise HskError(rc, self.lib.hsk_last_error(self.h).decode())

    # ---- multi-GPU -----------------------------------------------------------------------------
    def comm_init(self, comm):
        """comm: hysortk_amd.dist.Comm; rank 0 creates the RCCL id, it is broadcast over comm."""
        if comm is None or comm.size == 1:
            return
        ident = (C.c_char * _lib.UNIQUE_ID_BYTES)()
        if comm.rank == 0:
            self._check(self.lib.hsk_comm_get_unique_id(ident))
        raw = comm.bcast_bytes(bytes(ident), root=0)
        buf = (C.c_char * _lib.UNIQUE_ID_BYTES).from_buffer_copy(raw)
        self._check(self.lib.hsk_comm_init(self.h, comm.size, comm.rank, buf))

    def copy_peak(self, nbytes=1 << 32, iters=3):
        """GB/s (read + written) of a plain 16-byte-per-lane HBM copy on this GPU: the measured yardstick beside the 8 TB/s spec."""
        g = C.c_double(0)
        self._check(self.lib.hsk_copy_peak(self.h, nbytes, iters, C.byref(g)))
        return float(g.value)

    def comm_selftest(self):
        """One-rank RCCL communicator on this GPU: all-reduce and grouped send/recv to self, results checked."""
        self._check(self.lib.hsk_comm_selftest(self.h))

    # ---- the hot path -----------------------------------------------------------------------------
    def _wrap(self, res):
        n, nw, nt = int(res.n), int(res.nw), int(res.ntasks)
        info = dict(total_kmers=int(res.total_kmers), total_supermers=int(res.total_supermers),
                    total_supermer_bytes=int(res.total_supermer_bytes), ntasks=nt,
                    ms_total=res.ms_total, ms_parse=res.ms_parse, ms_exchange=res.ms_exchange, ms_extract=res.ms_extract,
                    ms_sort=res.ms_sort, ms_count=res.ms_count, ms_d2h=res.ms_d2h)
        task_off = np.ctypeslib.as_array(res.task_off, shape=(nt + 1,)).copy()
        histo = np.ctypeslib.as_array(res.histo, shape=(int(res.histo_len),)).copy()
        kmers = cnt = payoff = pos = rid = None
        if res.entries:
            e = np.ctypeslib.as_array(res.entries, shape=(max(n, 1) * (nw + 1),))[: n * (nw + 1)].reshape(n, nw + 1)
            kmers, cnt = e[:, :nw].copy(), e[:, nw].copy()
            if res.payload_off:
                payoff = np.ctypeslib.as_array(res.payload_off, shape=(n + 1,)).copy()
                P = int(payoff[n])
                pos = np.ctypeslib.as_array(res.pos, shape=(max(P, 1),))[:P].copy()
                rid = np.ctypeslib.as_array(res.rid, shape=(max(P, 1),))[:P].copy()
        else:
            info["n"] = n
        self.lib.hsk_result_free(self.h, C.byref(res))
        if kmers is None:
            kmers, cnt = np.zeros((0, nw), dtype=np.uint64), np.zeros(0, dtype=np.uint64)
        return KmerList(self.K, kmers, cnt, task_off, payoff, pos, rid, histo, info)

    def count_resident(self, dna, rid_base=0):
        """kmer_count with the result LEFT IN HBM (the context must have keep_device=True): returns a DeviceResult whose
        per-task entry / CSR payload arrays a following GPU stage reads in place (hsk_result_device_task)."""
        if not self.keep_device:
            raise ValueError("count_resident needs Context(keep_device=True)")
        packed, off, lens = dna.arrays() if isinstance(dna, DnaBuffer) else dna
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        res = _lib.Result()
        self._check(self.lib.hsk_count(self.h, _p(packed), packed.size, _p(off), _p(lens), lens.size, rid_base, C.byref(res)))
        return DeviceResult(self, res)

    def count(self, dna, rid_base=0):
        packed, off, lens = dna.arrays() if isinstance(dna, DnaBuffer) else dna
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        res = _lib.Result()
        self._check(self.lib.hsk_count(self.h, _p(packed), packed.size, _p(off), _p(lens), lens.size, rid_base, C.byref(res)))
        return self._wrap(res)

    def count_host_timed(self, packed, off, lens, rid_base=0):
        """Wall time of ONE hsk_count() call on host arrays (bench.py's e2e_host leg): returns (seconds, entries, info); the
        result block is handed back to the library right away (no numpy copy: the C ABI result is the product)."""
        import time
        res = _lib.Result()
        t0 = time.perf_counter()
        rc = self.lib.hsk_count(self.h, _p(packed), packed.size, _p(off), _p(lens), lens.size, rid_base, C.byref(res))
        dt = time.perf_counter() - t0
        self._check(rc)
        n = int(res.n)
        info = dict(ms_total=res.ms_total, ms_parse=res.ms_parse, ms_extract=res.ms_extract, ms_sort=res.ms_sort, ms_count=res.ms_count, ms_d2h=res.ms_d2h,
                    total_kmers=int(res.total_kmers), ntasks=int(res.ntasks))
        self.lib.hsk_result_free(self.h, C.byref(res))
        return dt, n, info

    def count_device(self, d_packed, packed_bytes, d_off, d_len, nreads, rid_base=0):
        res = _lib.Result()
        self._check(self.lib.hsk_count_device(self.h, d_packed, packed_bytes, d_off, d_len, nreads, rid_base, C.byref(res)))
        return self._wrap(res)

    def count_loopback(self, dnas):
        """`len(dnas)` virtual ranks on this GPU (hsk_count_loopback): returns ([KmerList per rank], owner table)."""
        R = len(dnas)
        arrs = [d.arrays() if isinstance(d, DnaBuffer) else d for d in dnas]
        pk = [np.ascontiguousarray(a[0], dtype=np.uint8) for a in arrs]
        of = [np.ascontiguousarray(a[1], dtype=np.uint64) for a in arrs]
        ln = [np.ascontiguousarray(a[2], dtype=np.uint32) for a in arrs]
        PP = (C.c_void_p * R)(*[x.ctypes.data for x in pk])
        OP = (C.c_void_p * R)(*[x.ctypes.data for x in of])
        LP = (C.c_void_p * R)(*[x.ctypes.data for x in ln])
        nb = np.array([x.size for x in pk], dtype=np.uint64)
        nr = np.array([x.size for x in ln], dtype=np.uint64)
        outs = (_lib.Result * R)()
        owner = np.zeros(1024, dtype=np.int32)
        self._check(self.lib.hsk_count_loopback(self.h, R, PP, _p(nb), OP, LP, _p(nr), outs, _p(owner), owner.size))
        nt = int(outs[0].ntasks)
        res = [self._wrap(outs[r]) for r in range(R)]
        return res, owner[:nt].copy()

    def count_loopback_device(self, reads, wrap=True):
        """The same with every virtual rank's reads resident in HBM: reads = [(d_packed, packed_bytes, d_off, d_len, nreads)] as synth_reads
        returns them.  Returns ([KmerList (or DeviceResult with keep_device) per rank], owner table)."""
        R = len(reads)
        PP = (C.c_void_p * R)(*[r[0] for r in reads]); OP = (C.c_void_p * R)(*[r[2] for r in reads]); LP = (C.c_void_p * R)(*[r[3] for r in reads])
        nb = np.array([r[1] for r in reads], dtype=np.uint64); nr = np.array([r[4] for r in reads], dtype=np.uint64)
        outs = (_lib.Result * R)()
        owner = np.zeros(1024, dtype=np.int32)
        self._check(self.lib.hsk_count_loopback_device(self.h, R, PP, _p(nb), OP, LP, _p(nr), outs, _p(owner), owner.size))
        nt = int(outs[0].ntasks)
        return [self._wrap(outs[r]) for r in range(R)], owner[:nt].copy()

    def stats(self, reset=True):
        s = _lib.Stats()
        self._check(self.lib.hsk_get_stats(self.h, C.byref(s), 1 if reset else 0))
        return {k: getattr(s, k) for k, _ in _lib.Stats._fields_ if k != "reserved"}

    # ---- stages -------------------------------------------------------------------------------------
    def stage_destinations(self, dna):
        packed, off, lens = dna.arrays() if isinstance(dna, DnaBuffer) else dna
        packed = np.ascontiguousarray(packed, dtype=np.uint8); off = np.ascontiguousarray(off, dtype=np.uint64); lens = np.ascontiguousarray(lens, dtype=np.uint32)
        total = int(np.maximum(lens.astype(np.int64) - self.K + 1, 0).sum())
        dest = np.zeros(max(total, 1), dtype=np.int32)
        doff = np.zeros(lens.size + 1, dtype=np.uint64)
        self._check(self.lib.hsk_stage_destinations(self.h, _p(packed), packed.size, _p(off), _p(lens), lens.size, _p(dest), total, _p(doff)))
        return dest[:total], doff

    def stage_task_kmers(self, dna, task, rid_base=0):
        packed, off, lens = dna.arrays() if isinstance(dna, DnaBuffer) else dna
        packed = np.ascontiguousarray(packed, dtype=np.uint8); off = np.ascontiguousarray(off, dtype=np.uint64); lens = np.ascontiguousarray(lens, dtype=np.uint32)
        cap = int(np.maximum(lens.astype(np.int64) - self.K + 1, 0).sum())
        keys = np.zeros((max(cap, 1), self.nw), dtype=np.uint64)
        pos = np.zeros(max(cap, 1), dtype=np.uint32)
        rid = np.zeros(max(cap, 1), dtype=np.int32)
        n = C.c_uint64(0)
        self._check(self.lib.hsk_stage_task_kmers(self.h, _p(packed), packed.size, _p(off), _p(lens), lens.size, rid_base, task,
                                                  _p(keys), _p(pos), _p(rid), cap, C.byref(n)))
        n = int(n.value)
        return keys[:n], pos[:n], rid[:n]

    def stage_sort(self, keys, vals=None):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        if keys.ndim == 1:
            keys = keys.reshape(-1, 1)
        n, nw = keys.shape
        out = keys.copy()
        v = None if vals is None else np.ascontiguousarray(vals, dtype=np.uint64).copy()
        self._check(self.lib.hsk_stage_sort(self.h, _p(out), _p(v), n, nw))
        return (out, v) if vals is not None else out

    def stage_count_sorted(self, keys):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        if keys.ndim == 1:
            keys = keys.reshape(-1, 1)
        n, nw = keys.shape
        out = np.zeros((max(n, 1), nw + 1), dtype=np.uint64)
        m = C.c_uint64(0)
        self._check(self.lib.hsk_stage_count_sorted(self.h, _p(keys), n, nw, _p(out), n, C.byref(m)))
        m = int(m.value)
        return out[:m, :nw].copy(), out[:m, nw].copy()

    # ---- synthetic reads in HBM ------------------------------------------------------------------------
    def synth_reads(self, genome_len, read_len, nreads, seed, first_read=0, error_rate=0.0):
        dp, do, dl = C.c_void_p(), C.c_void_p(), C.c_void_p()
        nb = C.c_uint64(0)
        if error_rate:
            self._check(self.lib.hsk_synth_reads_err(self.h, genome_len, read_len, nreads, seed, first_read, float(error_rate), C.byref(dp), C.byref(nb), C.byref(do), C.byref(dl)))
        else:
            self._check(self.lib.hsk_synth_reads(self.h, genome_len, read_len, nreads, seed, first_read, C.byref(dp), C.byref(nb), C.byref(do), C.byref(dl)))
        return dp, int(nb.value), do, dl

    def synth_free(self, dp, do, dl):
        self.lib.hsk_synth_free(self.h, dp, do, dl)

    def format_entries(self, kmers, cnt):
        """The "KMER\\tcount\\n" lines of the entries, formatted on the GPU (hsk_format_entries); returns bytes."""
        n = len(cnt)
        if n == 0:
            return b""
        nw = kmers.shape[1]
        e = np.ascontiguousarray(np.concatenate([kmers.astype(np.uint64), np.asarray(cnt, dtype=np.uint64)[:, None]], axis=1))
        need = C.c_uint64()
        self._check(self.lib.hsk_format_entries(self.h, _p(e), n, nw, 0, None, 0, C.byref(need)))
        buf = np.zeros(int(need.value), dtype=np.uint8)
        self._check(self.lib.hsk_format_entries(self.h, _p(e), n, nw, 0, _p(buf), buf.size, C.byref(need)))
        return buf.tobytes()

    def d2h_into(self, arr, dptr, nbytes):
        self._check(self.lib.hsk_memcpy_d2h(self.h, _p(arr), dptr, nbytes))

    def d2h(self, dptr, nbytes):
        out = np.zeros(nbytes, dtype=np.uint8)
        self._check(self.lib.hsk_memcpy_d2h(self.h, _p(out), dptr, nbytes))
        return out


# ---- pure-host planning (no GPU needed) ------------------------------------------------------------------
def plan_tot_tasks(omp_max_threads, nprocs, thread_per_worker=4, avg_task_per_worker=3):
    return _lib.load().hsk_plan_tot_tasks(omp_max_threads, thread_per_worker, avg_task_per_worker, nprocs)


def plan_classify(task_kmers, unbalanced_ratio=2.3):
    a = np.ascontiguousarray(task_kmers, dtype=np.uint64)
    out = np.zeros(a.size, dtype=np.int32)
    rc = _lib.load().hsk_plan_classify(_p(a), a.size, unbalanced_ratio, _p(out))
    if rc:
        raise HskError(rc)
    return out


def plan_dispatch(task_bytes, nprocs, plain=False, upper_coe=1.5, step=0.05):
    a = np.ascontiguousarray(task_bytes, dtype=np.uint64)
    out = np.zeros(a.size, dtype=np.int32)
    rc = _lib.load().hsk_plan_dispatch(_p(a), a.size, nprocs, 1 if plain else 0, upper_coe, step, _p(out))
    if rc:
        raise HskError(rc)          # "Cannot dispatch tasks. May be too unbalanced." (kmerops.cpp:1319)
    return out


def plan_partition_reads(read_len, nprocs):
    a = np.ascontiguousarray(read_len, dtype=np.uint64)
    out = np.zeros(nprocs, dtype=np.uint64)
    rc = _lib.load().hsk_plan_partition_reads(_p(a), a.size, nprocs, _p(out))
    if rc:
        raise HskError(rc)
    return out


def plan_exchange(nranks, rank, owner, size_matrix):
    """All-to-all-v plan of the supermer exchange for `rank` (see hsk_plan_exchange in include/hsk.h).
    Returns (send_recv [nranks, 8], segs [ntasks, nranks, 4])."""
    owner = np.ascontiguousarray(owner, dtype=np.int32)
    M = np.ascontiguousarray(size_matrix, dtype=np.uint64)
    ntasks = owner.size
    assert M.shape == (nranks, ntasks, 3)
    sr = np.zeros((nranks, 8), dtype=np.uint64)
    segs = np.zeros((ntasks, nranks, 4), dtype=np.uint64)
    rc = _lib.load().hsk_plan_exchange(nranks, rank, ntasks, _p(owner), _p(M), _p(sr), _p(segs))
    if rc:
        raise HskError(rc)
    return sr, segs


# ---- the four reference functions ---------------------------------------------------------------------------
def read_fai(path):
    """Parses <fasta>.fai records: name, length, byte offset of first base, bases per line
    (reference src/fastaindex.cpp:118-123 reads the first four columns)."""
    recs = []
    with open(path) as f:
        for line in f:
            p = line.rstrip("\n").split("\t")
            if len(p) >= 4:
                recs.append((p[0], int(p[1]), int(p[2]), int(p[3])))
    return recs


def read_fai5(path):
    """Same with the line width in bytes (column 5; the reference assumes linebases + 1, src/fastaindex.cpp:285)."""
    recs = []
    with open(path) as f:
        for line in f:
            p = line.rstrip("\n").split("\t")
            if len(p) >= 4:
                recs.append((p[0], int(p[1]), int(p[2]), int(p[3]), int(p[4]) if len(p) >= 5 else int(p[3]) + 1))
    return recs


class DeviceDna:
    """A DnaBuffer that lives in HBM (packed reads + read index), as hsk_pack_fasta / hsk_synth_reads produce it."""

    def __init__(self, ctx, dp, nbytes, do, dl, nreads, first_read_id=0):
        self.ctx, self.dp, self.nbytes, self.do, self.dl, self.nreads, self.first_read_id = ctx, dp, nbytes, do, dl, nreads, first_read_id

    def count(self, rid_base=None):
        return self.ctx.count_device(self.dp, self.nbytes, self.do, self.dl, self.nreads, rid_base=self.first_read_id if rid_base is None else rid_base)

    def count_resident_device(self, rid_base=None):
        """hsk_count_device with the result LEFT IN HBM (Context(keep_device=True)): a DeviceResult."""
        if not self.ctx.keep_device:
            raise ValueError("count_resident_device needs Context(keep_device=True)")
        res = _lib.Result()
        self.ctx._check(self.ctx.lib.hsk_count_device(self.ctx.h, self.dp, self.nbytes, self.do, self.dl, self.nreads,
                                                      self.first_read_id if rid_base is None else rid_base, C.byref(res)))
        return DeviceResult(self.ctx, res)

    def packed(self):
        return self.ctx.d2h(self.dp, self.nbytes) if self.nbytes else np.zeros(0, np.uint8)

    def free(self):
        if self.dp is not None:
            self.ctx.synth_free(self.dp, self.do, self.dl)
            self.dp = None


def read_dna_buffer_device(ctx, fasta_fname, comm=None):
    """FASTA + .fai -> this rank's reads, 2-bit packed ON THE GPU (hsk_pack_fasta): the host only maps the file.
    Same partition of the records over the ranks as read_dna_buffer."""
    recs = read_fai5(fasta_fname + ".fai")
    size = 1 if comm is None else comm.size
    rank = 0 if comm is None else comm.rank
    counts = plan_partition_reads([r[1] for r in recs], size) if size > 1 else np.array([len(recs)], dtype=np.uint64)
    first = int(counts[:rank].sum())
    mine = recs[first:first + int(counts[rank])]
    n = len(mine)
    pos = np.array([r[2] for r in mine], dtype=np.uint64)
    rlen = np.array([r[1] for r in mine], dtype=np.uint32)
    lb = np.array([r[3] for r in mine], dtype=np.uint32)
    lw = np.array([r[4] for r in mine], dtype=np.uint32)
    text = np.zeros(0, dtype=np.uint8)
    if n:
        lo = int(pos.min())
        ends = [int(p) + (((l + b - 1) // b - 1) * w + (l - ((l + b - 1) // b - 1) * b) if b and l else l) for p, l, b, w in zip(pos, rlen.astype(np.int64), lb.astype(np.int64), lw.astype(np.int64))]
        hi = max(ends)
        text = np.memmap(fasta_fname, dtype=np.uint8, mode="r")[lo:hi]
        pos = pos - np.uint64(lo)
    text = np.ascontiguousarray(text)
    dp, do, dl, nb = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
    ctx._check(ctx.lib.hsk_pack_fasta(ctx.h, _p(text) if text.size else None, text.size, _p(pos) if n else None, _p(rlen) if n else None,
                                      _p(lb) if n else None, _p(lw) if n else None, n, C.byref(dp), C.byref(nb), C.byref(do), C.byref(dl)))
    return DeviceDna(ctx, dp.value, int(nb.value), do.value, dl.value, n, first)


def read_dna_buffer(fasta_fname, comm=None):
    """FASTA + .fai -> this rank's DnaBuffer: rank r gets a contiguous run of records chosen by
    FastaIndex::getpartition (reference src/fastaindex.cpp:52-100), 2-bit packed."""
    recs = read_fai(fasta_fname + ".fai")
    size = 1 if comm is None else comm.size
    rank = 0 if comm is None else comm.rank
    counts = plan_partition_reads([r[1] for r in recs], size) if size > 1 else np.array([len(recs)], dtype=np.uint64)
    first = int(counts[:rank].sum())
    mine = recs[first:first + int(counts[rank])]
    buf = DnaBuffer()
    buf.first_read_id = first
    if not mine:
        return buf
    with open(fasta_fname, "rb") as f:
        for _, length, pos, linebases in mine:
            nlines = (length + linebases - 1) // linebases if linebases else 0
            f.seek(pos)
            raw = f.read(length + nlines)
            buf.push_back(raw.replace(b"\n", b"")[:length].decode())
    return buf


_CTX_CACHE = {}


def kmer_count(mydna, comm=None, K=31, M=17, L=15, U=40, EXT=0, ntasks=0, device=None):
    """The path the reference times as "Overall kmer counting (Excluding I/O)" (src/hysortk.cpp:91)."""
    if device is None:
        device = 0 if comm is None else comm.local_rank
    key = (K, M, L, U, EXT, ntasks, device, None if comm is None else id(comm))
    ctx = _CTX_CACHE.get(key)
    if ctx is None:
        ctx = Context(K=K, M=M, L=L, U=U, EXT=EXT, ntasks=ntasks, device=device)
        ctx.comm_init(comm)
        _CTX_CACHE[key] = ctx
    rid_base = 0
    if comm is not None and comm.size > 1:
        rid_base = comm.exscan_sum(mydna.size())        # MPI_Exscan, reference src/kmerops.cpp:65-71
    return ctx.count(mydna, rid_base=rid_base)


def histogram_text(histo):
    """Text of print_kmer_histogram (reference src/hysortk.cpp:122-131); 64-bit bins (the reference's
    int bins overflow beyond 2^31-1 k-mers per count)."""
    lines = ["#count\tnumkmers"]
    for i in range(1, len(histo)):
        if histo[i] > 0:
            lines.append("%d\t%d" % (i, int(histo[i])))
    return "\n".join(lines) + "\n\n"


def paradis_order(kmers, cnt, task_off):
    """The order a PARADIS build of the reference (SORT=1, or SORT=0 without SLURM_TASKS_PER_NODE: src/kmerops.cpp:1330-1360) leaves an
    UNFILTERED task in, for multi-word keys (K > 32; for K <= 32 both sorters give ascending u64).  paradis::sort
    (dependency/Paradis/paradissort.hpp:42-216) partitions by key byte from byte NBYTES-1 down -- the key as a little-endian multi-word
    integer, which is the order this library returns -- and hands every bucket of 2..64 k-mer INSTANCES to std::sort with operator<
    (longs[0] first, include/kmer.hpp:217), buckets of more than 64 to the next byte, nothing below byte 0.  Returns the permutation that
    turns this library's list into that order.  The bucket sizes count instances, so the order of a FILTERED list depends on k-mers the
    filter dropped and cannot be rebuilt from the list (L = 1, U = 65535 only)."""
    kmers = np.asarray(kmers, dtype=np.uint64)
    cnt = np.asarray(cnt, dtype=np.uint64)
    n, nw = kmers.shape
    perm = np.arange(n, dtype=np.int64)
    kb = np.ascontiguousarray(kmers).view(np.uint8).reshape(n, nw * 8)        # byte b of the key = column b (little endian)
    csum = np.concatenate([[0], np.cumsum(cnt.astype(np.int64))])

    def rec(lo, hi, byte):
        col = kb[lo:hi, byte]
        cuts = np.flatnonzero(col[1:] != col[:-1]) + 1
        bounds = [lo] + (cuts + lo).tolist() + [hi]
        if byte == 0:
            return
        for a, b in zip(bounds[:-1], bounds[1:]):
            c = int(csum[b] - csum[a])
            if c > 64:
                rec(a, b, byte - 1)
            elif c > 1 and b - a > 1:
                order = np.lexsort(tuple(kmers[a:b, j] for j in range(nw - 1, -1, -1)))      # operator<: longs[0] most significant
                perm[a:b] = a + order

    for t in range(len(task_off) - 1):
        a, b = int(task_off[t]), int(task_off[t + 1])
        if b - a > 1:
            rec(a, b, nw * 8 - 1)
    return perm


def print_kmer_histogram(kmerlist, comm=None, file=None):
    histo = np.asarray(kmerlist.histo, dtype=np.uint64)
    if comm is not None and comm.size > 1:
        histo = comm.allreduce_sum(histo)                # MPI_Allreduce, reference src/hysortk.cpp:115
    if comm is None or comm.rank == 0:
        (file or sys.stdout).write(histogram_text(histo))
    if comm is not None:
        comm.barrier()


def write_output_file(kmerlist, output_dir, comm=None, ctx=None):
    """<output_dir>/<rank>.out with lines "KMER\\tcount" (reference src/hysortk.cpp:138-164).  With a Context the text is
    formatted on the GPU (hsk_format_entries): spelling 10^8 k-mers on the host takes longer than counting them."""
    rank = 0 if comm is None else comm.rank
    fname = os.path.join(output_dir, "%d.out" % rank)
    try:
        f = open(fname, "wb")
    except OSError:
        raise HskError(1, "cannot open output file " + fname)
    with f:
        if ctx is not None:
            f.write(ctx.format_entries(kmerlist.kmers, kmerlist.cnt))
        else:
            strs = kmerlist.strings()
            f.write("".join("%s\t%d\n" % (s, int(c)) for s, c in zip(strs, kmerlist.cnt)).encode())
