/*
 * hsk.h -- C ABI of libhsk.so, the MI355X (gfx950) k-mer counting hot path.
 *
 * This is the drop-in boundary for the reference's `kmerops` path: everything that
 * hysortk::kmer_count() (reference src/hysortk.cpp:36-96) does between receiving the
 * 2-bit packed DnaBuffer and returning the filtered KmerListS --
 *     prepare_supermer   (reference src/kmerops.cpp:23-127)
 *     exchange_supermer  (reference src/kmerops.cpp:130-195)
 *     filter_kmer        (reference src/kmerops.cpp:198-250)
 * -- runs behind hsk_count() as hand-written HIP kernels.  The C++ shim in
 * include/hysortk/ (same names and layouts as the reference's public headers) and the Python
 * host mirror (hysortk_amd/) both sit on top of exactly these entry points.
 *
 * Rules: plain C, POD only, no exceptions cross the boundary, every function returns an
 * hsk_status (0 = ok).  Buffers returned in hsk_result are owned by the library and released
 * by hsk_result_free().  One hsk_ctx per process and GPU; a ctx is not thread-safe.
 */
#ifndef HSK_H_
#define HSK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSK_ABI_VERSION 4

typedef enum {
    HSK_OK = 0,
    HSK_ERR_INVALID_ARG = 1,   /* bad K/M/L/U/ntasks or NULL pointer (reference: static_assert, compiletime.h:10-22) */
    HSK_ERR_NO_DEVICE = 2,     /* no HIP device / wrong arch: the product path never falls back to a CPU */
    HSK_ERR_HIP = 3,           /* a HIP runtime call failed; see hsk_last_error() */
    HSK_ERR_OOM = 4,           /* device or pinned-host allocation failed */
    HSK_ERR_DISPATCH = 5,      /* "Cannot dispatch tasks. May be too unbalanced." (reference kmerops.cpp:1319) */
    HSK_ERR_INTERNAL = 6,      /* device-side consistency check failed (e.g. look-back timeout) */
    HSK_ERR_COMM = 7,          /* RCCL not available / collective failed */
    HSK_ERR_UNSUPPORTED = 8    /* valid in the reference, not built yet here */
} hsk_status;

/* Runtime form of the reference's compile-time macros (reference Makefile:1-46). */
typedef struct {
    int32_t kmer_size;        /* KMER_SIZE        2 < K < 96, K % 32 != 0 (reference UB, kmer.hpp:260) */
    int32_t minimizer_size;   /* MINIMIZER_SIZE   0 < M < K, M % 32 != 0 (one-, two- and three-word minimizers) */
    int32_t lower_freq;       /* LOWER_KMER_FREQ  1 <= L <= U */
    int32_t upper_freq;       /* UPPER_KMER_FREQ  U <= 65535 */
    int32_t extension;        /* EXTENSION        0 | 1: carry (PosInRead, ReadId) through the sort */
    int32_t ntasks;           /* tot_tasks of prepare_supermer (kmerops.cpp:40-43,76); 0 = pick for the GPU */
    int32_t device;           /* HIP device ordinal */
    int32_t plain_dispatcher; /* PLAIN_DISPATCHER: 1 = round robin, 0 = balanced (kmerops.cpp:115-119) */
    double  dispatch_upper_coe; /* DISPATCH_UPPER_COE (1.5) */
    double  dispatch_step;      /* DISPATCH_STEP      (0.05) */
    int32_t radix_bits;       /* digit width of the full-width LSD radix plan: 4 .. 8, 0 = 8 (default 8; narrower = more passes) */
    int32_t flags;            /* HSK_FLAG_* */
    double  unbalanced_ratio; /* UNBALANCED_RATIO (2.3): a task is a heavy hitter above ratio x the mean task (kmerops.cpp:1190); ABI 3 */
    const char *tuning;       /* ABI 4 (was reserved[0]): NULL, or "name=value,name=value": forced paths for tests and a few measured thresholds, read per
                                 context (rounds 1-3: process-wide environment variables).  Copied by hsk_init. */
    int64_t reserved[2];
} hsk_config;

#define HSK_FLAG_PROFILE      1   /* HIP-event timing of every radix scatter launch (hsk_stats) */
#define HSK_FLAG_KEEP_DEVICE  2   /* hsk_count_device leaves the result in HBM (entries_dev) */
#define HSK_FLAG_PLAIN_CLASSIFIER 4 /* PLAIN_CLASSIFIER: no heavy-hitter pre-aggregation (kmerops.cpp:109-113) */
/* Which algorithm orders and counts the k-mers of a task (ABI 3).  Default: two radix scatter passes on the top 16 key bits,
 * then one LDS hash aggregation per 16-bit prefix bin -- the fast plan for sequencing data, where every k-mer repeats about
 * `coverage` times; the library leaves it by itself when the input turns out to hold (nearly) only unique k-mers. */
#define HSK_FLAG_NO_AGGREGATION 8   /* never aggregate in LDS tables: four scatter passes on the top 32 bits + an in-LDS finish per
                                       tile (one-word keys), the full sort below for every other record shape */
#define HSK_FLAG_NO_COMBINE     32   /* never take the combining extraction (one GPU, one-word keys, no payload, from 64 MB of packed reads on:
                                       the supermers are ordered by minimizer bucket, every bucket's k-mers are counted in an LDS table where
                                       they are extracted, and only the {k-mer, count} pairs enter the passes above); the library leaves it by
                                       itself when the input yields more than one pair per sixteen k-mers (reads with ~0.2 % errors and more, coverage below ~20) */
#define HSK_FLAG_FULL_SORT     16   /* the reference's own algorithm: LSD radix sort over ALL key bytes of every task
                                       (sort_task, kmerops.cpp:1382) + adjacent-equal merge-count over the sorted array
                                       (count_sorted_kmers, kmerops.cpp:1410); nothing fused, nothing skipped */

typedef struct hsk_ctx hsk_ctx;

/*
 * Result of one hsk_count(): the rank-local KmerListS.
 *   entries: n records of (nw + 1) uint64 = { TKmer longs[nw]; uint64_t cnt } -- byte-identical
 *            to the reference's KmerListEntryS for EXTENSION == 0 (kmer.hpp:368-383), so the
 *            C++ shim memcpy's it into std::vector<KmerListEntryS>.
 *   order:   ascending task id over the tasks this rank owns (copy_results, kmerops.cpp:883-904);
 *            inside a task ascending as a little-endian multi-word integer (= sort_task,
 *            kmerops.cpp:1382, RADULS order; for K <= 32 this is plain ascending uint64).
 *   EXTENSION == 1: entry i owns pos/rid[payload_off[i] .. payload_off[i] + cnt_i): its slice of the
 *            task's sorted payload array (slices of filtered-out k-mers stay in pos/rid as unused
 *            gaps; payload_off[n] = total payload length).
 */
typedef struct {
    uint64_t n;               /* number of (k-mer, count) entries */
    int32_t  nw;              /* 64-bit words per k-mer: 1 (K<=32), 2 (K<=64), 3 (K<=95) */
    int32_t  ntasks;          /* tot_tasks actually used */
    uint64_t *entries;        /* host (pinned) n * (nw+1) words; NULL with HSK_FLAG_KEEP_DEVICE */
    uint64_t *task_off;       /* host, ntasks+1: entry range of each task id (empty if not owned) */
    uint64_t *payload_off;    /* host, n+1 (EXTENSION): first payload of entry i; [n] = length of pos/rid */
    uint32_t *pos;            /* host, payload_off[n] values (EXTENSION): PosInRead */
    int32_t  *rid;            /* host, payload_off[n] values (EXTENSION): ReadId */
    uint64_t *histo;          /* host, histo_len bins: histo[c] = #entries with cnt == c */
    uint64_t histo_len;
    void     *entries_dev;    /* device copy when HSK_FLAG_KEEP_DEVICE (owned by the ctx) */
    /* --- measurements of this call --- */
    uint64_t total_kmers;     /* k-mer instances of this rank's tasks (after the exchange; a heavy-hitter task's, which arrive as lists, incl.),
                                 plus the instances this rank's scan left out as certain to be dropped (hsk_stats::dropped_kmers): over the
                                 ranks they add up to the k-mers of the input */
    uint64_t total_supermers;
    uint64_t total_supermer_bytes;
    double   ms_total;        /* device time of the whole path (HIP events) */
    double   ms_parse;        /* minimizer/supermer kernels */
    double   ms_exchange;     /* RCCL all-to-all (0 on one GPU) */
    double   ms_extract;      /* supermer -> canonical k-mer kernels */
    double   ms_sort;         /* histogram + all radix passes */
    double   ms_count;        /* merge-count + filter */
    double   ms_d2h;          /* result copy to the host */
    void    *priv;            /* library bookkeeping */
} hsk_result;

/* Per-kernel accounting (HIP events on the launch stream around every launch of the named kernels), filled when
 * HSK_FLAG_PROFILE is set.  bytes = algorithmic bytes (records read + written). */
typedef struct {
    uint64_t scatter_launches;
    uint64_t scatter_keys;        /* sum over launches of keys moved */
    uint64_t scatter_bytes;       /* sum over launches of 2 * record_bytes * keys */
    double   scatter_ms;          /* sum of launch durations (HIP events on the launch stream) */
    uint64_t hist_launches;
    uint64_t hist_bytes;
    double   hist_ms;
    int64_t  fused_tasks;         /* tasks finished by a fused finish kernel (aggregating or tile finish) */
    int64_t  redone_tasks;        /* tasks the hybrid path had to redo with the full-width passes */
    uint64_t agg_launches;        /* aggregating finish kernel (hsk_agg.h): launches, record bytes read, duration */
    uint64_t agg_bytes;
    double   agg_ms;
    int64_t  agg_retried_tasks;   /* tasks that needed the large hash table (a bin with many distinct keys) */
    int64_t  parse_fallbacks;     /* parses that left the fast path (a tile with more supermers than the record capacity) */
    int64_t  heavy_tasks;         /* heavy-hitter tasks this rank pre-aggregated and shipped as k-mer lists (multi-GPU) */
    int64_t  dropped_kmers;       /* k-mer instances the scan left out because their k-mer -- the all-A or the all-C k-mer -- has more than U copies inside the
                                     plan's sample alone and so cannot be in the result (round 4; the field was `onepass_misses`, always 0, before) */
    /* --- ABI 2 --- */
    uint64_t scan_launches;       /* scan_kernel (minimizers + supermer records): launches, packed read bytes, duration */
    uint64_t scan_bytes;
    double   scan_ms;
    uint64_t place_launches;      /* place_kernel (supermers to their task slots): launches, supermers placed, duration */
    uint64_t place_supermers;
    double   place_ms;
    uint64_t host_syncs;          /* blocking waits of the host on the GPU (stream or event) inside hsk_count* since the last reset */
    uint64_t host_waits_covered;  /* ... of which the host had already enqueued the next batch's kernels behind the awaited work,
                                     so the wait does not leave the GPU idle */
    uint64_t h2d_bytes;           /* hsk_count(): input bytes copied (or read in place over PCIe) from the host */
    uint64_t d2h_bytes;           /* result bytes copied to the host */
    double   h2d_ms;              /* duration of the input copies (0 when the parse reads pinned host memory in place) */
    double   d2h_ms;              /* duration of the result copies, whether or not they overlapped the kernels */
    /* --- ABI 3, combining extraction (hsk_combine.h) --- */
    uint64_t bucket_launches;     /* bucket order of the supermer items (histogram + scatter launches), items moved, duration */
    uint64_t bucket_items;
    double   bucket_ms;
    uint64_t combine_launches;    /* combine_kernel: launches, k-mers counted in LDS tables, {k-mer, count} pairs written, duration */
    uint64_t combine_kmers;
    uint64_t combine_pairs;
    double   combine_ms;
    /* --- appended in ABI 4: prefix bins of very many records (one k-mer seen millions of times) that many workgroups counted slice by slice --- */
    uint64_t agg_large_bins;      /* such bins counted through their slices since the last reset (a bin that turned out to hold too many distinct
                                     k-mers for that and was counted by its own workgroup after all is not among them) */
    uint64_t agg_large_slices;    /* slices of those bins */
    /* --- appended in ABI 4: equal supermer items of a unit are rolled once (tuning combine_dedup, hsk_combine.h) --- */
    uint64_t combine_items;           /* supermer items combine_kernel read */
    uint64_t combine_distinct_items;  /* items whose k-mers it rolled: the distinct items of its item tables and the items that went past them;
                                         equal to combine_items when combine_dedup=0 and for two-word keys */
} hsk_stats;

/* ---- lifecycle ------------------------------------------------------------------------- */
int  hsk_abi_version(void);
int  hsk_device_count(void);                       /* HIP devices visible to this process (0 if none / no driver) */
/* Pinned (page-locked) host memory for the DnaBuffer handed to hsk_count(): such a buffer is read by the GPU in place, the
 * transfer overlaps the minimizer scan.  Pageable memory works too (staged copies first).  NULL when the allocation fails. */
void *hsk_host_alloc(uint64_t bytes);
void  hsk_host_free(void *p);
int  hsk_init(const hsk_config *cfg, hsk_ctx **out);
void hsk_destroy(hsk_ctx *ctx);
const char *hsk_strerror(int status);
const char *hsk_last_error(const hsk_ctx *ctx);   /* detail text of the last failure */
void hsk_config_default(hsk_config *cfg);          /* reference Makefile defaults: K=31 M=17 L=15 U=40 */

/* ---- the hot path ---------------------------------------------------------------------- */
/*
 * hsk_count: replaces prepare_supermer + exchange_supermer + filter_kmer for the reads of
 * this rank.  Input is the reference's DnaBuffer memory as is (dnabuffer.hpp:14, dnaseq.hpp:33):
 *   packed        2-bit bases, 4 per byte, first base in the two MSBs; every read starts on a
 *                 byte boundary
 *   read_byte_off nreads offsets into packed (DnaBuffer::getbufoffset)
 *   read_len      nreads lengths in bases (DnaSeq::size)
 *   rid_base      global id of read 0 (reference: MPI_Exscan of read counts, kmerops.cpp:65-71)
 * Collective over the communicator when hsk_comm_init() has been called.
 */
int hsk_count(hsk_ctx *ctx, const uint8_t *packed, uint64_t packed_bytes,
              const uint64_t *read_byte_off, const uint32_t *read_len, uint64_t nreads,
              int64_t rid_base, hsk_result *out);

/* Same, inputs already resident in HBM (d_read_byte_off has nreads entries). */
int hsk_count_device(hsk_ctx *ctx, const void *d_packed, uint64_t packed_bytes,
                     const void *d_read_byte_off, const void *d_read_len, uint64_t nreads,
                     int64_t rid_base, hsk_result *out);

/* Test/diagnostic entry: `nranks` VIRTUAL ranks on the one GPU of this ctx.  Runs the multi-GPU data path
 * (task-size probe, dispatch, owner-grouped parse, byte packing, all-to-all-v plan, multi-segment extraction)
 * with device-to-device copies in place of the RCCL send/recv; outs[r] is what rank r would return.
 * owner_out (optional, capacity in entries) receives the task -> rank table. */
int hsk_count_loopback(hsk_ctx *ctx, int nranks, const uint8_t *const *packed, const uint64_t *packed_bytes,
                       const uint64_t *const *read_byte_off, const uint32_t *const *read_len, const uint64_t *nreads,
                       hsk_result *outs, int32_t *owner_out, int32_t owner_capacity);

/* The same with every virtual rank's reads already resident in HBM (d_read_byte_off[r] has nreads[r] entries): full-size runs of the
 * multi-rank data path on one GPU.  outs[r].ms_parse / ms_exchange / ms_extract / ms_sort / ms_count / ms_total are rank r's device
 * times (the virtual ranks run one after the other). */
int hsk_count_loopback_device(hsk_ctx *ctx, int nranks, const void *const *d_packed, const uint64_t *packed_bytes,
                              const void *const *d_read_byte_off, const void *const *d_read_len, const uint64_t *nreads,
                              hsk_result *outs, int32_t *owner_out, int32_t owner_capacity);

/* ctx == NULL is allowed when the context is already destroyed: a result outlives its context (its pinned host blocks belong to the
 * result; hsk_destroy frees only the context's cache of released blocks). */
void hsk_result_free(hsk_ctx *ctx, hsk_result *res);
/* HSK_FLAG_KEEP_DEVICE: where task `task`'s share of the result lives in HBM -- entries (n records of nw + 1 words), and with
 * EXTENSION the CSR payload: payload_off (n values in the rank's payload numbering), pos / rid (npay values each, the
 * task's whole sorted payload) and payload_base: entry i owns pos / rid[payload_off[i] - payload_base ...][0 .. cnt_i).
 * A downstream GPU stage (e.g. an overlap detector consuming (ReadId, PosInRead) lists, reference README.md:52,74) reads
 * them in place; the memory belongs to the result. */
int hsk_result_device_task(const hsk_result *res, int32_t task, const void **entries, uint64_t *n,
                           const void **payload_off, const void **pos, const void **rid, uint64_t *npay, uint64_t *payload_base);
/*
 * Read pairs that share k-mers (what a client such as ELBA builds from the (ReadId, PosInRead) lists, reference README.md:52,74),
 * computed on the GPU from a result that was left there: HSK_FLAG_KEEP_DEVICE and EXTENSION, tasks [task_lo, task_hi).
 *
 * Definition.  Every entry of those tasks (a retained k-mer, L <= cnt <= U) has cnt occurrences (rid, pos), which form
 * cnt (cnt - 1) / 2 unordered occurrence pairs.  A pair whose two occurrences lie in the same read is dropped (the k-mer occurs twice
 * in that read); every other pair is one RECORD
 *     key   = rid_a << 32 | rid_b      rid_a < rid_b, both read as unsigned 32-bit numbers
 *     value = pos_a << 32 | pos_b      pos_a = the position in read rid_a.
 * The records are grouped by key.  The list has one ROW of four uint64 words per key with at least min_shared records, in
 * ascending key order:
 *     { key, shared, first, last }     shared = records with that key, first / last = the smallest / largest value of the run
 * (as 64-bit numbers: ordered by pos_a, then pos_b).  Minimum and maximum do not depend on the order of the payload inside an
 * entry, which is unspecified.  There is NO STRAND in a row: the payload carries none, so a pair of reads that overlap on opposite
 * strands is told from one on the same strand only by the way pos_b runs against pos_a, which first and last bracket
 * (hsk_result_strands and hsk_result_pairs_oriented, below, recover the strand from the reads and split the rows by it).
 *
 * Several lists (the multi-rank contract).  The lists of disjoint task ranges combine to the list of their union, and so do the
 * lists of the ranks of a several-GPU run (every k-mer belongs to one task and every task to one rank): rows with equal keys
 * join -- shared adds up, first is the minimum, last the maximum -- and min_shared is applied AFTER that (compute the parts with
 * min_shared = 1).  The call itself is rank-local and not collective; nothing is exchanged between the ranks here.
 *
 * Memory: two key and two value buffers of `records` 8-byte words plus the rows.  `records` is known after one counting pass and
 * before any of them is allocated: HSK_ERR_OOM then says how many records and bytes, and a narrower task range is the way out --
 * or hsk_result_pairs_sliced (below), which computes the same list from as many records at a time as the caller allows.
 * HSK_ERR_INVALID_ARG: a NULL pointer, a result that was not left on the device, a context without EXTENSION, a task range outside
 * [0, ntasks], min_shared == 0.  An empty range is no error (n = 0).  hsk_pairs_free before hsk_destroy of the context.
 */
typedef struct {
    uint64_t n;             /* rows */
    uint64_t *rows;         /* host (pinned), n * 4 words; NULL when left on the device */
    void     *rows_dev;     /* device copy when asked for */
    uint64_t records;       /* occurrence pairs expanded, same-read ones included */
    uint64_t self_records;  /* of which dropped: both occurrences in one read */
    uint64_t keys;          /* distinct read pairs before min_shared */
    int32_t  sort_passes;   /* scatter passes the key sort took (-1: not known) */
    double   ms_expand, ms_sort, ms_reduce, ms_d2h, ms_total;   /* HIP events */
    void    *priv;
} hsk_pairs;

int  hsk_result_pairs(hsk_ctx *ctx, const hsk_result *res, int32_t task_lo, int32_t task_hi,
                      uint32_t min_shared, int32_t on_device, hsk_pairs *out);
void hsk_pairs_free(hsk_ctx *ctx, hsk_pairs *p);
/*
 * The same list within a memory budget.  hsk_result_pairs_sliced has the definition, the row order and the refusals of
 * hsk_result_pairs, and expands at most max_records records at a time: the record array of the task range is cut at entry boundaries
 * into SLICES of at most max_records records, every slice is expanded, sorted and reduced to a row list of its own (32 bytes per
 * record of the slice while that runs), and the lists are merged on the device (rows with equal keys join, as in the several-list
 * contract above; min_shared is applied by the last merge).  The memory at the peak is 32 bytes x the largest slice plus the row
 * lists: up to three times 32 bytes x the rows of the result while the last merge runs.
 *   max_records  the budget.  A slice holds at least one entry: an entry with more records than the budget (cnt (cnt - 1) / 2 of them,
 *                2 147 385 345 at most) is a slice of its own, and info->peak_records says how large the largest slice was.  When that
 *                allocation fails the error is the HSK_ERR_OOM of hsk_result_pairs.  A budget of at least `records` runs
 *                hsk_result_pairs' single pass (info->slices == 1).
 *                0 = the library chooses: 1/96 of the device memory the context can still get when the record count is known (what the
 *                runtime reports free plus what the context's pool holds unused), in records -- a third of that memory for the 32 bytes
 *                per record, the rest for the row lists and the merges.
 *   out          records and self_records are the sums over the slices, keys the distinct keys of the merged list before min_shared,
 *                sort_passes the most any slice's sort took, ms_expand / ms_sort / ms_reduce the sums over the slices, ms_total the call.
 *   info         may be NULL.
 * The limit of 2^31 expansion tiles holds per slice, not per range.
 */
typedef struct {
    uint64_t slices;        /* record windows expanded (1 = the unsliced path ran) */
    uint64_t peak_records;  /* largest window: max(max_records, the largest single entry's records) at most */
    uint64_t merges;        /* merge launches (COUNT + EMIT = one) */
    uint64_t merged_rows;   /* input rows read by all merges */
    double   ms_merge;      /* HIP events around the merges */
    int64_t  reserved[4];
} hsk_pairs_slices;

int  hsk_result_pairs_sliced(hsk_ctx *ctx, const hsk_result *res, int32_t task_lo, int32_t task_hi, uint32_t min_shared,
                             int32_t on_device, uint64_t max_records, hsk_pairs *out, hsk_pairs_slices *info);
/*
 * The several-list contract on the GPU: the list of the union of `nparts` lists that were computed with min_shared = 1 (disjoint task
 * ranges, or the ranks of a several-GPU run).  Of each part the call reads n, rows_dev if set or else rows (host memory, pageable or
 * pinned), records and self_records; its priv may be NULL, so a part may be a struct the caller filled in for rows of its own.
 * rows_dev must be 16-byte aligned (every list of this library is).  Host lists are uploaded, the lists are merged two at a time on the
 * device -- ascending keys, a key at most once per list: a two-way merge that reads and writes every row once per merge, in the order
 * of a binary counter, so that no row goes through more than ceil(log2(nparts)) + 1 merges -- and min_shared is applied by the last
 * merge.  out is an ordinary hsk_pairs (host rows, or device rows with on_device), freed by hsk_pairs_free: n, rows, records and
 * self_records (the sums), keys (before min_shared), ms_reduce (the merges), ms_d2h, ms_total.  The parts are left as they are.
 * Needs neither EXTENSION nor a resident result.  HSK_ERR_INVALID_ARG: a NULL pointer, nparts < 0, min_shared == 0, a part with n > 0
 * and no rows.  nparts == 0, or parts that are all empty, give an empty list.
 */
int  hsk_pairs_merge(hsk_ctx *ctx, const hsk_pairs *const *parts, int32_t nparts, uint32_t min_shared, int32_t on_device, hsk_pairs *out);
/*
 * The strand of every k-mer occurrence of a result that was left on the device (HSK_FLAG_KEEP_DEVICE and EXTENSION), recovered from the
 * reads the result was counted from: the payload (ReadId, PosInRead) carries no strand, but the entry holds the canonical k-mer, and the
 * read's K bases at the position spell either it or its reverse complement.
 *
 * Definition.  For entry e of task t and each of its cnt_e payload slots s (indices into the task's pos / rid arrays, as
 * hsk_result_device_task describes them: s = payload_off[e] - payload_base + 0 .. cnt_e - 1), the read rid[s] - rid_base has K bases at
 * pos[s], in the packed bytes exactly as hsk_count reads them: base i of a read in byte i / 4 of the read at shift 6 - 2 (i % 4).  Put into
 * the layout of the entry's k-mer words (base i in word i / 32 at shift 2 (31 - i % 32)) they are the word f.  f equals the entry's k-mer:
 * strand 0; else the reverse complement of f (Kmer::GetTwin, kmer.hpp:266-296) equals it: strand 1.  Equality with the entry is tested
 * first, so a k-mer that is its own reverse complement (even K only) has strand 0; such occurrences are counted in `palindromes`.
 *
 * Output.  One device array of (npay + 63) / 64 uint64 words per task (hsk_strands_task): bit s & 63 of word s >> 6 is the strand of slot
 * s.  Slots that belong to no entry -- the gaps that filtered k-mers leave -- have bit 0 and are never read as (rid, pos).  The arrays
 * belong to the hsk_strands: hsk_strands_free before hsk_destroy of the context.
 *
 *   packed, read_byte_off, read_len, nreads, rid_base   the reads as hsk_count / hsk_count_device took them; reads_on_device != 0: the
 *                three arrays are device memory (what hsk_count_device, hsk_pack_fasta and hsk_synth_reads leave in HBM; packed 4-byte
 *                aligned), else host memory that is uploaded for the call.  No byte at or beyond packed_bytes is read.
 * The call is rank-local: a rank of a several-GPU run is given the reads its payload names (a payload that names another read is the
 * out-of-range refusal below).
 * HSK_ERR_INVALID_ARG, with a hsk_last_error text that names the case, the context usable afterwards: a NULL pointer; a context without
 * EXTENSION; a result that was not left on the device; rid_base + nreads > 2^31; an owned slot whose rid lies outside
 * [rid_base, rid_base + nreads); an owned slot with pos + K > read_len; a read of the index outside the packed bytes; an owned slot whose
 * bases are neither the entry's k-mer nor its reverse complement ("these are not the reads the result was counted from").
 */
typedef struct {
    int32_t  ntasks;
    uint64_t payloads;     /* payload slots owned by entries of the result (sum of cnt) */
    uint64_t reverse;      /* of which strand 1 */
    uint64_t palindromes;  /* occurrences whose k-mer is its own reverse complement (even K only); strand 0 */
    double   ms_total;     /* HIP events */
    int64_t  reserved[4];
    void    *priv;
} hsk_strands;

int  hsk_result_strands(hsk_ctx *ctx, const hsk_result *res,
                        const void *packed, uint64_t packed_bytes, const void *read_byte_off, const void *read_len,
                        uint64_t nreads, int64_t rid_base, int32_t reads_on_device, hsk_strands *out);
/* task `task`'s bit words in HBM (NULL when the task has no payload) and the number of its payload slots */
int  hsk_strands_task(const hsk_strands *s, int32_t task, const void **bits_dev, uint64_t *npay);
void hsk_strands_free(hsk_ctx *ctx, hsk_strands *s);
/*
 * Read pairs split by relative strand.  hsk_result_pairs_oriented has the definition, the refusals, the memory rules and the slicing of
 * hsk_result_pairs_sliced (max_records: 0 lets the library choose, a budget of at least `records` -- UINT64_MAX -- is the single pass), with
 * one difference: the record of an occurrence pair (i, j) of two different reads has
 *     key = o << 63 | rid_a << 32 | rid_b        o = strand_i XOR strand_j   (`strands`: hsk_result_strands of the same result)
 * Read ids are below 2^31 here (hsk_result_strands has refused anything else), so bit 63 is free.  The list has all same-strand rows first
 * and all opposite-strand rows behind them, each half in ascending (rid_a, rid_b); key & ~(1 << 63) is the key hsk_result_pairs gives.
 * A pair inside one read is still key 0 and counted in self_records, whatever its strands; keys counts distinct (read pair, orientation).
 * Seeds of a same-strand overlap and of a reverse-complement overlap of two reads thus arrive as two rows, each with its own shared count
 * and first / last bracket.
 * Folding property.  Clearing bit 63 and joining equal keys -- shared adds up, first is the minimum, last the maximum, min_shared applied
 * afterwards -- gives exactly the list of hsk_result_pairs for the same task range.
 * Oriented lists of disjoint task ranges or of several ranks combine through hsk_pairs_merge as they are: bit 63 is part of the key.
 * HSK_ERR_INVALID_ARG also for a NULL `strands` and for one that does not belong to `res` (ntasks and every task's payload slots are compared).
 */
int  hsk_result_pairs_oriented(hsk_ctx *ctx, const hsk_result *res, const hsk_strands *strands,
                               int32_t task_lo, int32_t task_hi, uint32_t min_shared, int32_t on_device,
                               uint64_t max_records, hsk_pairs *out, hsk_pairs_slices *info);
/*
 * Read pairs by diagonal: the seed bins of every oriented read pair, and the best-supported one (what a client of the BELLA kind does
 * next with the oriented rows: bin a pair's seeds by diagonal, keep the bin with the most seeds, start the alignment from a seed of it).
 *
 * Definition.  The RECORDS are exactly those of hsk_result_pairs_oriented for the same result, strands and task range:
 *     key   = o << 63 | rid_a << 32 | rid_b        value = pos_a << 32 | pos_b
 * a pair inside one read is no record and counted in self_records.  Every record has a diagonal number
 *     D = pos_a - pos_b + 2^32   (o = 0)           D = pos_a + pos_b   (o = 1)
 * in 64-bit arithmetic, never negative -- seeds of a same-strand overlap keep the difference of their positions, seeds of a
 * reverse-complement overlap keep the sum; no read length is needed -- and a bin
 *     bin = D / diag_bin                           (unsigned integer division).
 * The records of a key fall into bins.  A ROW has six uint64 words (48 bytes; the lists are 16-byte aligned):
 *     { key, shared, bin, support, first, last }
 *   all_bins == 0   the list by best bin, one row per key: shared = the records of the key over all its bins (the `shared` of the oriented
 *                   list); bin = the bin with the most records, among equal counts the smallest bin; support = its records; first / last =
 *                   the smallest / largest value among the records of THAT bin only.  Rows with support < min_support are dropped after
 *                   the selection.  The row order is that of the oriented list.
 *   all_bins != 0   the list before the selection, one row per (key, bin) in ascending (key, bin): shared = support = the records of the
 *                   bin, first / last over the bin; min_support is applied per row.
 * Selection property.  The first list is a pure function of the second (computed with min_support = 1): per key, shared is the sum of
 * support, the row with the largest support is kept -- on a tie the one with the smallest bin -- and min_support is applied afterwards.
 *
 * Several lists.  The ALL-BINS lists of disjoint task ranges, or of the ranks of a several-GPU run, join on (key, bin): support (and
 * shared) add up, first is the minimum, last the maximum; the selection then runs on the joined list.  Compute the parts with
 * min_support = 1.  The best-bin lists themselves DO NOT combine: the best bin of a part need not be the best bin of the union.
 * hsk_pair_diags_merge (below) is that join and selection on the GPU; hsk_result_pair_diagonals_sliced (below) computes either list of a
 * task range from as many records at a time as the caller allows, through the same join.
 *
 *   diag_bin      the bin width W, 1 .. 2^31
 *   out           records, self_records as hsk_result_pairs_oriented; keys = distinct (read pair, orientation) before min_support; bins =
 *                 distinct (key, bin) before min_support; sort_passes = scatter passes of the sort over the two-word key (pair key, bin)
 *                 (-1: not known); ms_* HIP events (ms_expand includes the record count, ms_reduce both reducers).
 * Memory: 48 bytes per record while the sort runs (two buffers of two-word keys and two of values); then 48 bytes per distinct (key, bin)
 * for the bin rows, beside the record buffers while they are written, and 48 bytes per row of the result.  `records` is known after one
 * counting pass and before the record buffers are asked for: HSK_ERR_OOM then says how many records and bytes, and
 * hsk_result_pair_diagonals_sliced (below) is the way out: the same list from fewer records at a time.  `bins` is known after
 * the reducer's count pass, before the bin rows are asked for.
 * HSK_ERR_INVALID_ARG, with a hsk_last_error text, the context usable afterwards: everything hsk_result_pairs_oriented refuses (a NULL
 * pointer, `strands` NULL or not of `res`, a result that was not left on the device, a context without EXTENSION, a task range outside
 * [0, ntasks]); diag_bin == 0 or diag_bin > 2^31; min_support == 0.  An empty range is no error (n = 0).
 * hsk_pair_diags_free before hsk_destroy of the context.
 */
typedef struct {
    uint64_t n;             /* rows */
    uint64_t *rows;         /* host (pinned), n * 6 words; NULL when left on the device */
    void     *rows_dev;     /* device copy when asked for */
    uint64_t records;       /* occurrence pairs expanded, same-read ones included */
    uint64_t self_records;  /* of which dropped: both occurrences in one read */
    uint64_t keys;          /* distinct (read pair, orientation) before min_support */
    uint64_t bins;          /* distinct (key, bin) before min_support */
    int32_t  sort_passes;   /* scatter passes the sort took (-1: not known) */
    double   ms_expand, ms_sort, ms_reduce, ms_d2h, ms_total;   /* HIP events */
    int64_t  reserved[4];
    void    *priv;
} hsk_pair_diags;

int  hsk_result_pair_diagonals(hsk_ctx *ctx, const hsk_result *res, const hsk_strands *strands,
                               int32_t task_lo, int32_t task_hi, uint64_t diag_bin, uint32_t min_support,
                               int32_t all_bins, int32_t on_device, hsk_pair_diags *out);
void hsk_pair_diags_free(hsk_ctx *ctx, hsk_pair_diags *d);
/*
 * The same lists within a memory budget.  hsk_result_pair_diagonals_sliced has the definition, the row order, the refusals and the results
 * of hsk_result_pair_diagonals, whatever the budget, and expands at most max_records records at a time: the record array of the task range
 * is cut at entry boundaries into SLICES, as hsk_result_pairs_sliced cuts it; the bound of the positions is taken once for the range, so
 * every slice sorts the same word; every slice is expanded, sorted and reduced to an all-bins list of its own with min_support 1 (48 bytes
 * per record of the slice while that runs); and the lists are merged on the device on the two-word key (key, bin) -- rows with equal
 * (key, bin) join, as in the several-list contract above.  all_bins != 0: the last merge applies min_support.  all_bins == 0: every merge
 * keeps every row, and the selection runs over the joined list and applies min_support; best-bin lists of slices are never merged.
 * The memory at the peak is 48 bytes x the largest slice plus the bin-row lists: up to three times 48 bytes x the joined list while the
 * last merge runs.
 *   max_records  the budget, with the meaning it has in hsk_result_pairs_sliced: a slice holds at least one entry, an entry above the
 *                budget is a slice of its own, a budget of at least `records` runs hsk_result_pair_diagonals' single pass
 *                (info->slices == 1).  0 = the library chooses: 1/144 of the device memory the context can still get when the record
 *                count is known, in records -- a third of that memory at 48 bytes per record.
 *   out          records and self_records are the sums over the slices, keys and bins those of the joined list before min_support,
 *                sort_passes the most any slice's sort took, ms_expand / ms_sort / ms_reduce the sums over the slices, ms_total the call.
 *   info         may be NULL; filled as hsk_result_pairs_sliced fills it.
 * The limit of 2^31 expansion tiles holds per slice, not per range.
 */
int  hsk_result_pair_diagonals_sliced(hsk_ctx *ctx, const hsk_result *res, const hsk_strands *strands,
                                      int32_t task_lo, int32_t task_hi, uint64_t diag_bin, uint32_t min_support,
                                      int32_t all_bins, int32_t on_device, uint64_t max_records,
                                      hsk_pair_diags *out, hsk_pairs_slices *info);
/*
 * The several-list contract of the diagonals on the GPU: the list of the union of `nparts` ALL-BINS lists that were computed with
 * min_support = 1 and one diag_bin (disjoint task ranges, or the ranks of a several-GPU run).  Of each part the call reads n, rows_dev if
 * set or else rows (host memory, pageable or pinned; uploaded), records and self_records; its priv may be NULL.  rows_dev must be 16-byte
 * aligned (every list of this library is).  The lists -- ascending (key, bin), a (key, bin) at most once per list -- are merged two at a
 * time on the device in the order of a binary counter, as hsk_pairs_merge merges its lists, and the last merge counts keys and bins of
 * the joined list (a single list goes through one merge with nothing for these counts).
 *   all_bins != 0   the joined list; min_support is applied by the last merge.
 *   all_bins == 0   the selection runs on the joined list, min_support is applied after it: with nparts == 1 this is the selection
 *                   property on the device.
 * out is an ordinary hsk_pair_diags (host rows, or device rows with on_device), freed by hsk_pair_diags_free: n, rows, records and
 * self_records (the sums), keys and bins (of the joined list, before min_support), ms_reduce (the merges and the selection), ms_d2h,
 * ms_total.  The parts are left as they are.  Needs neither EXTENSION nor a resident result.  Memory: the uploaded parts, and up to three
 * times 48 bytes x the joined list while the last merge runs.  HSK_ERR_INVALID_ARG: a NULL pointer, nparts < 0, min_support == 0, a part
 * with n > 0 and no rows, a rows_dev that is not 16-byte aligned.  nparts == 0, or parts that are all empty, give an empty list.
 */
int  hsk_pair_diags_merge(hsk_ctx *ctx, const hsk_pair_diags *const *parts, int32_t nparts, uint32_t min_support,
                          int32_t all_bins, int32_t on_device, hsk_pair_diags *out);
/*
 * Ungapped x-drop overlaps: the seed of every diagonal row, extended in both directions over the reads in HBM.  One overlap row per
 * input row; exact integer work, held to this definition word for word (csrc/hsk_xdrop.h is the one implementation the kernels, the
 * host and the CPU tests share; tests/extend_ref.py spells it base by base).
 *
 * Input.  A list of hsk_pair_diags rows, best-bin or all-bins: of `in` the call reads n, rows_dev if set, else rows (host memory,
 * pageable or pinned; uploaded as hsk_pair_diags_merge uploads its parts); its priv may be NULL, so a list the caller filled in by hand is
 * valid.  The reads as hsk_result_strands takes them (packed, packed_bytes, read_byte_off, read_len, nreads, rid_base, reads_on_device).
 * K is the context's.  Needs neither EXTENSION nor a resident result.
 *
 * Seed.  For each row: pa = first >> 32, pb = first & 0xffffffff, o = key >> 63; the reads a = rid_a - rid_base, b = rid_b - rid_base with
 * lengths la, lb; base codes as the packed bytes hold them (N is A; base i of a read in byte i / 4 at shift 6 - 2 (i % 4)).
 *
 * Columns.  Column t (t = 0: the seed's first base in A's forward direction) pairs
 *     o = 0:  A[pa + t] with B[pb + t];                valid t in [-min(pa, pb), min(la - pa, lb - pb))
 *     o = 1:  A[pa + t] with 3 - B[pb + K - 1 - t];    valid t in [max(-pa, pb + K - lb), min(la - pa, pb + K))
 * [t_lo, t_hi) is the valid range, span = t_hi - t_lo.  A column matches iff the two codes are equal.  Columns 0 .. K - 1 must be valid and
 * must all match; else the row is no seed of these reads and the call refuses.
 *
 * Extension.  match in 1 .. 2^15, mismatch (a penalty) in 0 .. 2^15, xdrop in 0 .. 2^31 - 1.  Right side, for t = K, K + 1, ... < t_hi,
 * from s = best = 0, end = K:  (1) s += match or s -= mismatch;  (2) if s > best: best = s, end = t + 1;  (3) if best - s > xdrop: stop.
 * The left side is the same over t = -1, -2, ... >= t_lo and gives `begin`.  score = K * match + best_right + best_left (64 bits); the
 * overlap is the columns [begin, end); mismatches counts the mismatching columns inside it.
 *
 * Row.  Six uint64 words (48 bytes; the lists are 16-byte aligned):
 *     { key, score, a_lo << 32 | a_hi, b_lo << 32 | b_hi, mismatches << 32 | ends, support }
 * in forward read coordinates, half-open: a_lo = pa + begin, a_hi = pa + end; o = 0: b_lo = pb + begin, b_hi = pb + end; o = 1:
 * b_lo = pb + K - end, b_hi = pb + K - begin.  ends: bit 0 a_lo == 0, bit 1 a_hi == la, bit 2 b_lo == 0, bit 3 b_hi == lb.  support is
 * word 3 of the input row.
 *
 * Filter.  Rows with score < min_score or a_hi - a_lo < min_length are dropped after the extension; the survivors keep the input's order.
 * With both 0 the output has the input's n rows, one to one.
 *
 *   opts       match, mismatch, xdrop, min_score, min_length; wave_span: a row whose span is at least wave_span is extended by a whole
 *              wavefront (64 windows of 32 columns per step), any other row by one lane.  0 = the library's default, 1 = every row by
 *              a wavefront, UINT32_MAX = none.  Both give the same rows.
 *   out        n, rows (host, pinned) or rows_dev (on_device); input_rows; dropped (by the filter); columns = the sum of a_hi - a_lo over
 *              all rows before the filter; wave_rows = rows a wavefront took; ms_* HIP events.  hsk_overlaps_free before hsk_destroy.
 * Memory: 48 + 8 bytes per input row, 1 + 48 per row more with a filter, and the uploaded rows and reads.
 * HSK_ERR_INVALID_ARG, with a hsk_last_error text that names the case and how many rows, the context usable afterwards, no partial result:
 * a NULL pointer; n > 0 without rows; a rows_dev that is not 16-byte aligned; match, mismatch or xdrop outside their ranges;
 * rid_base + nreads > 2^31; a row whose rid_a or rid_b lies outside [rid_base, rid_base + nreads); a read of a row that does not lie
 * inside packed_bytes; a seed that does not fit its reads (pa + K > la or pb + K > lb); a seed whose K columns do not all match ("these
 * are not the reads the rows were computed from").  No byte at or beyond packed_bytes is read.  n == 0 is an empty list, no error.
 */
typedef struct {
    int32_t  match, mismatch;
    uint32_t xdrop;
    uint64_t min_score;
    uint32_t min_length;
    uint32_t wave_span;
    int64_t  reserved[4];
} hsk_extend_opts;

typedef struct {
    uint64_t n;             /* rows */
    uint64_t *rows;         /* host (pinned), n * 6 words; NULL when left on the device */
    void     *rows_dev;     /* device copy when asked for */
    uint64_t input_rows, dropped, columns, wave_rows;
    double   ms_extend, ms_d2h, ms_total;   /* HIP events */
    uint64_t cells;         /* hsk_pair_diags_extend_gapped: live cells (below); 0 from the ungapped call.  The first word of what was reserved[4] */
    int64_t  reserved[3];
    void    *priv;
} hsk_overlaps;

int  hsk_pair_diags_extend(hsk_ctx *ctx, const hsk_pair_diags *in,
                           const void *packed, uint64_t packed_bytes, const void *read_byte_off, const void *read_len,
                           uint64_t nreads, int64_t rid_base, int32_t reads_on_device,
                           const hsk_extend_opts *opts, int32_t on_device, hsk_overlaps *out);
void hsk_overlaps_free(hsk_ctx *ctx, hsk_overlaps *o);
/*
 * Gapped x-drop overlaps: the seed of every diagonal row, extended in both directions inside a band of diagonals, so that the overlap
 * follows the reads across insertions and deletions.  One overlap row per input row; exact integer work, held to this definition word
 * for word (csrc/hsk_gapped.h is the one implementation the kernel and the CPU tests share; tests/gapped_ref.py spells it base by base).
 *
 * Input.  Input, seed checks and refusals are exactly those of hsk_pair_diags_extend: the rows come from host memory or from HBM; the
 * reads are given as hsk_result_strands takes them; K is the context's; the seed's K columns must fit their reads and all match.
 *
 * Sides.  For a row with seed (pa, pb), orientation o and reads A, B of lengths la, lb, each side walks two base sequences x (from A) and
 * y (from B) away from the seed.  Indices start at 1.
 *     side   x_i                 na            o   y_j                      nb
 *     right  A[pa + K - 1 + i]   la - pa - K   0   B[pb + K - 1 + j]        lb - pb - K
 *     right  A[pa + K - 1 + i]   la - pa - K   1   3 - B[pb - j]            pb
 *     left   A[pa - i]           pa            0   B[pb - j]                pb
 *     left   A[pa - i]           pa            1   3 - B[pb + K - 1 + j]    lb - pb - K
 *
 * Cells.  Cell (i, j) exists for 0 <= i <= na, 0 <= j <= nb and |i - j| <= band.  It lies on antidiagonal d = i + j.  A live cell holds a
 * pair (s, e): score and edits.  Pairs compare by larger s first, then smaller e.  Cell (0, 0) is live with (0, 0).  For d = 1, 2, ...,
 * the candidates of a cell come from its live predecessors:
 *     from (i-1, j-1): (s + match, e) if x_i == y_j, else (s - mismatch, e + 1);
 *     from (i-1, j) and from (i, j-1): (s - gap, e + 1).
 * The cell takes the best candidate.  A cell with no candidate is dead.  It is also dead if best - s > xdrop.  Here `best` is the side's
 * best score over antidiagonals 0 .. d - 1.
 * After antidiagonal d: if its best live cell has s > best (strictly), then best, (i*, j*) and e* become that cell's.  The best live cell is
 * the one with the largest (s, e) pair, and the smallest i on a tie.
 * The side ends after two consecutive antidiagonals without a live cell, or after d = na + nb.  Nothing beyond that can be live, so the
 * stop is exact.
 *
 * Row.  { key, score, a_lo << 32 | a_hi, b_lo << 32 | b_hi, edits << 32 | ends, support }
 *     score = K * match + best_right + best_left.      edits = e*_right + e*_left.
 *     a_lo = pa - i*_left, a_hi = pa + K + i*_right.
 *     o = 0: b_lo = pb - j*_left, b_hi = pb + K + j*_right.      o = 1: b_lo = pb - j*_right, b_hi = pb + K + j*_left.
 * `ends`, `support` and the order-keeping min_score / min_length filter are as in the ungapped call.
 *
 * Consequence.  With band = 0 the row equals hsk_pair_diags_extend's row word for word, for every match, mismatch and xdrop.
 *
 * Ranges.  match 1 .. 255; mismatch and gap 0 .. 255; xdrop 0 .. 2^31 - 1; band 0 .. 63.  A row with la + lb >= 2^22 is refused.  A 32-bit
 * score is then exact.
 *
 *   opts       match, mismatch, gap, xdrop, band, min_score, min_length; group: the lanes that take one row.  0 = the smallest group that
 *              holds the band; 8, 16, 32 or 64 force a width; a width with band > group - 1, or any other value, is
 *              HSK_ERR_INVALID_ARG.  All legal widths give the same rows.
 *   out        an hsk_overlaps as the ungapped call fills it; cells = the number of live cells on antidiagonals d >= 1 of both sides,
 *              summed over all rows before the filter; columns as before; wave_rows = 0.
 * Memory: 48 bytes per input row, 1 + 48 per row more with a filter, and the uploaded rows and reads.
 * HSK_ERR_INVALID_ARG: every case of hsk_pair_diags_extend, with the same texts; match, mismatch, gap, xdrop, band or group outside
 * their ranges; a row with la + lb >= 2^22 (no row is written).  The texts name the case and the number of rows.
 */
typedef struct {
    int32_t  match, mismatch, gap;
    uint32_t xdrop, band;
    uint64_t min_score;
    uint32_t min_length;
    uint32_t group;
    int64_t  reserved[4];
} hsk_gapped_opts;

int  hsk_pair_diags_extend_gapped(hsk_ctx *ctx, const hsk_pair_diags *in,
                                  const void *packed, uint64_t packed_bytes, const void *read_byte_off, const void *read_len,
                                  uint64_t nreads, int64_t rid_base, int32_t reads_on_device,
                                  const hsk_gapped_opts *opts, int32_t on_device, hsk_overlaps *out);
/*
 * String graph: the reads that lie inside another read go out, the dovetails become arcs between read ends, and every arc that two
 * shorter arcs explain is marked.  What is left are the edges of the string graph.  Integer work on the whole list at once, held to this
 * definition word for word (csrc/hsk_strgraph.h is the one implementation the kernels and the CPU tests share; tests/strgraph_ref.py
 * spells it with dictionaries).
 *
 * Input.  A list of hsk_overlaps rows: of `in` the call reads n, rows_dev if set, else rows (host memory, uploaded as the extend calls
 * upload theirs); its priv may be NULL.  The reads' lengths read_len[nreads] (uint32; on the device with lens_on_device) and rid_base.
 * No bases are read.  For a row: o = key >> 63; a, b are the reads rid_a - rid_base, rid_b - rid_base with lengths la, lb;
 * e = word4 & 15 (the ends bits).
 *
 * Vertices.  Two per read: v = 2 r + s; s = 0 is the read as stored, s = 1 its reverse complement; the complement of v is v ^ 1.  An arc
 * v -> w says that a suffix of oriented read v overlaps a prefix of oriented read w; len(v -> w) is the number of bases of v, in v's
 * orientation, in front of the overlap.
 *
 * Row class (one byte per input row; the first rule that applies wins):
 *     7 SELF          rid_a == rid_b
 *     3 A_CONTAINED   e & 3 == 3: marks read a contained (also e == 15: of two reads that cover each other, a goes)
 *     4 B_CONTAINED   e & 12 == 12: marks read b contained
 *     2 INTERNAL      not a dovetail: o = 0 and e not in {6, 9}, or o = 1 and e not in {10, 5}
 *     5 DROPPED_READ  a dovetail with a or b marked contained by ANY row of the list
 *     6 DUPLICATE     among dovetails with equal (key, e) all but the one with the largest score; on a tie the smallest row index stays
 *     1 REDUCED       a surviving dovetail with at least one transitive arc
 *     0 KEPT          an edge of the string graph
 *
 * Arcs of a surviving dovetail: two, complements of each other.
 *     o, e                              arc 1 (len)                  arc 2 (len)
 *     0, 6   a_hi == la, b_lo == 0      2a   -> 2b   (a_lo)          2b+1 -> 2a+1 (lb - b_hi)
 *     0, 9   a_lo == 0,  b_hi == lb     2b   -> 2a   (b_lo)          2a+1 -> 2b+1 (la - a_hi)
 *     1, 10  a_hi == la, b_hi == lb     2a   -> 2b+1 (a_lo)          2b   -> 2a+1 (b_lo)
 *     1, 5   a_lo == 0,  b_lo == 0      2b+1 -> 2a   (lb - b_hi)     2a+1 -> 2b   (la - a_hi)
 *
 * Transitive.  G is all arcs of surviving dovetails, duplicates out; arcs that are themselves transitive stay in G.  An arc v -> x of
 * length L is transitive iff G has arcs v -> w and w -> x with w's read different from both v's read and x's read and
 * len(v -> w) + len(w -> x) <= L + fuzz (64-bit sums).  One round on the unreduced graph: the result does not depend on the order of
 * evaluation, and a second round would find nothing new.  A row is REDUCED iff either of its two arcs is transitive.  (Two rows with a
 * and b exchanged can give the same arc twice; they are no duplicates, both arcs are in G.)
 *
 *   opts       fuzz; wave_degree: a vertex with at least this many out-arcs (arc records, duplicates included) is reduced by a whole
 *              workgroup, any other arc by one lane.  0 = the library's default, 1 = every vertex by a workgroup, UINT32_MAX = none.
 *              The result is the same for every value.
 *   out        n, rows / rows_dev: the KEPT rows, six words unchanged, in the input's order -- again a valid hsk_overlaps list;
 *              row_class / row_class_dev: input_rows bytes; contained / contained_dev: (nreads + 31) / 32 uint32 words, read r is
 *              bit r % 32 of word r / 32.  With on_device all three stay in HBM, else all three are pinned host memory.
 *              class_rows[c] = rows of class c; contained_reads; arcs = arcs of G; wave_vertices = vertices a workgroup took;
 *              max_degree = the most arc records of one vertex; wave_degree = the threshold that was used; ms_classify (classes,
 *              contained bits, arc records), ms_sort, ms_reduce (duplicates, offsets, the reduction, the kept rows), ms_d2h, ms_total
 *              (HIP events).  hsk_reduced_free before hsk_destroy.
 * Memory: the uploaded rows and lengths; 1 byte per row; 64 bytes per dovetail row between live reads (two arc records, sorted in two
 * buffers) and the sort's tables; 8 bytes x (2 nreads + 1); 48 bytes per kept row.  HSK_ERR_OOM names the bytes that were asked for.
 * HSK_ERR_INVALID_ARG, with a hsk_last_error text that names the case and how many rows, the context usable afterwards, no partial result:
 * a NULL pointer; n > 0 without rows; a rows_dev that is not 16-byte aligned; rid_base + nreads > 2^31; n >= 2^32 (the row index travels
 * in 32 bits); a row that names a read outside [rid_base, rid_base + nreads); a row whose coordinates and ends bits do not agree with the
 * lengths ("these are not the lengths of the reads the rows were computed from"): a_lo < a_hi <= la and b_lo < b_hi <= lb must hold, and
 * bit 0 <=> a_lo == 0, bit 1 <=> a_hi == la, bit 2 <=> b_lo == 0, bit 3 <=> b_hi == lb.  n == 0 is an empty graph, no error.
 */
typedef struct {
    uint32_t fuzz;
    uint32_t wave_degree;
    int64_t  reserved[4];
} hsk_reduce_opts;

typedef struct {
    uint64_t n;             /* kept rows */
    uint64_t *rows;         /* host (pinned), n * 6 words; NULL when left on the device */
    void     *rows_dev;
    uint8_t  *row_class;    /* host (pinned), input_rows bytes */
    void     *row_class_dev;
    uint32_t *contained;    /* host (pinned), (nreads + 31) / 32 words */
    void     *contained_dev;
    uint64_t input_rows, nreads;
    uint64_t class_rows[8];
    uint64_t contained_reads, arcs, wave_vertices, max_degree;
    uint32_t wave_degree, pad_;
    double   ms_classify, ms_sort, ms_reduce, ms_d2h, ms_total;   /* HIP events */
    int64_t  reserved[4];
    void    *priv;
} hsk_reduced;

int  hsk_overlaps_reduce(hsk_ctx *ctx, const hsk_overlaps *in, const void *read_len, uint64_t nreads, int64_t rid_base,
                         int32_t lens_on_device, const hsk_reduce_opts *opts, int32_t on_device, hsk_reduced *out);
void hsk_reduced_free(hsk_ctx *ctx, hsk_reduced *r);
/*
 * Unitigs: the maximal non-branching paths of a list of string graph edges, one of each complement pair, with every member read's
 * orientation and position in the unitig.  Integer work in HBM, held to this definition word for word (csrc/hsk_unitig.h is the one
 * implementation the kernels and the CPU tests share; tests/unitig_ref.py spells it with dictionaries and a sequential walk).
 *
 * Input.  A list of hsk_overlaps rows: of `edges` the call reads n, rows_dev if set, else rows (host memory, uploaded as
 * hsk_overlaps_reduce uploads its own); its priv may be NULL.  The contained bits: (nreads + 31) / 32 uint32 words laid out as
 * hsk_reduced.contained, on the host or (contained_on_device) on the device; NULL: no read is contained.  The reads' lengths
 * read_len[nreads] (uint32; on the device with lens_on_device) and rid_base.  No bases are read.  The vertices, the two arcs of a row and
 * their len are those of hsk_overlaps_reduce.
 *
 * Out-arcs.  out(v) is the set of distinct w with an arc v -> w.  Two rows with a and b exchanged can give the same arc twice: the arc
 * is then represented by the record with the smallest len, then the smallest row index.  deg(v) = |out(v)|.  Every row gives an arc and
 * its complement, so the in-arcs of v are the complements of out(v ^ 1).
 *
 * Links.  An arc v -> w is a link iff deg(v) == 1 and deg(w ^ 1) == 1; then succ(v) = w and pred(w) = v.  Links form vertex-disjoint
 * paths and cycles over the live vertices -- the two vertices of every read that is not contained; a live vertex without a link is a
 * path of one.  No chain holds both v and v ^ 1 (its middle would be an arc between the two vertices of one read, and SELF rows are
 * refused), so chains come in disjoint complement pairs over the same reads.
 *
 * Unitigs.  Of each complement pair, the unitig is the chain in which the smallest read id is forward: whose smallest vertex is even.
 * A path starts at its head; a cycle starts at its smallest vertex and is marked circular.  Unitigs are numbered in increasing order of
 * their first vertex.  Every live read is therefore a member of exactly one unitig, exactly once.
 *
 * Layout rows: one row of four words per (unitig, member), ordered by (unitig, rank):
 *     { unitig << 32 | rank, rid << 1 | s, offset, link }
 * rid is the absolute read id, s = 1 the reverse complement; offset is the sum of the len of the links in front of the member, in 64
 * bits: the unitig coordinate of the oriented read's first base; link = len << 32 | row of the link to the next member (row: the index
 * of the representative's row in `edges`); ~0 for the last member of a path; for the last member of a cycle the link back to rank 0.
 * Unitig rows: one row of four words per unitig:
 *     { first layout row, reads, bases, circular }
 * bases of a path = offset(last) + len(last read); of a cycle = the sum of all its links' len.
 *
 *   opts       nothing yet: a reserved block, zero.
 *   out        members, rows / rows_dev: the layout rows; unitigs, table / table_dev: the unitig rows.  With on_device both stay in HBM,
 *              else both are pinned host memory.  singletons = unitigs of one read; circular; longest = the most reads in one unitig;
 *              links (both orientations are counted); branch_vertices = live v with deg(v) > 1; live_reads; input_rows; arcs = the sum
 *              of deg(v) (distinct arcs, both orientations); rounds = the ranking launches: the ranking is pointer doubling, and the
 *              number of its rounds is fixed before the first launch, 2 ceil(log2(min(nreads, n + 1))) -- one phase brings every
 *              path's prefix sums to its head and every cycle's smallest vertex around it, the second ranks the cycles cut there;
 *              ms_arcs (checks, arc records), ms_sort, ms_rank (degrees, links, rounds), ms_emit (unitig ids, the two row lists, the
 *              counts), ms_d2h, ms_total (HIP events).  hsk_unitigs_free before hsk_destroy.
 * Memory: the uploaded rows, bits and lengths; 1 byte per row; 64 bytes per row (two arc records, sorted in two buffers) and the sort's
 * tables; 104 bytes per vertex, two vertices per read; 32 bytes per unitig and per member.  HSK_ERR_OOM names the bytes asked for.
 * HSK_ERR_INVALID_ARG, with a hsk_last_error text that names the call, the case and how many rows, the context usable afterwards, no
 * partial result: every pointer, alignment, 2^31, 2^32, read-range and lengths-disagree case of hsk_overlaps_reduce, with the same
 * texts; a row that is not a dovetail between two different reads -- its own class is SELF, A_CONTAINED, B_CONTAINED or INTERNAL -- ("k of
 * n rows are no dovetails: this is not a list of string graph edges"); a row that names a read whose contained bit is set.  Of a row
 * with several faults the first of this order counts.  n == 0 is no error: every live read is then a unitig of its own.
 */
typedef struct {
    int64_t  reserved[4];
} hsk_unitig_opts;

typedef struct {
    uint64_t members;       /* layout rows */
    uint64_t *rows;         /* host (pinned), members * 4 words; NULL when left on the device */
    void     *rows_dev;
    uint64_t unitigs;       /* unitig rows */
    uint64_t *table;        /* host (pinned), unitigs * 4 words */
    void     *table_dev;
    uint64_t input_rows, nreads;
    uint64_t singletons, circular, longest, links, branch_vertices, live_reads, arcs, rounds;
    double   ms_arcs, ms_sort, ms_rank, ms_emit, ms_d2h, ms_total;   /* HIP events */
    int64_t  reserved[4];
    void    *priv;
} hsk_unitigs;

int  hsk_overlaps_unitigs(hsk_ctx *ctx, const hsk_overlaps *edges, const void *contained, int32_t contained_on_device,
                          const void *read_len, uint64_t nreads, int64_t rid_base, int32_t lens_on_device,
                          const hsk_unitig_opts *opts, int32_t on_device, hsk_unitigs *out);
void hsk_unitigs_free(hsk_ctx *ctx, hsk_unitigs *u);
/* Result egress (write_output_file, reference src/hysortk.cpp:138-164): the lines "KMERSTRING\tcount\n" of `n` entries
 * ((nw + 1)-word records: host memory, or device memory when `on_device`), formatted on the GPU into `text` (host, capacity
 * bytes); *nbytes = bytes needed (call with capacity 0 to size the buffer: K + 2 + up to 20 digits per entry). */
int hsk_format_entries(hsk_ctx *ctx, const void *entries, uint64_t n, int32_t nw, int32_t on_device,
                       char *text, uint64_t capacity, uint64_t *nbytes);
int  hsk_get_stats(hsk_ctx *ctx, hsk_stats *out, int reset);

/* ---- stage entry points (each one is a reference function of SURVEY 8a; used by the parity
 *      tests and by callers that want one stage only) ---------------------------------------- */
/* a4: FindKmerDestinationsParallel (kmerops.cpp:1010): dest[j] for every k-mer of every read,
 * concatenated in read order; dest_off[r] .. dest_off[r+1] is read r.  Host in / host out. */
int hsk_stage_destinations(hsk_ctx *ctx, const uint8_t *packed, uint64_t packed_bytes,
                           const uint64_t *read_byte_off, const uint32_t *read_len, uint64_t nreads,
                           int32_t *dest, uint64_t dest_capacity, uint64_t *dest_off);
/* a5+a11: supermer split followed by GetRepKmers: the canonical k-mers (nw words each, plus
 * pos,rid when EXTENSION) of task `task`, in unspecified order.  Returns count in *n. */
int hsk_stage_task_kmers(hsk_ctx *ctx, const uint8_t *packed, uint64_t packed_bytes,
                         const uint64_t *read_byte_off, const uint32_t *read_len, uint64_t nreads,
                         int64_t rid_base, int32_t task, uint64_t *keys, uint32_t *pos, int32_t *rid,
                         uint64_t capacity, uint64_t *n);
/* a12: sort_task (kmerops.cpp:1382): in-place LSD radix sort of n records of nw words by their
 * first key_bytes bytes read as a little-endian integer; optional 8-byte payload per record. */
int hsk_stage_sort(hsk_ctx *ctx, uint64_t *keys, uint64_t *vals, uint64_t n, int32_t nw);
/* a13: count_sorted_kmers (kmerops.cpp:1410) on a sorted host array; writes entries
 * {key words, cnt} to out_entries (capacity in entries), *n_out = number kept. */
int hsk_stage_count_sorted(hsk_ctx *ctx, const uint64_t *sorted_keys, uint64_t n, int32_t nw,
                           uint64_t *out_entries, uint64_t capacity, uint64_t *n_out);

/* ---- host-side planning (pure CPU; usable without a GPU) ---------------------------------- */
/* tot_tasks rule of prepare_supermer (kmerops.cpp:40-43,76). */
int hsk_plan_tot_tasks(int omp_max_threads, int thread_per_worker, int avg_task_per_worker, int nprocs);
/* HeavyHitterClassifier (kmerops.cpp:1157-1199). */
int hsk_plan_classify(const uint64_t *task_kmers, int ntasks, double unbalanced_ratio, int32_t *types);
/* BalancedDispatcher / RoundRobinDispatcher (kmerops.cpp:1201-1327): task -> owner rank. */
int hsk_plan_dispatch(const uint64_t *task_bytes, int ntasks, int nprocs, int plain,
                      double upper_coe, double step, int32_t *owner);
/* FastaIndex::getpartition (fastaindex.cpp:52-100): contiguous split of reads by bases. */
int hsk_plan_partition_reads(const uint64_t *read_len, uint64_t nreads, int nprocs, uint64_t *counts);

/* The all-to-all-v plan of the supermer exchange (csrc/hsk_comm.h), as pure arithmetic: given the
 * owner table and the full size matrix M[src][task] = {supermers, bytes, kmers}, what `rank` sends
 * to / receives from each peer (counts and offsets in supermers and bytes; a rank's tasks are stored
 * grouped by owner, ascending task id) and where every (task, src) segment lands in the receive
 * arrays.  send_recv: [nranks][8] = send_sup, send_bytes, send_sup_off, send_byte_off, recv_sup,
 * recv_bytes, recv_sup_off, recv_byte_off.  segs: [ntasks][nranks][4] = sup_off, n_sup, byte_off,
 * kmer_off (zero rows for tasks `rank` does not own). */
int hsk_plan_exchange(int nranks, int rank, int ntasks, const int32_t *owner, const uint64_t *size_matrix,
                      uint64_t *send_recv, uint64_t *segs);

/* ---- multi-GPU (one process per GPU; RCCL over xGMI) -------------------------------------- */
#define HSK_UNIQUE_ID_BYTES 128
int hsk_comm_get_unique_id(void *id128);                       /* rank 0, then broadcast by the caller */
int hsk_comm_init(hsk_ctx *ctx, int nranks, int rank, const void *id128);
int hsk_comm_destroy(hsk_ctx *ctx);
/* One-rank communicator on this GPU: all-reduce and grouped send/recv to self with checked results (exercises the
 * RCCL binding on a single-GPU box). */
int hsk_comm_selftest(hsk_ctx *ctx);

/* ---- synthetic reads, generated in HBM (bench / tests) ------------------------------------ */
/* S-reads(G, c) of BASELINE.md: random genome of genome_len bases, error-free reads of read_len
 * bases sampled uniformly, strand 50/50.  Outputs device pointers owned by the ctx (freed by
 * hsk_synth_free or hsk_destroy).  The same generator exists in numpy (hysortk_amd/synth.py). */
int hsk_synth_reads(hsk_ctx *ctx, uint64_t genome_len, uint32_t read_len, uint64_t nreads, uint64_t seed,
                    uint64_t first_read, /* index of read 0 in the global read stream (rank * nreads for weak scaling) */
                    void **d_packed, uint64_t *packed_bytes, void **d_read_byte_off, void **d_read_len);
/* Same with substitution errors: every base is replaced by one of the other three with probability error_rate (0 .. 0.75; at 0.75 every base is uniform over ACGT).
 * Error-free reads are the best case of the LDS hash aggregation (distinct keys per prefix bin = records / coverage); with
 * ~1 % errors most bins hold several times more distinct keys. */
int hsk_synth_reads_err(hsk_ctx *ctx, uint64_t genome_len, uint32_t read_len, uint64_t nreads, uint64_t seed, uint64_t first_read,
                        double error_rate, void **d_packed, uint64_t *packed_bytes, void **d_read_byte_off, void **d_read_len);
int hsk_synth_free(hsk_ctx *ctx, void *d_packed, void *d_read_byte_off, void *d_read_len);

/* ---- FASTA ingest on the device (what read_dna_buffer + DnaSeq::compress do on the host, reference src/hysortk.cpp:18-33,
 *      src/dnaseq.cpp:9-31) -------------------------------------------------------------------------------------------- */
/* `text` = the FASTA file's bytes (host memory, e.g. an mmap); record r has rec_len[r] bases, the first at text[rec_pos[r]],
 * with line_bases[r] bases per line and line_width[r] bytes per line including the line break (the .fai columns 2-5;
 * line_bases 0 = no line breaks).  Builds the 2-bit packed DnaBuffer of these records in HBM (every record byte-aligned,
 * same bytes as the reference's packer incl. its code-4 spill for non-ACGTN characters) and returns device arrays that
 * hsk_count_device takes (free them with hsk_synth_free). */
int hsk_pack_fasta(hsk_ctx *ctx, const char *text, uint64_t text_bytes, const uint64_t *rec_pos, const uint32_t *rec_len,
                   const uint32_t *line_bases, const uint32_t *line_width, uint64_t nrec,
                   void **d_packed, uint64_t *packed_bytes, void **d_read_byte_off, void **d_read_len);
int hsk_memcpy_d2h(hsk_ctx *ctx, void *dst, const void *d_src, uint64_t bytes);
/* Measurement aid (ABI 3): what a plain HBM copy reaches on this GPU -- a hand-written kernel, 16 bytes per lane, `bytes` read and
 * `bytes` written per launch, best of `iters` launches over four grid sizes; *gbs = 2 * bytes / time.  bench.py quotes the
 * kernels' achieved GB/s against the 8 TB/s spec AND against this figure. */
int hsk_copy_peak(hsk_ctx *ctx, uint64_t bytes, int iters, double *gbs);

#ifdef __cplusplus
}
#endif
#endif /* HSK_H_ */
