// hsk_host_ctx.h -- host side: device memory pool, context, error plumbing, event pool, phase timer.
// Part of the single translation unit hsk_api.hip (included in this order; everything here is file-local).
#pragma once

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
// (the device memory pool: hsk_pool.h -- segments of the regions hipMalloc returned, best fit with split and coalesce)
static int pool_hip_malloc(void **p, size_t n) { if (hipMalloc(p, n) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return 1; } return 0; }
static int pool_hip_free(void *p) { return hipFree(p) == hipSuccess ? 0 : 1; }

// pinned host memory for results (hipHostMalloc of gigabytes takes longer than counting them: freed result blocks are kept)
struct HostPool {
    std::multimap<size_t, void *> free_blocks;
    std::map<void *, size_t> live;
    void *alloc(size_t bytes)
    {
        if (bytes == 0) bytes = 64;
        // sizes are rounded up to 1/8 of their power of two: the result of the next call (a few per cent larger or
        // smaller) lands in the same size class and takes this call's block instead of pinning gigabytes again (~0.2 s per GB)
        { size_t g = 4096; while (g * 16 <= bytes) g <<= 1; bytes = (bytes + g - 1) & ~(g - 1); }
        auto it = free_blocks.lower_bound(bytes);
        if (it != free_blocks.end() && it->first <= bytes + bytes / 2 + (1u << 20)) {
            void *p = it->second; live[p] = it->first; bytes_cached -= it->first; free_blocks.erase(it); return p;
        }
        void *p = nullptr;
        if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            trim();
            if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        }
        live[p] = bytes;
        return p;
    }
    // cached (free) pinned blocks are capped: a 10 Gbp call leaves ~8 GB of result and staging blocks behind, which the next call of
    // the same size takes again; beyond the cap the largest cached blocks go back to the system
    static constexpr size_t CACHE_CAP = (size_t)24 << 30;
    size_t bytes_cached = 0;
    void release(void *p)
    {
        auto it = live.find(p);
        if (it == live.end()) return;
        free_blocks.insert({it->second, p}); bytes_cached += it->second; live.erase(it);
        while (bytes_cached > CACHE_CAP && !free_blocks.empty()) { auto big = std::prev(free_blocks.end()); (void)hipHostFree(big->second); bytes_cached -= big->first; free_blocks.erase(big); }
    }
    void trim() { for (auto &kv : free_blocks) (void)hipHostFree(kv.second); free_blocks.clear(); bytes_cached = 0; }
    // hsk_destroy: the cache goes; blocks of results the caller still holds are NOT freed here (they belong to the results:
    // hsk_result_free(NULL, &res) releases them after the context is gone, include/hsk.h)
    void destroy() { trim(); live.clear(); }
};

struct EvPair { hipEvent_t a, b; int kind; u64 keys; u64 bytes; };

// What a call learns about its input BEFORE it commits to a plan (estimate_plan, hsk_api.hip): the k-mer spectrum of a small prefix of
// the reads, counted by the instance path, extrapolated to the whole input -- distinct k-mers per k-mer instance is what the combining
// extraction (pairs per k-mer), the first table of the LDS aggregation (distinct keys per prefix bin) and the decision to aggregate at
// all depend on.  Valid for the call that made it; the adaptive fields of the context are only the fallback where no estimate is made.
struct PlanEstimate {
    bool valid = false;
    double distinct_per_kmer = 0;      // estimated (distinct canonical k-mers) / (k-mer instances) of the WHOLE input
    double lambda_sample = 0;          // mean copies per genomic k-mer inside the sample
    double fraction = 0;               // sample bytes / input bytes
    u64 sample_kmers = 0, n1 = 0, n2 = 0, n3 = 0, distinct_sample = 0;
    u64 homo_at = 0, homo_cg = 0;      // exact copies of the all-A / all-C k-mer inside the sample (valid even where `valid` is not: payloads, wide keys)
    double ms = 0;                     // host wall clock of the estimate
};

// What describes only the call that is running: reset by value when an entry point opens its scope and when it closes it (ApiCall,
// hsk_api.hip), so that nothing of one call reaches the next.  What a call learns for the calls after it stays in hsk_ctx.
struct CallState {
    // the plan
    PlanEstimate est;                  // this call's estimate (estimate_plan); est.valid decides instead of combine_off / agg_off / agg_first_cap
    int plan_attempt = 0;              // dispatch_pipeline: how often this call has been started again (HSK_RETRY_PLAN); bounded there
    // combining extraction (hsk_combine.h): combine_now = this call lays the store out for it (one GPU, one-word keys, no payload)
    bool combine_now = false;
    bool item_mode_now = false;        // ... on ONE GPU: the store holds items (several ranks: byte runs + minimizer bits, items built by the owners)
    u32 vt_shift = 0;                  // this call's parse splits every task into 1 << vt_shift virtual tasks (combining extraction)
    bool combine_left_now = false;     // this call has left the combining extraction (binding for the attempts that follow, whatever the estimate said)
    bool combine_veto = false;         // this attempt's store turned out to be no use to the combining extraction (too few tasks for a batch ...): the next attempt goes without it
    bool pair_cap_full = false;        // this call's pair buffers ran over once: full size for the attempts that follow
    u32 drop_mask_now = 0;             // bit 0 / 1 = the all-A / all-C k-mer has more than U copies inside the sample alone, the scan leaves its instances out
    u64 dropped_now = 0;               // ... and how many it left out (they count as k-mers of the input: hsk_result::total_kmers)
    // the input
    const u8 *zc_src = nullptr;        // hsk_count() with pinned input: device view of the caller's packed reads (scan_kernel reads them in place)
    const u8 *h2d_src = nullptr;       // hsk_count() with pinned input, slab ingest: the caller's packed reads (host pointer); enqueue_slab_copies sends them slab by
    int h2d_slabs = 0;                 // slab (DMA, d2h_stream) and the driver (parse_ingest_pipelined, parse_count) hashes slab s while slab s + 2 is on the link
    // hsk_count() with derived read offsets: host threads compare the caller's offsets with the back-to-back layout while the GPU
    // scans (result collected with the task totals); roff_host / roff_given: the caller's array and a device buffer for it, used
    // only when the comparison fails (a buffer with gaps)
    std::future<bool> roff_check;
    bool roff_bad = false;             // ... its verdict, when somebody other than count_verdict collected it (parse_ingest_pipelined)
    const uint32_t *rlen_host = nullptr;   // the read lengths were generated on the device from a sample (all reads equally long): the caller's array,
                                           // copied after all if the host threads find a read of another length (same fallback as a buffer with gaps)
    const uint64_t *roff_host = nullptr;
    u64 *roff_given = nullptr;
    bool index_unchecked = false;      // hsk_count(): the read index is validated on the device (index_check_kernel), the verdict is read with the task totals
    u32 scan_blocks = 0;               // experiments (hsk_debug_parse_overlap): workgroups of the parse kernels instead of PARSE_MAX_BLOCKS (never more: parse_tiling)
};

struct hsk_ctx {
    hsk_config cfg;
    Tuning tune;                       // hsk_config::tuning, then HSK_TUNING (hsk_tuning.h); not written after hsk_init
    int nw = 1;
    hipStream_t stream = nullptr;
    hipStream_t comm_stream = nullptr;
    hipStream_t d2h_stream = nullptr;  // result copies, overlapped with the kernels of the following batches
    DevPool pool;
    HostPool hpool;
    double entries_per_kmer = 0;       // kept entries per input k-mer of the last hsk_count (sizes the pinned result block of the next one)
    char err[512] = {0};
    hsk_stats stats;
    std::vector<hipEvent_t> ev_free;
    std::vector<EvPair> ev_pending;
    void *pinned = nullptr; size_t pinned_bytes = 0;     // small staging area (histograms, totals)
    u32 *d_err = nullptr;
    Comm comm;
    CallState call;                    // the running call's
    int agg_first_cap = 10;            // log2 of the hash table the next aggregation starts with (AG_LOG2CAP_*): follows the fullest bin of the
                                       // previous batch, so that reads with errors / low coverage do not pay for a table they overflow anyway
    bool xcd_batch_ok = true;          // hsk_init's census saw workgroups on all eight XCC ids (see xcc_census_kernel)
    int agg_clean_batches = 0;         // EXTENSION: batches in a row whose first table held every bin (four of them: one table size down again)
    int agg_off_calls = 0;             // calls since agg_off / agg_off_wide was set
    bool agg_off_wide = false;         // the same for multi-word keys and EXTENSION: no prefix passes + tables, the full-width passes and the two-pass counter
    bool agg_off = false;              // one-word keys without payload: the input has too few copies per k-mer for the LDS aggregation (most bins of a
                                       // batch overflowed the 2048-slot table): batches take four prefix passes + the tile finish from here on
    // combine_off = the input kept too many pairs per k-mer (or a bin beat the weighted finish): the instance path until another look
    bool combine_off = false; int combine_off_calls = 0;
    // ... another look after combine_off_period calls: 8, and twice as many every time the look finds the same kind of input again (up
    // to 64: a look costs the call ~2 x, reads with errors should not pay that every eighth call); back to 8 once a call has gone through
    int combine_off_period = 8, combine_good_calls = 0;
    void leave_combine() { call.combine_left_now = true; combine_off_period = combine_good_calls ? 8 : std::min(combine_off_period * 2, 64); combine_good_calls = 0; combine_off = true; combine_off_calls = 0; }
    int combine_prefix_floor = 0;      // ... never below this again (set when a bin beat the last table with fewer bits)
    int combine_prefix = 0;            // key bits of the weighted finish's bins the next batch is planned with (0: the default; follows the pairs per task)
    double est_bias = 1.0;             // pairs per k-mer the combining extraction really produced / what the estimate promised, when a call had to leave the plan after all
    // a call that followed its estimate into the combining extraction and had to start again: estimates like this one are not believed again on this context
    void distrust_estimate(double ratio) { const PlanEstimate &est = call.est; if (est.valid && est.distinct_per_kmer > 0) est_bias = std::max(est_bias, 1.05 / (est.distinct_per_kmer * ratio)); }
    bool forbid_long_way = false;      // heavy-hitter pre-aggregation: a task the aggregating finish cannot handle is reported, not redone
};

// The staging words at the end of hsk_ctx::pinned: small device results the host waits for, and host words a copy reads.  One field per
// user, at the offset the user has always had (the kernels and copies see the same addresses); a field with several users says why
// they are never live together.
struct PinnedTail {
    unsigned char agg[2][512];         // agg_stage1 / agg_stage2: the AggHostRead of the batch in slot 0 / 1
    unsigned char agg_large[2][512];   // agg_stage1: host copy of the batch's eight AggLarge structs (slot 0 / 1) until the copy to the device has run
    u64 pairs[2][16];                  // combining extraction: pairs per task + error word of the batch in slot 0 / 1 (combine_batch -> process_rank)
    u64 read_pairs[8];                 // hsk_result_pairs: record count, row count, self records, keys, error word -- copied, waited for and read on the spot
    unsigned char free1[1280 - 64];
    u64 estimate[16];                  // estimate_plan: the sample's counters
    unsigned char free2[64];
    u32 parse_flags[16];               // the parse's verdict words (ParseFlags, hsk_host_parse.h: read_parse_flags writes, the drivers read).  One parse per attempt:
                                       // the pipelined ingest has read its words before it falls back to parse_count
    alignas(64) u64 packed_bytes;      // the last read offset on its way to the device: one entry point per call writes it, and every call ends with a wait
    alignas(64) u32 sort_flag;         // sort_task_device: a long bin with several keys
    alignas(64) u64 total;             // count_task_device, merge_sorted_pairs, hsk_format: entries kept -- copied, waited for and read on the spot
    alignas(64) u32 err;               // the sticky device error word: check_device_error and the end of process_rank, each copy, wait and read in one go
};
static_assert(sizeof(PinnedTail) == 4096, "the staging words are the last 4096 bytes of the pinned block");
static_assert(offsetof(PinnedTail, agg) == 4096 - 4096 && offsetof(PinnedTail, agg_large) == 4096 - 3072 && offsetof(PinnedTail, pairs) == 4096 - 2048 && offsetof(PinnedTail, estimate) == 4096 - 512, "staging offsets");
static_assert(offsetof(PinnedTail, parse_flags) == 4096 - 320 && offsetof(PinnedTail, packed_bytes) == 4096 - 256 && offsetof(PinnedTail, sort_flag) == 4096 - 192, "staging offsets");
static_assert(offsetof(PinnedTail, total) == 4096 - 128 && offsetof(PinnedTail, err) == 4096 - 64, "staging offsets");
static PinnedTail *staging(hsk_ctx *c) { return (PinnedTail *)((char *)c->pinned + c->pinned_bytes - sizeof(PinnedTail)); }

static int fail(hsk_ctx *c, int code, const char *fmt, ...)
{
    if (c) {
        va_list ap; va_start(ap, fmt);
        vsnprintf(c->err, sizeof c->err, fmt, ap);
        va_end(ap);
    }
    return code;
}

#define HIPCHK(c, call)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail(c, HSK_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define DALLOC(c, ptr, type, bytes)                                                              \
    do {                                                                                         \
        ptr = (type)(c)->pool.alloc(bytes, __FILE__, __LINE__);                                  \
        if (!ptr) return fail(c, HSK_ERR_OOM, "device allocation of %zu bytes failed (%s:%d)", (size_t)(bytes), __FILE__, __LINE__); \
    } while (0)

// HSK_TIMING=1 (diagnostic): host-side wall-clock marks of one hsk_count call on stderr
#include <chrono>
constexpr int HSK_RETRY_PLAN = -2000;               // internal: the call is run again with another plan (dispatch_pipeline; never returned to the caller)
static bool timing_enabled() { static const bool on = getenv("HSK_TIMING") && atoi(getenv("HSK_TIMING")) != 0; return on; }
// a call that starts again with another plan says why when HSK_TIMING is set
static int retry_plan(const char *why, unsigned info = 0) { if (timing_enabled()) fprintf(stderr, "[hsk] the call starts again without the combining extraction: %s (%u)\n", why, info); return HSK_RETRY_PLAN; }
static void tmark(const char *what)
{
    if (!timing_enabled()) return;
    static auto t0 = std::chrono::steady_clock::now();
    static auto last = t0;
    const auto now = std::chrono::steady_clock::now();
    if (!what) { t0 = last = now; return; }
    fprintf(stderr, "[hsk %8.2f ms  +%7.2f] %s\n", std::chrono::duration<double, std::milli>(now - t0).count(), std::chrono::duration<double, std::milli>(now - last).count(), what);
    last = now;
}

// pool_redzone (tests): the device side of DevPool's red zones -- the fill on the context's stream, and one kernel that compares every zone
// with the pattern.  Its result is a word of its own (words 16..31 of d_err are census scratch), in a buffer that is not the pool's.
static void pool_hip_fill(void *arg, void *p, size_t n) { (void)hipMemsetAsync(p, DevPool::RZ_BYTE, n, ((hsk_ctx *)arg)->stream); }

__global__ void redzone_check_kernel(const unsigned long long *zones, u32 nz, unsigned long long *first_bad)
{
    for (u32 z = blockIdx.x; z < nz; z += gridDim.x) {
        const unsigned char *p = (const unsigned char *)zones[2 * z];
        const unsigned long long n = zones[2 * z + 1];
        for (unsigned long long i = threadIdx.x; i < n; i += blockDim.x)
            if (p[i] != DevPool::RZ_BYTE) { atomicMin(first_bad, ((unsigned long long)z << 32) | i); break; }
    }
}

static int pool_hip_check(void *arg, const DevPool::Zone *z, size_t nz, size_t *bad_zone, size_t *bad_off)
{
    hsk_ctx *c = (hsk_ctx *)arg;
    std::vector<unsigned long long> h(2 * nz + 1);
    for (size_t i = 0; i < nz; ++i) { h[2 * i] = (unsigned long long)(uintptr_t)z[i].p; h[2 * i + 1] = z[i].bytes; }
    h[2 * nz] = ~0ull;
    unsigned long long *d = nullptr, res = ~0ull;
    if (hipMalloc(&d, h.size() * 8) != hipSuccess) { (void)hipGetLastError(); return -1; }
    bool ok = hipMemcpyAsync(d, h.data(), h.size() * 8, hipMemcpyHostToDevice, c->stream) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(redzone_check_kernel, dim3((u32)std::min<size_t>(nz, 1024)), dim3(256), 0, c->stream, d, (u32)nz, d + 2 * nz);
        ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(&res, d + 2 * nz, 8, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
             hipStreamSynchronize(c->stream) == hipSuccess;
    }
    (void)hipFree(d);
    if (!ok) return -1;
    if (res == ~0ull) return 0;
    *bad_zone = (size_t)(res >> 32); *bad_off = (size_t)(res & 0xffffffffu);
    return 1;
}

// every blocking wait of the host on a stream inside the counting path goes through here (hsk_stats.host_syncs)
static hipError_t hsk_sync(hsk_ctx *c, hipStream_t s) { c->stats.host_syncs++; return hipStreamSynchronize(s); }

static hipEvent_t ev_get(hsk_ctx *c)
{
    if (!c->ev_free.empty()) { hipEvent_t e = c->ev_free.back(); c->ev_free.pop_back(); return e; }
    hipEvent_t e; (void)hipEventCreate(&e); return e;
}
static void ev_put(hsk_ctx *c, hipEvent_t e) { c->ev_free.push_back(e); }

// events of one scope: handed back to the pool on every way out (the early returns of HIPCHK included)
struct EvList {
    hsk_ctx *c; std::vector<hipEvent_t> v;
    explicit EvList(hsk_ctx *c_) : c(c_) {}
    hipEvent_t get() { v.push_back(ev_get(c)); return v.back(); }
    ~EvList() { for (auto e : v) ev_put(c, e); }
};

// phase timer: records an event pair on the stream, elapsed time is summed after the final sync
struct PhaseTimer {
    hsk_ctx *c; std::vector<std::pair<hipEvent_t, hipEvent_t>> pairs[8];
    explicit PhaseTimer(hsk_ctx *c_) : c(c_) {}
    void begin(int ph, hipStream_t s = nullptr) { hipEvent_t a = ev_get(c); (void)hipEventRecord(a, s ? s : c->stream); pairs[ph].push_back({a, nullptr}); }
    void end(int ph, hipStream_t s = nullptr) { hipEvent_t b = ev_get(c); (void)hipEventRecord(b, s ? s : c->stream); pairs[ph].back().second = b; }
    double collect(int ph)
    {
        double ms = 0;
        for (auto &p : pairs[ph]) {
            float f = 0;
            if (p.second && hipEventElapsedTime(&f, p.first, p.second) == hipSuccess) ms += f;
            ev_put(c, p.first); if (p.second) ev_put(c, p.second);
        }
        pairs[ph].clear();
        return ms;
    }
};
enum { PH_TOTAL = 0, PH_PARSE, PH_EXCH, PH_EXTRACT, PH_SORT, PH_COUNT, PH_D2H };
