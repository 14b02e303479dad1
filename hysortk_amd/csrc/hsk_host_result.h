// hsk_host_result.h -- a rank's result on its way to the host: copies that overlap the kernels, host threads that widen compact batches,
// the assembly of the list in ascending task id.
// Part of the single translation unit hsk_api.hip (included in this order; everything here is file-local).
#pragma once

constexpr u32 EMPTY_TASK = ~0u;                                     // the empty place of a padded batch (process_rank)
// The prefix form of a task's n entries (one-word keys): low 32 key bits, next 16, counts of cw bytes, directory (padded to 16 bytes) -- each rounded
// up to 16 bytes.  Offsets from the task's start (lo32 at 0) and the size of the whole.
struct PrefixForm { size_t mid16, cnt, dir, total; };
static PrefixForm prefix_form(u64 n, int cw)
{
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    PrefixForm f; f.mid16 = up16((size_t)n * 4); f.cnt = f.mid16 + up16((size_t)n * 2); f.dir = f.cnt + up16((size_t)n * cw); f.total = f.dir + (size_t)65537 * 4 + 12;
    return f;
}

// Host threads that widen compact result batches (pack_entries_kernel's k-mer words + 16-bit counts, copied into pinned staging)
// into the caller-visible entries while the GPU counts the next batches.  Every thread of a batch waits for the batch's copy
// event, then takes its slice.  The destructor joins: no thread outlives the call that started it.
struct WidenPiece {                                                 // one task's share of a batch
    hipEvent_t copied; const u64 *keys; const unsigned short *cnts; u64 *dst; u64 n;
    // prefix form (one-word keys): low 48 key bits as u32 + u16, counts of cw bytes, dir[p] = first entry of prefix p (dir[65536] = n)
    const u32 *lo32 = nullptr; const unsigned short *mid16 = nullptr; const u8 *cnt8 = nullptr; const u32 *dir = nullptr; int cw = 0;
};
struct WidenPool {
    hsk_ctx *c;
    std::vector<std::thread> th;
    std::vector<hipEvent_t> evs;
    explicit WidenPool(hsk_ctx *c_) : c(c_) {}
    int nthreads() const                                            // (asked by add(), on the thread of the call: the pool's threads read no setting)
    {
        { const int v = (int)c->tune.widen_threads; if (v > 0) return std::min(v, 64); }
        static const int n = []() { const unsigned hc = std::thread::hardware_concurrency(); return (int)std::min<unsigned>(32, std::max<unsigned>(2, hc / 2)); }();
        return n;
    }
    // A batch arrives task by task (one copy + one event per piece): thread t widens slice t of every piece in turn, so that all
    // threads are done shortly after the LAST piece has landed -- the tail of the call is one piece's widening, not one batch's.
    void add(const std::vector<WidenPiece> &pieces, int nw)
    {
        for (auto &p : pieces) evs.push_back(p.copied);
        const int nt = nthreads(), dev = c->cfg.device;
        for (int t = 0; t < nt; ++t) {
            th.emplace_back([=]() {
                (void)hipSetDevice(dev);
                for (const WidenPiece &p : pieces) {
                    (void)hipEventSynchronize(p.copied);
                    const u64 lo = p.n * (u64)t / nt, hi = p.n * (u64)(t + 1) / nt;
                    const u64 *keys = p.keys; const unsigned short *cnts = p.cnts; u64 *dst = p.dst;
                    if (p.dir) {                                       // prefix form: the top 16 key bits come from the directory
                        if (lo >= hi) continue;
                        typedef unsigned long long v2u64p __attribute__((vector_size(16)));
                        u32 pl = 0, ph = 65536;                        // last prefix that starts at or before entry lo
                        while (ph - pl > 1) { const u32 mid = (pl + ph) >> 1; if ((u64)p.dir[mid] <= lo) pl = mid; else ph = mid; }
                        u32 pre = pl; u64 next = p.dir[pre + 1];
                        const bool nt = ((uintptr_t)dst & 15) == 0;
                        for (u64 i = lo; i < hi; ++i) {
                            while (i >= next) { ++pre; next = p.dir[pre + 1]; }
                            const unsigned long long key = ((unsigned long long)pre << 48) | ((unsigned long long)p.mid16[i] << 32) | p.lo32[i];
                            const unsigned long long cv = p.cw == 1 ? (unsigned long long)p.cnt8[i] : (unsigned long long)reinterpret_cast<const unsigned short *>(p.cnt8)[i];
                            if (nt) { const v2u64p e = {key, cv}; __builtin_nontemporal_store(e, (v2u64p *)dst + i); }
                            else { dst[2 * i] = key; dst[2 * i + 1] = cv; }
                        }
                        continue;
                    }
                    // one-word keys: an entry is one aligned 16-byte store that nobody reads back soon -- non-temporal (no read for
                    // ownership: a plain store loop is bound by the cache lines it first has to fetch)
                    typedef unsigned long long v2u64 __attribute__((vector_size(16)));
                    if (nw == 1 && ((uintptr_t)dst & 15) == 0) for (u64 i = lo; i < hi; ++i) { const v2u64 e = {keys[i], (unsigned long long)cnts[i]}; __builtin_nontemporal_store(e, (v2u64 *)dst + i); }
                    else if (nw == 1) for (u64 i = lo; i < hi; ++i) { dst[2 * i] = keys[i]; dst[2 * i + 1] = cnts[i]; }
                    else for (u64 i = lo; i < hi; ++i) { for (int w = 0; w < nw; ++w) dst[i * (nw + 1) + w] = keys[i * nw + w]; dst[i * (nw + 1) + nw] = cnts[i]; }
                }
            });
        }
    }
    void join() { for (auto &t : th) if (t.joinable()) t.join(); th.clear(); for (auto e : evs) ev_put(c, e); evs.clear(); }
    ~WidenPool() { join(); }
};

// What a rank has counted (touts, the histogram) and how it reaches the caller.  Host result, no payload, tasks finished in ascending id:
// every finished batch is copied while the next ones are counted (copy_batch).  The pinned block is sized from the entries-per-k-mer ratio of
// the previous call (or of this call's first batch); should the list outgrow it, the early copies are given up and everything is copied
// at the end (finish_list).  process_rank keeps the order of the calls: copy_batch per batch, finish_list, drain.
template <int NW>
struct ResultCopier {
    hsk_ctx *c; ResultPriv *rp; const std::vector<TaskSegs> &segs; const u32 ntasks; const u64 total_kmers; const bool ext, keep, profile_ev;
    // compact copies: counts fit 16 bits whenever the filter's upper bound does.  tuning "compact_d2h": 0 entries as they are (16 bytes), 1 k-mer
    // words + 16-bit counts (10 bytes), 2 (default) the prefix form for one-word keys (7 bytes with U <= 255, else 8; + 256 KB of directory per task)
    const int compact_mode; const bool compact;
    std::vector<TaskOut> touts;                           // [task] what the finish left in HBM
    u64 *d_histo = nullptr; u32 histo_len = 0;
    bool early;                                           // early copies are still worth trying (given up for good on the first doubt)
    u64 *early_buf = nullptr; u64 early_cap = 0, early_used = 0, compact_bytes = 0, compact_entries = 0;
    std::vector<void *> pk_dev, pk_host;                  // device / pinned staging of the compact batches (handed back when the call ends)
    std::vector<u8> copied; std::vector<EvPair> d2h_ev; WidenPool widen;
    ResultCopier(hsk_ctx *c_, ResultPriv *rp_, const std::vector<TaskSegs> &segs_, u32 ntasks_, u64 total_kmers_, bool early_, int compact_mode_)
        : c(c_), rp(rp_), segs(segs_), ntasks(ntasks_), total_kmers(total_kmers_), ext(c_->cfg.extension != 0), keep((c_->cfg.flags & HSK_FLAG_KEEP_DEVICE) != 0),
          profile_ev((c_->cfg.flags & HSK_FLAG_PROFILE) != 0), compact_mode(compact_mode_), compact(compact_mode_ > 0 && c_->cfg.upper_freq <= 65535),
          touts(ntasks_), early(early_), copied(ntasks_, 0), widen(c_) {}
    // the outputs of a batch's finish: fo[i] belongs to task tk[i]
    void take(const u32 *tk, const TaskOut *fo) { for (int i = 0; i < XCD_BATCH; ++i) if (tk[i] != EMPTY_TASK) touts[tk[i]] = fo[i]; }

    int copy_batch(const u32 *tasks, int ntk)
    {
        if (!early) return HSK_OK;
        u64 nb = 0, kb = 0;
        for (int i = 0; i < ntk; ++i) if (tasks[i] != EMPTY_TASK) { nb += touts[tasks[i]].n; kb += segs[tasks[i]].nkmers; }
        if (!early_buf) {
            const double ratio = c->entries_per_kmer > 0 ? c->entries_per_kmer : (kb ? (double)nb / (double)kb : 1.0);
            early_cap = (u64)(ratio * 1.08 * (double)total_kmers) + (1u << 16);
            if (early_cap * (NW + 1) * 8 > (64ULL << 30)) { early = false; return HSK_OK; }      // not worth pinning that much on a guess
            early_buf = (u64 *)host_alloc(c, rp, early_cap * (NW + 1) * 8);
            if (!early_buf) { early = false; return HSK_OK; }
        }
        if (early_used + nb > early_cap) { early = false; return HSK_OK; }                       // the guess was too small: copy at the end
        // compact: every task's entries are packed on the main stream ([k-mer words][16-bit counts], 16-byte aligned per task), copied
        // task by task into pinned staging and widened into early_buf by host threads while the next batch is counted
        u8 *d_pk = nullptr, *h_pk = nullptr;
        size_t pk_off[XCD_BATCH + 1] = {0}, pk_len[XCD_BATCH] = {0};
        // one-word keys: the prefix form (7 or 8 bytes per entry + a 256 KB directory per task); otherwise k-mer words + 16-bit counts
        const bool prefix = NW == 1 && compact_mode >= 2;
        const int cw = c->cfg.upper_freq <= 255 ? 1 : 2;
        if (compact && nb) {
            bool fits = true;
            for (int i = 0; i < ntk; ++i) {
                const u64 n_i = (tasks[i] == EMPTY_TASK) ? 0 : touts[tasks[i]].n;
                if (n_i >= 0xFFFFFFF0ULL) fits = false;
                pk_len[i] = prefix ? (n_i ? prefix_form(n_i, cw).total : 0) : (size_t)n_i * (NW * 8 + 2);
                pk_off[i + 1] = pk_off[i] + ((pk_len[i] + 15) & ~(size_t)15);
            }
            const size_t pk_bytes = pk_off[ntk] + 64;
            if (fits) { d_pk = (u8 *)c->pool.alloc(pk_bytes); h_pk = (u8 *)host_alloc(c, rp, pk_bytes); }
            if (!d_pk || !h_pk) { c->pool.release(d_pk); if (h_pk) host_release(c, rp, h_pk); d_pk = nullptr; h_pk = nullptr; }      // (no room: this batch travels as it is)
            else {
                pk_dev.push_back(d_pk); pk_host.push_back(h_pk);
                for (int i = 0; i < ntk; ++i) {
                    if (tasks[i] == EMPTY_TASK || !touts[tasks[i]].n) continue;
                    const TaskOut &to = touts[tasks[i]];
                    const u32 grid = (u32)std::min<u64>((to.n + 255) / 256, 2048);
                    u8 *b = d_pk + pk_off[i];
                    if (prefix) {
                        if constexpr (NW == 1) {
                            const PrefixForm f = prefix_form(to.n, cw);
                            u32 *lo32 = (u32 *)b, *dir = (u32 *)(b + f.dir); unsigned short *mid16 = (unsigned short *)(b + f.mid16); u8 *cnt = b + f.cnt;
                            HIPCHK(c, hipMemsetAsync(dir, 0xFF, (size_t)65537 * 4, c->stream));
                            if (cw == 1) hipLaunchKernelGGL((pack_entries_prefix_kernel<u8>), dim3(grid), dim3(256), 0, c->stream, to.entries, to.n, lo32, mid16, cnt, dir);
                            else hipLaunchKernelGGL((pack_entries_prefix_kernel<unsigned short>), dim3(grid), dim3(256), 0, c->stream, to.entries, to.n, lo32, mid16, (unsigned short *)cnt, dir);
                            hipLaunchKernelGGL(pack_dir_close_kernel, dim3(1), dim3(1024), 0, c->stream, dir, (u32)to.n);
                        }
                    } else hipLaunchKernelGGL(pack_entries_kernel, dim3(grid), dim3(256), 0, c->stream, to.entries, to.n, NW, (u64 *)b, (unsigned short *)(b + (size_t)to.n * NW * 8));
                }
            }
        }
        hipEvent_t done = ev_get(c);
        HIPCHK(c, hipEventRecord(done, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->d2h_stream, done, 0));
        ev_put(c, done);
        EvPair ep{}; if (profile_ev) { ep.a = ev_get(c); ep.b = ev_get(c); ep.kind = 6; (void)hipEventRecord(ep.a, c->d2h_stream); }
        if (d_pk) {
            std::vector<WidenPiece> pieces;
            u64 o = 0;
            for (int i = 0; i < ntk; ++i) {
                if (tasks[i] == EMPTY_TASK || !touts[tasks[i]].n) continue;
                const u64 n_i = touts[tasks[i]].n;
                HIPCHK(c, hipMemcpyAsync(h_pk + pk_off[i], d_pk + pk_off[i], pk_len[i], hipMemcpyDeviceToHost, c->d2h_stream));
                WidenPiece wp; wp.copied = ev_get(c);
                HIPCHK(c, hipEventRecord(wp.copied, c->d2h_stream));
                wp.keys = nullptr; wp.cnts = nullptr;
                const u8 *b = h_pk + pk_off[i];
                if (prefix) {
                    const PrefixForm f = prefix_form(n_i, cw);
                    wp.lo32 = (const u32 *)b; wp.mid16 = (const unsigned short *)(b + f.mid16); wp.cnt8 = b + f.cnt; wp.dir = (const u32 *)(b + f.dir); wp.cw = cw;
                } else { wp.keys = (const u64 *)b; wp.cnts = (const unsigned short *)(b + (size_t)n_i * NW * 8); }
                wp.dst = early_buf + (early_used + o) * (NW + 1); wp.n = n_i;
                pieces.push_back(wp);
                o += n_i;
                compact_bytes += pk_len[i];
            }
            widen.add(pieces, NW);
            compact_entries += nb;
        }
        for (int i = 0; i < ntk; ++i) {
            const u32 t = tasks[i];
            if (t == EMPTY_TASK) continue;
            TaskOut &to = touts[t];
            if (to.n && !d_pk) HIPCHK(c, hipMemcpyAsync(early_buf + early_used * (NW + 1), to.entries, to.n * (NW + 1) * 8, hipMemcpyDeviceToHost, c->d2h_stream));
            early_used += to.n; copied[t] = 1;
        }
        if (profile_ev) { (void)hipEventRecord(ep.b, c->d2h_stream); d2h_ev.push_back(ep); }
        return HSK_OK;
    }

    // every task is finished: the list's blocks, and whatever the early copies have not brought over, on the main stream
    int finish_list(hsk_result *out, u64 n_total, u64 pay_total)
    {
        out->n = n_total;
        out->task_off = (uint64_t *)host_alloc(c, rp, (size_t)(ntasks + 1) * 8);
        out->histo = (uint64_t *)host_alloc(c, rp, (size_t)histo_len * 8);
        out->histo_len = histo_len;
        if (!out->task_off || !out->histo) return fail(c, HSK_ERR_OOM, "pinned host allocation failed");
        HIPCHK(c, hipMemcpyAsync(out->histo, d_histo, (size_t)histo_len * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&staging(c)->err, c->d_err, 4, hipMemcpyDeviceToHost, c->stream));      // the sticky device error word travels with the result
        if (!keep) {
            // the early copies are good if they stayed inside the block and cover a prefix of the list (tasks in ascending id)
            bool early_ok = early_buf != nullptr && early && n_total <= early_cap;
            if (early_ok) { bool gap = false; for (u32 t = 0; t < ntasks && early_ok; ++t) { if (!touts[t].n) continue; if (!copied[t]) gap = true; else if (gap) early_ok = false; } }
            if (early_buf && !early_ok) { HIPCHK(c, hsk_sync(c, c->d2h_stream)); widen.join(); host_release(c, rp, early_buf); early_buf = nullptr; std::fill(copied.begin(), copied.end(), 0); compact_bytes = compact_entries = 0; }
            out->entries = early_buf ? early_buf : (uint64_t *)host_alloc(c, rp, n_total * (NW + 1) * 8);
            if (!out->entries) return fail(c, HSK_ERR_OOM, "pinned host allocation of %llu bytes failed", (unsigned long long)(n_total * (NW + 1) * 8));
            if (ext) {
                out->payload_off = (uint64_t *)host_alloc(c, rp, (n_total + 1) * 8);
                out->pos = (uint32_t *)host_alloc(c, rp, pay_total * 4);
                out->rid = (int32_t *)host_alloc(c, rp, pay_total * 4);
                if (!out->payload_off || !out->pos || !out->rid) return fail(c, HSK_ERR_OOM, "pinned host allocation failed");
            }
        }
        EvPair d2h_tail{}; if (profile_ev && !keep) { d2h_tail.a = ev_get(c); d2h_tail.b = ev_get(c); d2h_tail.kind = 6; (void)hipEventRecord(d2h_tail.a, c->stream); }
        u64 o = 0, po = 0;
        for (u32 t = 0; t < ntasks; ++t) {
            out->task_off[t] = o;
            TaskOut &to = touts[t];
            if (!keep) {
                if (to.n && !copied[t]) HIPCHK(c, hipMemcpyAsync(out->entries + o * (NW + 1), to.entries, to.n * (NW + 1) * 8, hipMemcpyDeviceToHost, c->stream));
                if (ext && to.n) HIPCHK(c, hipMemcpyAsync(out->payload_off + o, to.payoff, to.n * 8, hipMemcpyDeviceToHost, c->stream));
                if (ext && to.npay) {
                    HIPCHK(c, hipMemcpyAsync(out->pos + po, to.pos, to.npay * 4, hipMemcpyDeviceToHost, c->stream));
                    HIPCHK(c, hipMemcpyAsync(out->rid + po, to.rid, to.npay * 4, hipMemcpyDeviceToHost, c->stream));
                }
            }
            o += to.n; po += to.npay;
        }
        out->task_off[ntasks] = o;
        if (profile_ev && !keep) { (void)hipEventRecord(d2h_tail.b, c->stream); d2h_ev.push_back(d2h_tail); }
        if (!keep) c->stats.d2h_bytes += (n_total - compact_entries) * (NW + 1) * 8 + compact_bytes + (ext ? (n_total + 1) * 8 + pay_total * 8 : 0);
        return HSK_OK;
    }

    // waits for everything finish_list and copy_batch have enqueued, and hands the staging back
    int drain()
    {
        HIPCHK(c, hsk_sync(c, c->stream));
        tmark("main stream drained");
        if (early_buf) HIPCHK(c, hsk_sync(c, c->d2h_stream));
        tmark("copy stream drained");
        widen.join();                                         // the last batch's entries are being widened
        for (void *p : pk_dev) c->pool.release(p);
        for (void *p : pk_host) host_release(c, rp, p);
        tmark("entries widened");
        for (auto &e : d2h_ev) c->ev_pending.push_back(e);
        return HSK_OK;
    }
};
