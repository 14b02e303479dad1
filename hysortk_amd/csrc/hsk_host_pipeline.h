// hsk_host_pipeline.h -- the whole path: exchange feeder, heavy-hitter lists, per-rank task loop, single-GPU / RCCL / virtual-rank drivers.
// Part of the single translation unit hsk_api.hip (included in this order; everything here is file-local).
#pragma once

// ------------------------------------------------------------------------------------------------
// Exchange / sort overlap (multi-GPU).  The owned tasks of every rank are cut into groups of
// XCD_BATCH consecutive tasks; group g+1 travels on `comm_stream` (RCCL send/recv, or device copies
// between the virtual ranks of the loopback driver) while group g is expanded, sorted and counted on
// the main stream.  The reference overlaps the same way with BATCH-sized MPI_Ialltoallv rounds
// (src/kmerops.cpp:130-196, exchange_supermer's stage loop); here the unit is a task group so that a
// sort batch never waits for bytes it does not need.  tuning "overlap=0" selects one exchange up front.
// ------------------------------------------------------------------------------------------------
static int estimate_plan(hsk_ctx *c, const u8 *d_packed, u64 packed_bytes, const u64 *d_roff, const u32 *d_rlen, u64 nreads, int nranks);      // hsk_api.hip
static u32 certain_drop_mask(hsk_ctx *c);                                                                                                          // hsk_api.hip

struct TaskInput { const u8 *len; BaseSource src; const u32 *pos; const int32_t *rid; const unsigned short *sub16 = nullptr; };

// HSK_TEST_FAIL="<rank>:<site>" (tests/test_gpu_rccl.py, read at every call): the named step of that rank fails as if an allocation had returned null.
// Sites: sortbuf (before the first task group travels), group1 (the exchange buffers of the second group: peers are already inside the exchange), late
// (the second batch: everything is in flight); and, in front of the status-carrying all-reduces before the exchange: parse (parse_count's result, several
// ranks only), place (parse_place's result), heavy (heavy_preaggregate's result), heavybuf (the owner's receive buffers of the heavy lists).
static bool test_fail(hsk_ctx *c, const char *site)
{
    const char *e = getenv("HSK_TEST_FAIL");
    if (!e || !*e) return false;
    const char *colon = strchr(e, ':');
    return colon && atoi(e) == c->comm.rank && strcmp(colon + 1, site) == 0;
}

// virtual ranks: the share that rank `src` sends to rank `dst` under their plans sp and p, from src's store into dst's receive arrays, by device copies
static int copy_share(hsk_ctx *c, const SupermerStore &ss, const ExchangePlan &sp, int src, const ExchangeBuffers &b, const ExchangePlan &p, int dst, bool ext, bool with_sub, hipStream_t s, int g = -1)
{
    const u64 n = sp.send_sup[dst], nb = sp.send_bytes[dst];
    if (n != p.recv_sup[src] || nb != p.recv_bytes[src])
        return g < 0 ? fail(c, HSK_ERR_INTERNAL, "exchange plan mismatch %d->%d", src, dst) : fail(c, HSK_ERR_INTERNAL, "exchange plan mismatch %d->%d (group %d)", src, dst, g);
    if (!n) return HSK_OK;
    HIPCHK(c, hipMemcpyAsync(b.len + p.recv_sup_off[src], ss.sm_len + sp.send_sup_off[dst], n, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipMemcpyAsync(b.bytes + p.recv_byte_off[src], ss.sm_bytes + sp.send_byte_off[dst], nb, hipMemcpyDeviceToDevice, s));
    if (with_sub) HIPCHK(c, hipMemcpyAsync(b.sub16 + p.recv_sup_off[src], ss.sm_sub16 + sp.send_sup_off[dst], n * 2, hipMemcpyDeviceToDevice, s));
    if (ext) {
        HIPCHK(c, hipMemcpyAsync(b.pos + p.recv_sup_off[src], ss.sm_pos + sp.send_sup_off[dst], n * 4, hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipMemcpyAsync(b.rid + p.recv_sup_off[src], ss.sm_rid + sp.send_sup_off[dst], n * 4, hipMemcpyDeviceToDevice, s));
    }
    return HSK_OK;
}

struct GroupFeeder {
    hsk_ctx *c = nullptr;
    int nranks = 1, rank = 0, ngroups = 0;
    bool ext = false;
    std::vector<int32_t> group_of;                     // task -> group inside its owner's task list
    std::vector<ExchangePlan> pl;                      // [group] this rank's plan
    std::vector<ExchangeBuffers> xb;                   // [group] receive arrays, alive from post to release
    std::vector<hipEvent_t> arrived;                   // [group] recorded on comm_stream after the transfer
    int posted = 0, released = 0;
    // transport: RCCL (store of this rank) or loopback (stores and plans of all virtual ranks)
    SupermerStore *st = nullptr;
    std::vector<SupermerStore> *st_all = nullptr;
    std::vector<std::vector<PackJob>> packs;           // [group] byte-packing jobs issued with the group (scratch released with it)
    bool lazy_pack = false;                            // the stores' bytes are produced group by group (pack_group_*)
    bool live = false;                                 // RCCL: every rank got past the last agreement before the exchange and will post every group
    bool with_sub = false;                             // every rank's store carries the supermers' minimizer bits (sm_sub16): they travel, the owners take the combining extraction
    const std::vector<std::vector<ExchangePlan>> *pl_all = nullptr;     // [rank][group]
    u64 bytes_moved = 0;

    int plan(hsk_ctx *c_, int nranks_, int rank_, u32 ntasks, const std::vector<int32_t> &owner, const std::vector<u32> &order,
             const std::vector<u64> &M, const std::vector<u64> &task_base, std::vector<TaskSegs> &segs)
    {
        c = c_; nranks = nranks_; rank = rank_; ext = c->cfg.extension != 0;
        assign_task_groups(nranks, ntasks, owner, XCD_BATCH, group_of, ngroups);
        pl.resize(ngroups); xb.resize(ngroups); arrived.assign(ngroups, nullptr); packs.assign(ngroups, std::vector<PackJob>());
        segs.assign(ntasks, TaskSegs());
        for (int g = 0; g < ngroups; ++g) plan_exchange(nranks, rank, ntasks, owner, order, M, task_base, pl[g], segs, &group_of, g);
        return HSK_OK;
    }
    int post(int g)
    {
        ExchangeBuffers &b = xb[g]; const ExchangePlan &p = pl[g];
        if (g == 1 && !draining && test_fail(c, "group1")) return fail(c, HSK_ERR_OOM, "exchange buffers of group %d (injected)", g);
        if (!b.alloc(c->pool, p, ext, with_sub)) return fail(c, HSK_ERR_OOM, "exchange buffers of group %d", g);
        // the bytes this group sends are packed now, on the communication stream (RCCL: this rank's store; virtual ranks:
        // the store of every source that has not produced group g yet)
        std::vector<SupermerStore *> to_pack;
        if (lazy_pack) {
            if (st_all) { for (int src = 0; src < nranks; ++src) { SupermerStore &ss = (*st_all)[src]; if (ss.group_packed.size() <= (size_t)g) ss.group_packed.resize(ngroups, 0); if (!ss.group_packed[g]) to_pack.push_back(&ss); } }
            else { if (st->group_packed.size() <= (size_t)g) st->group_packed.resize(ngroups, 0); if (!st->group_packed[g]) to_pack.push_back(st); }
            packs[g].resize(to_pack.size());
            for (size_t i = 0; i < to_pack.size(); ++i) {
                const ExchangePlan &sp = st_all ? (*pl_all)[(int)(to_pack[i] - &(*st_all)[0])][g] : p;
                int rc = pack_group_alloc(c, sp, nranks, packs[g][i]); if (rc) return rc;
            }
        }
        // the pool hands out blocks whose previous user may still be running on the main stream: order the
        // transfer after everything launched there so far (that is the work of group g-2 and earlier)
        hipEvent_t fence = ev_get(c);
        HIPCHK(c, hipEventRecord(fence, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->comm_stream, fence, 0));
        ev_put(c, fence);
        hipStream_t s = c->comm_stream;
        for (size_t i = 0; i < to_pack.size(); ++i) { int rc = pack_group_launch(c, *to_pack[i], packs[g][i], s); if (rc) return rc; to_pack[i]->group_packed[g] = 1; }
        if (st_all) {
            for (int src = 0; src < nranks; ++src) { int rc = copy_share(c, (*st_all)[src], (*pl_all)[src][g], src, b, p, rank, ext, with_sub, s, g); if (rc) return rc; }
        } else {
            int rc = post_exchange(c->comm, s, ext, p, st->sm_len, st->sm_bytes, st->sm_pos, st->sm_rid, b, with_sub ? st->sm_sub16 : nullptr);
            if (rc) return fail(c, HSK_ERR_COMM, "supermer exchange (group %d) failed: %d (%s)", g, rc, c->comm.last_error.c_str());
        }
        bytes_moved += p.recv_tot_bytes + p.recv_tot_sup * (ext ? 9 : 1) + (with_sub ? p.recv_tot_sup * 2 : 0);
        arrived[g] = ev_get(c);
        HIPCHK(c, hipEventRecord(arrived[g], s));
        return HSK_OK;
    }
    // the main stream is about to read group g: make sure g and g+1 are on their way, wait for g
    int need(int g)
    {
        const int upto = std::min(g + 1, ngroups - 1);
        while (posted <= upto) { int rc = post(posted); if (rc) return rc; ++posted; }
        HIPCHK(c, hipStreamWaitEvent(c->stream, arrived[g], 0));
        return HSK_OK;
    }
    // the main stream has launched its last reader of every group below g
    void release_below(int g)
    {
        for (; released < g && released < posted; ++released) drop_group(released);      // next user is ordered after the readers by post()'s fence (or is on the main stream)
    }
    void drop_group(int g)
    {
        xb[g].release(c->pool);
        for (auto &pj : packs[g]) expand_release(c, pj.x);
        packs[g].clear();
        if (arrived[g]) { ev_put(c, arrived[g]); arrived[g] = nullptr; }
    }
    // This rank's count has failed after the exchange began (RCCL only).  Its peers still expect its supermers and still send
    // it theirs: a rank that simply returned would leave them blocked in ncclRecv for ever (the reference dies together there:
    // MPI_Abort, src/kmerops.cpp:1477).  So the rank drains its own work, hands every device block the failed count allocated
    // (since `mark`: the supermer store stays) back to the pool -- a failed allocation is the usual reason to be here -- and posts
    // the remaining groups one by one, receiving into buffers it drops at once.  The ranks then agree on the outcome (agree_on_outcome)
    // and all return an error.
    bool draining = false;
    int drain_after_failure(unsigned long long mark)
    {
        draining = true;
        (void)hipStreamSynchronize(c->stream); (void)hipStreamSynchronize(c->comm_stream); (void)hipStreamSynchronize(c->d2h_stream);
        for (int g = 0; g < ngroups; ++g) { xb[g] = ExchangeBuffers(); packs[g].clear(); if (arrived[g]) { ev_put(c, arrived[g]); arrived[g] = nullptr; } }
        released = posted;
        c->pool.rollback(mark);
        for (; posted < ngroups; ++posted) {
            const int g = posted;
            int rc = post(g); if (rc) return rc;
            HIPCHK(c, hipStreamSynchronize(c->comm_stream));
            drop_group(g);
            released = g + 1;
        }
        return HSK_OK;
    }
    // every rank must take part in every group even when it owns no task of it
    int finish()
    {
        while (posted < ngroups) { int rc = post(posted); if (rc) return rc; ++posted; }
        HIPCHK(c, hsk_sync(c, c->comm_stream));
        release_below(ngroups);
        return HSK_OK;
    }
    TaskInput input(u32 t) const
    {
        const ExchangeBuffers &b = xb[group_of[t]];
        TaskInput in; in.len = b.len; in.src = source_from_bytes(b.bytes, b.nbytes); in.pos = b.pos; in.rid = b.rid; in.sub16 = b.sub16;
        return in;
    }
};

// ---- heavy-hitter tasks (a8): the owner's side --------------------------------------------------------------
// d_entries: the {k-mer, count} lists of all ranks for one task, concatenated (n entries, each list key-ordered,
// a key at most once per list).  Orders them by key with the count as payload, sums equal keys, filters [L, U].
template <int NW>
static int heavy_merge_task(hsk_ctx *c, const u64 *d_entries, u64 n, u64 *d_histo, u32 histo_len, TaskOut &out)
{
    out = TaskOut();
    if (n == 0) return HSK_OK;
    u64 *kA, *kB, *vA, *vB;
    DALLOC(c, kA, u64 *, n * NW * 8 + 64); DALLOC(c, kB, u64 *, n * NW * 8 + 64); DALLOC(c, vA, u64 *, n * 8 + 64); DALLOC(c, vB, u64 *, n * 8 + 64);
    hipLaunchKernelGGL(heavy_split_kernel<NW>, dim3((u32)std::min<u64>((n + HV_THREADS - 1) / HV_THREADS, 4096)), dim3(HV_THREADS), 0, c->stream, d_entries, n, kA, vA);
    SortScratch sc; int rc = alloc_sort_scratch(c, sc); if (rc) return rc;
    u64 *sk, *sv;
    rc = sort_task_device<NW>(c, kA, kB, vA, vB, n, c->cfg.kmer_size, sc, &sk, &sv);
    free_sort_scratch(c, sc);
    if (rc) return rc;
    rc = merge_sorted_pairs<NW>(c, sk, sv, n, d_histo, histo_len, out); if (rc) return rc;
    HIPCHK(c, hsk_sync(c, c->stream));
    c->pool.release(kA); c->pool.release(kB); c->pool.release(vA); c->pool.release(vB);
    return HSK_OK;
}

struct HeavyIn { u32 task; u64 *d_entries; u64 n; };       // a heavy task this rank owns: concatenated lists of all ranks
static void free_heavy_in(hsk_ctx *c, std::vector<HeavyIn> &hin) { for (auto &h : hin) c->pool.release(h.d_entries); hin.clear(); }
struct ProcExtra {
    bool force_batch = false;                              // every task through the batch kernels (partial batches padded)
    const std::vector<HeavyIn> *heavy_in = nullptr;        // merged and filtered here (they have no supermers)
    u32 vt_shift = 0;                                      // item-mode store: minimizer bits the parse's virtual tasks have consumed (a segment's virtual task: ExpSeg::byte_off)
    SupermerStore *items_store = nullptr;                  // item-mode store of one GPU: its items go back to the pool as soon as the bucket order has read them
};

static bool agg_is_off(const hsk_ctx *c, int nw) { return nw == 1 ? c->agg_off : c->agg_off_wide; }      // (run-time state: may change in the middle of a call)

// Result of an all-reduce with status (Comm::allreduce_with_status) -> return code of this rank: 0 everybody is fine; the transport failed; this
// rank (local_rc) or another one (peer_msg, may name `what` as %s) has failed since the last collective and all ranks leave together.
static int left_together(hsk_ctx *c, int st, const char *what, int local_rc, const char *peer_msg)
{
    if (st == 0) return HSK_OK;
    if (st < 0) return fail(c, HSK_ERR_COMM, "allreduce(%s) failed: %d (%s)", what, st, c->comm.last_error.c_str());
    return local_rc ? local_rc : fail(c, HSK_ERR_COMM, peer_msg, what);
}

// Step of its own, before the plan reads hsk_ctx::agg_off: this call's estimate says how many distinct keys a 16-bit prefix bin of the largest
// task holds -- the first table of the ladder, or no tables at all (most bins beyond 2048 slots: four prefix passes + the tile finish; what a batch
// used to find out the hard way, agg_stage2).  `items`: the store holds items (or virtual tasks), which only the aggregating finish can take.
static void first_table_from_estimate(hsk_ctx *c, int nw, u64 max_task, bool items)
{
    if (!c->call.est.valid || nw != 1 || c->cfg.extension || c->forbid_long_way || !max_task) return;
    const double d = c->call.est.distinct_per_kmer * (double)max_task / 65536.0;
    c->agg_first_cap = d <= 600.0 ? AG_LOG2CAP_SMALL : d <= 1250.0 ? AG_LOG2CAP_MEDIUM : AG_LOG2CAP_LARGE;
    if (d > 1450.0 && !items) { c->agg_off = true; c->agg_off_calls = 0; }
}

// What a rank's count will do, decided once (plan_rank) from the context's flags and tuning, the owned tasks' sizes, the feeder, the kind of
// store and ProcExtra; const afterwards.  What may change while the batches run (hsk_ctx::agg_off, agg_off_wide, combine_off, the result
// copier giving up its early copies) is not here: it is read where a batch needs it.
template <int NW>
struct RankPlan {
    static constexpr int XS_CH = XsCfg<(NW <= 2 ? NW : 1)>::CHUNK;
    bool ext = false; int K = 0; u64 max_task = 0;
    std::vector<u32> mine;             // the owned, non-empty tasks in ascending id; padded with EMPTY_TASK to whole batches where that pays
    bool batch = false;                // eight tasks at a time, one per XCD (a remainder: the single-task kernels)
    bool fused = false, agg = false, fused_ext = false;      // the finish a batch may take
    bool lag = false;                  // two batches in flight (two slots)
    bool xs = false;                   // expand fused with the first scatter pass
    bool item_mode = false, combine = false, fed_combine = false;      // the combining extraction: at all / on items the owner builds (several ranks)
    u64 rec_cap = 0;                   // records a task's sort buffers hold
    bool early = false; int compact_mode = 0;      // the result's way to the host (ResultCopier)
    int retry = HSK_OK;                // HSK_RETRY_PLAN: this store is no use to this plan, the call starts again
    int nslot() const { return lag ? 2 : 1; }
    int nsets() const { return batch ? XCD_BATCH : 1; }
    bool own_items() const { return combine && !fed_combine; }      // one GPU: the store holds the items, one bucket order for all tasks
};

template <int NW>
static RankPlan<NW> plan_rank(const hsk_ctx *c, u32 ntasks, const std::vector<int32_t> &owner, int rank, const std::vector<TaskSegs> &segs, u64 max_task, const GroupFeeder *feeder, bool item_mode, const ProcExtra *ex)
{
    RankPlan<NW> p; p.max_task = max_task; p.item_mode = item_mode;
    const bool ext = p.ext = c->cfg.extension != 0;
    const int K = p.K = c->cfg.kmer_size;
    // Tasks are sorted eight at a time, one per XCD (sort_batch_device); a remainder of fewer than eight
    // tasks goes through the single-task kernel.  tuning "xcd_batch=0" forces the single-task path.
    const bool batch_enabled = c->tune.xcd_batch != 0 && c->xcd_batch_ok;          // the one-task-per-XCD kernels need all eight XCDs (hsk_init's census)
    std::vector<u32> &mine = p.mine;
    for (u32 t = 0; t < ntasks; ++t) if (owner[t] == rank && segs[t].nkmers) mine.push_back(t);
    // several ranks, the supermers arrived with their minimizer bits: the owner builds the items, batch by batch (hsk_combine.h, 1b)
    const bool fed_wanted = NW <= 2 && feeder && feeder->with_sub && c->call.combine_now && !ext;
    const bool forced = ((ex && ex->force_batch) || item_mode || fed_wanted) && batch_enabled;      // (item-mode store: every task goes through whole batches)
    // a caller's task count below eight (the reference's default for one rank is five): three to seven tasks of some size still
    // go faster as one padded batch (5/8 of the batch path's rate) than one by one on the single-task path (about 1/3 of it)
    u64 mine_kmers = 0; for (u32 t : mine) mine_kmers += segs[t].nkmers;
    const bool small_batch = batch_enabled && mine.size() >= 3 && mine.size() < (size_t)XCD_BATCH && mine_kmers >= (1ULL << 25);
    // A remainder of three or more tasks is padded to a full batch with empty slots (an XCD without a task idles, which
    // still beats eight full-width passes per task on the single-task path); ex->force_batch pads any remainder.
    if ((batch_enabled && mine.size() >= (size_t)XCD_BATCH && mine.size() % XCD_BATCH >= 3) || (forced && !mine.empty()) || small_batch)
        while (mine.size() % XCD_BATCH) mine.push_back(EMPTY_TASK);
    const bool whole = mine.size() % XCD_BATCH == 0;
    p.batch = batch_enabled && mine.size() >= (size_t)XCD_BATCH;
    // fused finish: one-word keys (aggregating or tile finish), two-word keys with K >= 40 (aggregating finish only)
    p.fused = !ext && finish_enabled(c) && (NW == 1 ? hybrid_enabled(c) : (NW <= 3 && agg_enabled(c) && prefix_plan_ok<NW>(c, K, true)));
    p.agg = p.fused && agg_enabled(c);
    // EXTENSION with one-word keys: two passes on the top 16 bits (payload carried) + grouping aggregation
    p.fused_ext = ext && NW <= 3 && hybrid_enabled(c) && finish_enabled(c) && agg_enabled(c) && prefix_plan_ok<NW>(c, K, true);
    // Two batches in flight on ONE stream (two sets of sort buffers): the host enqueues expand / scatter / aggregation of
    // batch b + 1 BEFORE it waits for the aggregation totals of batch b, sizes batch b's outputs and enqueues its
    // compaction.  The GPU therefore never runs dry while the host waits (tuning "lag=0": one batch at a time, every wait drains
    // the stream).  An earlier version expanded batch b + 1 on a second stream beside the sort of batch b:
    // every kernel of the path already fills the chip, the gain was 1 %, and it is gone.
    // Measured (10 Gbp, 5 batches): the batch interval is the same with and without the lag (18.7 / 18.8 ms: a drained
    // stream costs well under 0.1 ms against ~19 ms of kernels per batch), but the lag delays every batch's compaction,
    // and with it the batch's result copy, by one batch: host results take 214 ms with it and 197 ms without.  Default: on
    // when the result stays in HBM (nothing to copy), off when it goes to the host; tuning "lag=0" / "=1" forces it.
    const bool keep_dev = (c->cfg.flags & HSK_FLAG_KEEP_DEVICE) != 0;
    const bool lag_enabled = c->tune.lag < 0 ? keep_dev : c->tune.lag != 0;
    p.lag = p.batch && p.agg && NW <= 2 && lag_enabled && mine.size() >= 2 * (size_t)XCD_BATCH;
    // expand fused with the first scatter pass (hsk_scatter.h): one-word keys, aggregating finish, whole batches
    // (EXTENSION: payload chunks beside the key chunks, tuning "fused_scatter_ext=0" turns that variant off; "fused_scatter_wide": two-word keys)
    p.xs = p.batch && (NW == 1 ? (!ext || c->tune.fused_scatter_ext != 0) : (NW == 2 && !ext && c->tune.fused_scatter_wide != 0 && prefix_top_bits(K, NW) == 16)) && c->tune.fused_scatter != 0 &&
           scatter_store_keys(max_task, p.XS_CH) < (1ULL << 32) && finish_enabled(c) && hybrid_enabled(c) && agg_enabled(c) && prefix_plan_ok<NW>(c, K, true);
    // the combining extraction (hsk_combine.h): the store carries the supermers' minimizer bits, whole batches, the aggregating finish
    // (an item-mode store holds nothing the instance path could read: every batch takes the combining extraction, or the call starts again
    //  without it)
    if constexpr (NW <= 2) {
        const bool can = p.xs && p.agg && !agg_is_off(c, NW) && whole;
        p.fed_combine = fed_wanted && !item_mode && can && p.batch;
        p.combine = (item_mode && can && !ext && !feeder) || p.fed_combine;
    }
    if (item_mode && !p.combine)
        p.retry = retry_plan("an item-mode store, but no batch to combine (xs / agg / batch)", (p.xs ? 1u : 0u) | (p.agg ? 2u : 0u) | (p.batch ? 4u : 0u) | (whole ? 8u : 0u));
    // The combining extraction's buffers hold {k-mer, count} PAIRS, not k-mers: with the call's own estimate of the input (estimate_plan: distinct k-mers
    // per k-mer) they are sized for four times the pairs it promises (+ 2 % of the k-mers) instead of one record per k-mer -- 20 GB instead of 102 at
    // 10 Gbp, and device memory is what a process's FIRST call pays for (~20-60 ms per GB mapped for the first time, tools/exp/malloc_cost.hip).  A call
    // whose pairs do not fit after all (error bit 512: the last chunk takes what runs over) starts again with full-sized buffers.  Several ranks: full
    // size (nobody starts again while peers wait).
    p.rec_cap = max_task;
    if (p.own_items() && !c->call.pair_cap_full) {
        if (c->call.est.valid && c->tune.pair_cap != 0)
            p.rec_cap = std::min<u64>(max_task, std::max<u64>((u64)((double)max_task * std::min(1.0, 4.0 * c->call.est.distinct_per_kmer * c->est_bias + 0.02)), 1ULL << 22));
        if (const long long forced_cap = c->tune.pair_cap_records; forced_cap > 0) p.rec_cap = std::min<u64>(max_task, (u64)forced_cap);      // (tests: stores that run over; the attempt after an overrun is full size)
    }
    // result copies that overlap the kernels: host result, no payload, tasks finished in ascending id (heavy tasks finish last, out of order)
    p.early = p.batch && p.agg && NW <= 2 && !keep_dev && !ext && c->tune.early_d2h != 0 && !(ex && ex->heavy_in && !ex->heavy_in->empty());
    p.compact_mode = (int)c->tune.compact_d2h;
    return p;
}

// The batch in flight in one slot: its buffers, what was decided for it when it was expanded, and the aggregation that waits for its totals.
struct BatchSlot {
    int index = 0;
    u64 *kA[XCD_BATCH] = {nullptr}, *kB[XCD_BATCH] = {nullptr}, *vA[XCD_BATCH] = {nullptr}, *vB[XCD_BATCH] = {nullptr};      // sort buffers (slot 0's first: also the single-task path)
    u64 *d_ghist = nullptr;                // [XCD_BATCH][MAX_PASSES][256]
    const u32 *tk = nullptr;               // the eight tasks (RankPlan::mine)
    BatchTask bt[XCD_BATCH];
    BucketOrder border_fed; FedItems fed_items;      // several ranks: the items and the bucket order of the batch
    ScatterBatch sbatch; PassDesc xs_plan[MAX_PASSES];
    bool combine = false;                  // the batch went through the combining extraction: its records are pairs
    int prefix = 0;                        // the digit plan the batch was expanded for
    // ... and which finish follows it: the aggregation (agg), the grouping aggregation of EXTENSION (fext), or -- once hsk_ctx::agg_off /
    // agg_off_wide have found the input to hold (nearly) only unique k-mers, possibly in the middle of a call -- the tile finish (one-word
    // keys) / full-width passes and the two-pass counter (everything else); follow: a finish that wants prefix passes only
    bool agg = false, fext = false, follow = false;
    AggPending pend;                       // the aggregation's second stage is still to come
};

template <int NW>
static int alloc_batch_buffers(hsk_ctx *c, const RankPlan<NW> &P, BatchSlot *slots, SortScratch &sc)
{
    // xs: the chunk store of the first pass (+ the chunk that takes what runs over)
    const u64 chunked = P.xs ? scatter_store_keys(P.rec_cap, P.XS_CH) + P.XS_CH : P.rec_cap;
    if (P.max_task) {
        for (int sl = 0; sl < P.nslot(); ++sl) for (int i = 0; i < P.nsets(); ++i) {
            BatchSlot &s = slots[sl];
            DALLOC(c, s.kA[i], u64 *, P.rec_cap * NW * 8 + 64); DALLOC(c, s.kB[i], u64 *, chunked * NW * 8 + 64);
            if (P.ext || P.combine) { DALLOC(c, s.vA[i], u64 *, P.rec_cap * 8 + 64); DALLOC(c, s.vB[i], u64 *, chunked * 8 + 64); }
        }
        int rc = alloc_sort_scratch(c, sc); if (rc) return rc;
    }
    if (P.batch) for (int sl = 0; sl < P.nslot(); ++sl) DALLOC(c, slots[sl].d_ghist, u64 *, (size_t)XCD_BATCH * MAX_PASSES * 256 * 8);
    return HSK_OK;
}
static void release_batch_buffers(hsk_ctx *c, BatchSlot *slots, SortScratch &sc)
{
    for (int sl = 0; sl < 2; ++sl) for (int i = 0; i < XCD_BATCH; ++i) { BatchSlot &s = slots[sl]; c->pool.release(s.kA[i]); c->pool.release(s.kB[i]); c->pool.release(s.vA[i]); c->pool.release(s.vB[i]); }
    free_sort_scratch(c, sc);
    c->pool.release(slots[0].d_ghist); c->pool.release(slots[1].d_ghist);
}

// one launch expands the eight tasks tk[] into the slot's buffers and counts the digits of the passes that follow
template <int NW>
static int expand_slot(hsk_ctx *c, const RankPlan<NW> &P, BatchSlot &s, const u32 *tk, u32 ntasks, const std::vector<TaskSegs> &segs, const GroupFeeder *feeder, const TaskInput &dflt, const BucketOrder &border, PhaseTimer &pt)
{
    s.tk = tk;
    s.agg = P.agg && !agg_is_off(c, NW);
    s.fext = P.fused_ext && !c->agg_off_wide;
    s.follow = s.agg || s.fext || (NW == 1 && P.fused);
    const bool will_combine = P.combine && (P.fed_combine || border.active) && s.agg;
    // (several ranks: the batch simply takes the instance path -- nobody starts a call again while peers wait)
    if (P.own_items() && !will_combine) { c->call.combine_veto = true; return retry_plan("a batch that cannot take the combining extraction"); }
    // (two-word keys: the finish orders a bin's keys by the bits below a 16-bit prefix, agg_order_many -- their pairs take bins of 16 bits)
    const int prefix_bits = will_combine ? (NW == 1 ? combine_prefix_bits(c) : AG_PREFIX_BITS) : (s.agg || s.fext) ? AG_PREFIX_BITS : 64 - HYBRID_SHIFT;
    s.prefix = prefix_bits;
    PassDesc plan[MAX_PASSES];
    int npass = batch_pass_plan<NW>(c, P.K, s.follow, will_combine ? AG_PREFIX_BITS : prefix_bits, plan);
    if (npass < 0) return plan_too_long(c, P.K, NW);
    // the pairs' two digits (most significant word): the low prefix bits, then the top 8
    if (will_combine) { npass = 2; plan[0] = PassDesc{NW - 1, 64 - prefix_bits, prefix_bits - 8}; plan[1] = PassDesc{NW - 1, 56, 8}; }
    pt.begin(PH_EXTRACT);
    HIPCHK(c, hipMemsetAsync(s.d_ghist, 0, (size_t)XCD_BATCH * MAX_PASSES * 256 * 8, c->stream));
    TaskSegs empty_segs;
    ExpandJob jobs[XCD_BATCH]; const unsigned short *s16[XCD_BATCH]; u64 *gh[XCD_BATCH];
    for (int i = 0; i < XCD_BATCH; ++i) {
        const u32 t = tk[i];
        BatchTask &b = s.bt[i];
        b = BatchTask();
        b.kA = s.kA[i]; b.kB = s.kB[i];
        if (P.ext || will_combine) { b.vA = s.vA[i]; b.vB = s.vB[i]; }      // (the payload buffers mean "records carry a payload" to everything downstream)
        gh[i] = s.d_ghist + (size_t)i * MAX_PASSES * 256; s16[i] = nullptr;
        if (t == EMPTY_TASK) { jobs[i] = ExpandJob(); jobs[i].ts = &empty_segs; continue; }
        b.n = segs[t].nkmers;
        const TaskInput in = feeder ? feeder->input(t) : dflt;
        jobs[i].ts = &segs[t]; jobs[i].sm_len = in.len; jobs[i].src = in.src; jobs[i].sm_pos = in.pos; jobs[i].sm_rid = in.rid; s16[i] = in.sub16;
        jobs[i].keys = b.kA; jobs[i].vals = b.vA; jobs[i].ghist = gh[i];
    }
    int rc;
    s.combine = false;
    if (will_combine) {
        if constexpr (NW <= 2) {
            memcpy(s.xs_plan, plan, sizeof(PassDesc) * 2);
            u64 *h_nout = staging(c)->pairs[s.index];
            if (P.fed_combine) {
                std::vector<TaskSegs> gsegs; BaseSource gsrc;
                rc = build_items_batch(c, ntasks, tk, jobs, s16, gsegs, gsrc, s.fed_items, c->stream); if (rc) return rc;
                rc = bucket_order_tasks(c, ntasks, gsegs, std::vector<u32>(tk, tk + XCD_BATCH), gsrc, FED_VT_SHIFT, s.border_fed); if (rc) return rc;
                if (!s.border_fed.active) return fail(c, HSK_ERR_UNSUPPORTED, "a task of 2^32 supermers and more");
                rc = combine_batch<NW>(c, tk, s.bt, gh, plan, s.border_fed, h_nout, s.sbatch, c->stream, P.rec_cap); if (rc) return rc;
                fed_release(c, s.fed_items); bucket_release(c, s.border_fed);      // (stream-ordered reuse: their readers are enqueued)
            } else { rc = combine_batch<NW>(c, tk, s.bt, gh, plan, border, h_nout, s.sbatch, c->stream, P.rec_cap); if (rc) return rc; }
            s.combine = s.sbatch.active;
        }
    } else if (P.xs && (s.agg || s.fext) && npass == 2 && plan[0].bits == 8 && plan[1].bits == 8) {
        if constexpr (NW <= 2) {
            for (int i = 0; i < XCD_BATCH; ++i) { jobs[i].keys = s.bt[i].kB; jobs[i].vals = s.bt[i].vB; }
            memcpy(s.xs_plan, plan, sizeof(PassDesc) * 2);
            rc = scatter_expand_batch<NW>(c, jobs, s.bt, plan, s.sbatch, c->stream); if (rc) return rc;
        }
    } else { rc = expand_batch<NW>(c, jobs, XCD_BATCH, npass, plan, c->stream, nullptr); if (rc) return rc; }
    pt.end(PH_EXTRACT);
    return HSK_OK;
}

// The pairs of every task of a combined batch are known on the device only: one wait per batch (the kernels behind it are sized from the answer).
// Every count is held to the pair stores; then the context learns from the batch (bin width, whether the detour pays).
template <int NW>
static int read_pair_counts(hsk_ctx *c, const RankPlan<NW> &P, BatchSlot &s)
{
    c->stats.host_syncs++;
    HIPCHK(c, hsk_sync(c, c->stream));
    const u64 *h_nout = staging(c)->pairs[s.index];
    // the pair stores ran over (they were sized from the estimate): once more, sized for the k-mers
    auto ran_over = [&](const char *why, unsigned info) -> int {
        if (P.fed_combine) return fail(c, HSK_ERR_INTERNAL, "pair stores overrun with several ranks");
        c->call.pair_cap_full = true; return retry_plan(why, info);
    };
    if ((u32)h_nout[XCD_BATCH] & 512u) { (void)hipMemsetAsync(c->d_err, 0, 4, c->stream); return ran_over("the pair stores ran over (sized from the estimate)", 0); }
    // Bit 512 fires only when a task's chunks exceed rec_cap / CH + 257: a task of a few hundred thousand pairs more than rec_cap fills fewer
    // spare chunks than that, and the sort below would write all its pairs into kA / vA (rec_cap records).  Every count is held to the store.
    u64 bp = 0, bk = 0, pmax = 0;
    for (int i = 0; i < XCD_BATCH; ++i) {
        BatchTask &b = s.bt[i];
        if (s.tk[i] == EMPTY_TASK || !b.n) continue;
        if (h_nout[i] > b.n) return fail(c, HSK_ERR_INTERNAL, "task %u: %llu pairs for %llu k-mers", s.tk[i], (unsigned long long)h_nout[i], (unsigned long long)b.n);
        if (h_nout[i] > P.rec_cap) return ran_over("the pair stores ran over (more pairs than records)", (unsigned)std::min<u64>(h_nout[i], 0xffffffffu));
    }
    for (int i = 0; i < XCD_BATCH; ++i) { BatchTask &b = s.bt[i]; if (s.tk[i] == EMPTY_TASK || !b.n) continue; bk += b.n; b.n = h_nout[i]; bp += h_nout[i]; pmax = std::max<u64>(pmax, h_nout[i]); }
    c->combine_prefix = std::max(c->combine_prefix_floor, combine_prefix_for(pmax));      // (the batches and calls after this one)
    c->stats.combine_pairs += bp;
    c->stats.combine_items += h_nout[COMBINE_STAT] + s.sbatch.items_host; c->stats.combine_distinct_items += h_nout[COMBINE_STAT + 1] + s.sbatch.items_host;
    if (timing_enabled()) fprintf(stderr, "[hsk] combining extraction: %llu pairs for %llu k-mers\n", (unsigned long long)bp, (unsigned long long)bk);
    // More than one pair per sixteen k-mers: this input has too few copies per k-mer for the detour to pay (measured on 10 Gbp, DESIGN.md 3.2d:
    // one pair per 25.6 k-mers 102 against 126 ms, one per 6.6 -- reads with 0.3 % errors -- 171 against 138: the tables overflow inside
    // the buckets and the parse side's extra 20 ms buy nothing; at one per sixteen a bucket's table is already 37 % full); the batches of this
    // call finish on the pairs, the next calls take the instance path
    if (bk && bp * combine_ratio(c) > bk && !c->combine_off) {
        c->leave_combine();
        // (the estimate promised fewer pairs: later estimates on this context are scaled)
        if (c->call.est.valid) c->est_bias = std::min(8.0, std::max(1.0, ((double)bp / (double)bk) / c->call.est.distinct_per_kmer));
    }
    return HSK_OK;
}

// second stage of the aggregating finish of the batch in the slot: totals -> outputs -> compaction -> result copy
template <int NW>
static int finish_slot(hsk_ctx *c, const RankPlan<NW> &P, BatchSlot &s, bool covered, ResultCopier<NW> &R, PhaseTimer &pt)
{
    if constexpr (NW <= 3) {
        TaskOut fo[XCD_BATCH];
        pt.begin(PH_COUNT);
        int rc = agg_stage2<NW>(c, s.pend, R.d_histo, R.histo_len, fo, covered);
        pt.end(PH_COUNT);
        tmark("batch stage 2 done (totals waited for, compaction enqueued)");
        if (rc) return rc;
        R.take(s.tk, fo);
        for (int i = 0; i < XCD_BATCH; ++i) if (s.tk[i] != EMPTY_TASK && fo[i].failed) {
            R.early = false;
            // a bin of pairs beyond the last table of the weighted finish: this call again, on the instance path (dispatch_pipeline)
            if (P.combine) {
                if (!combine_prefix_forced(c) && s.prefix < COMBINE_PREFIX_MAX) c->combine_prefix = c->combine_prefix_floor = COMBINE_PREFIX_MAX;      // once more with the narrowest bins
                else if (!c->combine_off) c->leave_combine();
                c->distrust_estimate((double)combine_ratio(c));
                return retry_plan("a bin beyond the weighted finish");
            }
        }
        return R.copy_batch(s.tk, XCD_BATCH);
    }
    return HSK_OK;
}

// The sorted batch of slot s is counted by the finish that was chosen when it was expanded.  `ahead`: with two batches in flight, the slot whose
// batch was sorted before this one and still waits for its aggregation totals.
template <int NW>
static int count_slot(hsk_ctx *c, const RankPlan<NW> &P, BatchSlot &s, BatchSlot *ahead, const std::vector<u64> &pay_before, ResultCopier<NW> &R, PhaseTimer &pt)
{
    BatchTask *bt = s.bt;
    if (s.agg) {
        if constexpr (NW <= 3) {
            // the previous batch first: this batch's expand and scatter pass are queued behind its aggregation, so the
            // wait for its totals does not idle the GPU, and its compaction (and result copy) starts one kernel earlier
            // (stage 2 of the previous batch BEFORE this batch's stage 1 would start its result copy one kernel earlier, but a
            // device-to-host copy running beside agg_finish_kernel stretches a batch from 19 to 32 ms: measured in round 2, gone)
            pt.begin(PH_COUNT);
            int rc = agg_stage1<NW>(c, bt, P.K, s.prefix, s.index, s.pend, s.combine);
            pt.end(PH_COUNT);
            if (rc) return rc;
            if (ahead && ahead->pend.active) { rc = finish_slot<NW>(c, P, *ahead, true, R, pt); if (rc) return rc; }
            if (!P.lag) { rc = finish_slot<NW>(c, P, s, false, R, pt); if (rc) return rc; }
        }
        return HSK_OK;
    }
    pt.begin(PH_COUNT);
    TaskOut fo[XCD_BATCH];
    if (s.fext) {
        if constexpr (NW <= 3) {
            u64 pb[XCD_BATCH];
            for (int i = 0; i < XCD_BATCH; ++i) pb[i] = s.tk[i] != EMPTY_TASK ? pay_before[s.tk[i]] : 0;
            int rc = agg_ext_finish_batch_device<NW>(c, bt, P.K, pb, R.d_histo, R.histo_len, fo); if (rc) return rc;
            R.take(s.tk, fo);
        }
    } else if (P.fused && NW == 1 && !P.ext) {
        if constexpr (NW == 1) {
            int rc = finish_batch_device<1>(c, bt, P.K, P.max_task, R.d_histo, R.histo_len, fo); if (rc) return rc;
            R.take(s.tk, fo);
        }
    } else {
        for (int i = 0; i < XCD_BATCH; ++i) {
            const u32 t = s.tk[i];
            if (t == EMPTY_TASK) continue;
            int rc = count_task_device<NW>(c, bt[i].out_k, bt[i].out_v, bt[i].n, pay_before[t], R.d_histo, R.histo_len, R.touts[t]); if (rc) return rc;
        }
    }
    pt.end(PH_COUNT);
    return HSK_OK;
}

// Everything after the supermers of the owned tasks are in place: per task expand, sort, count; then the
// result of this rank.  `segs[t]` lists where the supermers of task t live (x_len / x_src / x_pos / x_rid).
template <int NW>
static int process_rank(hsk_ctx *c, u32 ntasks, const std::vector<int32_t> &owner, int rank, std::vector<TaskSegs> &segs, const u8 *x_len, const BaseSource &x_src, const u32 *x_pos,
                        const int32_t *x_rid, hsk_result *out, ResultPriv *rp, PhaseTimer &pt, bool pt_total_open, GroupFeeder *feeder = nullptr, const ProcExtra *ex = nullptr)
{
    u64 max_task = 0, total_kmers = 0;
    for (u32 t = 0; t < ntasks; ++t) { finalize_segs(segs[t]); max_task = std::max(max_task, segs[t].nkmers); total_kmers += segs[t].nkmers; }
    out->total_kmers = total_kmers;
    const bool item_mode = x_src.item != nullptr;
    const u32 vt_shift = ex ? ex->vt_shift : 0;
    first_table_from_estimate(c, NW, max_task, vt_shift || item_mode);
    const u32 histo_len = (u32)std::min<int64_t>((int64_t)c->cfg.upper_freq + 1, 65536);    // (U <= 65535 except in the unfiltered pre-aggregation)
    u64 *d_histo; DALLOC(c, d_histo, u64 *, (size_t)histo_len * 8);
    HIPCHK(c, hipMemsetAsync(d_histo, 0, (size_t)histo_len * 8, c->stream));

    // ---- the plan ---------------------------------------------------------------------------------------
    const RankPlan<NW> P = plan_rank<NW>(c, ntasks, owner, rank, segs, max_task, feeder, item_mode, ex);
    if (P.retry) { c->call.combine_veto = true; return P.retry; }
    const std::vector<u32> &mine = P.mine;
    const bool ext = P.ext;
    ResultCopier<NW> R(c, rp, segs, ntasks, total_kmers, P.early, P.compact_mode);
    R.d_histo = d_histo; R.histo_len = histo_len;
    std::vector<TaskOut> &touts = R.touts;

    // ---- bucket order (one GPU) -------------------------------------------------------------------------
    // The bucket order of ALL owned tasks comes before the sort buffers are allocated: once its scatter is enqueued nobody reads the item store
    // again, and its 21 GB (10 Gbp) go back to the pool: the call's peak of live device memory 68 -> 46 GB (HSK_TIMING prints the pool's state;
    // what the pool has MAPPED stays at 89 GB -- it hands a cached block only to requests of nearly its size -- and that, mapped for the first
    // time, is what a process's first call pays for).
    BucketOrder border;
    if (P.own_items()) {
        pt.begin(PH_EXTRACT);
        int rc = bucket_order_tasks(c, ntasks, segs, mine, x_src, vt_shift, border); if (rc) return rc;
        pt.end(PH_EXTRACT);
        if (!border.active) { c->call.combine_veto = true; return retry_plan("no bucket order"); }
        if (ex && ex->items_store) {                      // (stream-ordered reuse: every later user of these blocks is enqueued behind the scatter)
            SupermerStore &is = *ex->items_store;
            c->pool.release(is.sm_item); is.sm_item = nullptr; c->pool.release(is.sm_sub); is.sm_sub = nullptr;
            c->pool.release(is.d_bitems); is.d_bitems = nullptr; is.n_bitems = 0; for (void *&q : is.bin_aux) { c->pool.release(q); q = nullptr; }
        }
    }

    // ---- buffers ----------------------------------------------------------------------------------------
    BatchSlot slots[2]; slots[1].index = 1;
    SortScratch sc;
    {
        int arc = alloc_batch_buffers<NW>(c, P, slots, sc);
        if (!arc && feeder && test_fail(c, "sortbuf")) arc = fail(c, HSK_ERR_OOM, "sort buffers (injected)");
        if (feeder && !feeder->st_all && c->comm.active()) {
            // the largest allocations of the call are behind us: make sure EVERY rank got them before the first task group
            // travels (a rank that gave up here alone would leave its peers blocked in their first send / receive)
            std::vector<u64> none;
            const int st_ = c->comm.allreduce_with_status(none, RCCL_MAX, arc != 0, c->stream, c->pool);
            if (st_) return left_together(c, st_, "status", arc, "another rank ran out of memory before the supermer exchange");
            feeder->live = true;                          // from here on a failing rank drains the exchange and the ranks agree at the end (run_pipeline)
        } else if (arc) return arc;
    }
    // payload offsets are global over the owned tasks in ascending id: prefix of k-mer counts
    std::vector<u64> pay_before(ntasks, 0);
    { u64 acc = 0; for (u32 t : mine) { if (t == EMPTY_TASK) continue; pay_before[t] = acc; if (ext) acc += segs[t].nkmers; } }
    TaskInput dflt; dflt.len = x_len; dflt.src = x_src; dflt.pos = x_pos; dflt.rid = x_rid;

    // ---- batches ----------------------------------------------------------------------------------------
    size_t pos = 0;
    const size_t nbatch = P.batch ? mine.size() / XCD_BATCH : 0;
    for (size_t b = 0; b < nbatch; ++b, pos += XCD_BATCH) {
        BatchSlot &s = slots[P.lag ? (b & 1) : 0];
        const u32 *tk = &mine[pos];
        if (b == 1 && feeder && test_fail(c, "late")) return fail(c, HSK_ERR_OOM, "second batch (injected)");
        // (only after hsk_ctx::agg_off ended the aggregation in the middle of the call: the slot's buffers are about to be reused)
        if (s.pend.active) { int rc = finish_slot<NW>(c, P, s, false, R, pt); if (rc) return rc; }
        if (feeder) {                                   // exposed (not overlapped) part of the exchange
            pt.begin(PH_EXCH);
            for (int i = 0; i < XCD_BATCH; ++i) { if (tk[i] == EMPTY_TASK) continue; int rc = feeder->need(feeder->group_of[tk[i]]); if (rc) return rc; }
            pt.end(PH_EXCH);
        }
        { int rc = expand_slot<NW>(c, P, s, tk, ntasks, segs, feeder, dflt, border, pt); if (rc) return rc; }
        if (feeder) feeder->release_below((pos + XCD_BATCH < mine.size() && mine[pos + XCD_BATCH] != EMPTY_TASK) ? feeder->group_of[mine[pos + XCD_BATCH]] : feeder->ngroups);
        if (s.combine) { int rc = read_pair_counts<NW>(c, P, s); if (rc) return rc; }
        pt.begin(PH_SORT);
        if (s.sbatch.active) { if constexpr (NW <= 2) { int rc = sort_batch_prescattered<NW>(c, s.bt, s.xs_plan, s.d_ghist, s.sbatch); if (rc) return rc; } }
        else { int rc = sort_batch_device<NW>(c, s.bt, P.K, s.follow, s.prefix, s.d_ghist); if (rc) return rc; }
        pt.end(PH_SORT);
        { int rc = count_slot<NW>(c, P, s, (P.lag && b > 0) ? &slots[s.index ^ 1] : nullptr, pay_before, R, pt); if (rc) return rc; }
    }
    if (P.lag && nbatch > 0) for (BatchSlot &s : slots) if (s.pend.active) { int rc = finish_slot<NW>(c, P, s, false, R, pt); if (rc) return rc; }

    // ---- single tasks (slot 0's first buffers) ----------------------------------------------------------
    for (; pos < mine.size(); ++pos) {
        const u32 t = mine[pos];
        const u64 n = segs[t].nkmers;
        u64 *kA = slots[0].kA[0], *kB = slots[0].kB[0], *vA = ext ? slots[0].vA[0] : nullptr, *vB = ext ? slots[0].vB[0] : nullptr;
        int rc;
        if (feeder) { pt.begin(PH_EXCH); rc = feeder->need(feeder->group_of[t]); pt.end(PH_EXCH); if (rc) return rc; }
        pt.begin(PH_EXTRACT);
        const TaskInput in = feeder ? feeder->input(t) : dflt;
        rc = expand_task<NW>(c, segs[t], in.len, in.src, in.pos, in.rid, kA, vA); if (rc) return rc;
        pt.end(PH_EXTRACT);
        if (feeder) feeder->release_below(pos + 1 < mine.size() ? feeder->group_of[mine[pos + 1]] : feeder->ngroups);
        pt.begin(PH_SORT);
        u64 *sk, *sv;
        rc = sort_task_device<NW>(c, kA, kB, vA, vB, n, P.K, sc, &sk, &sv); if (rc) return rc;
        pt.end(PH_SORT);
        pt.begin(PH_COUNT);
        rc = count_task_device<NW>(c, sk, sv, n, pay_before[t], d_histo, histo_len, touts[t]); if (rc) return rc;
        pt.end(PH_COUNT);
    }

    // ---- heavy lists: the heavy-hitter tasks this rank owns arrive as k-mer lists: order, sum, filter ----
    if (ex && ex->heavy_in) {
        pt.begin(PH_COUNT);
        for (const HeavyIn &hv : *ex->heavy_in) { int rc = heavy_merge_task<NW>(c, hv.d_entries, hv.n, d_histo, histo_len, touts[hv.task]); if (rc) return rc; }
        pt.end(PH_COUNT);
    }
    u64 n_total = 0, pay_total = 0;
    for (u32 t = 0; t < ntasks; ++t) { touts[t].pay_base = pay_before[t]; n_total += touts[t].n; pay_total += touts[t].npay; }      // (a task of another rank: all zero)
    if (feeder) { int rc = feeder->finish(); if (rc) return rc; }
    release_batch_buffers(c, slots, sc);
    if (P.combine && !c->combine_off) c->combine_good_calls++;
    bucket_release(c, border);

    // ---- result ----------------------------------------------------------------------------------------
    pt.begin(PH_D2H);
    { int rc = R.finish_list(out, n_total, pay_total); if (rc) return rc; }
    pt.end(PH_D2H);
    if (pt_total_open) pt.end(PH_TOTAL);
    tmark("result copies enqueued");
    { int rc = R.drain(); if (rc) return rc; }
    if (const u32 w = staging(c)->err) return device_check_failed(c, w);
    if (!ext && total_kmers && !c->forbid_long_way) c->entries_per_kmer = (double)n_total / (double)total_kmers;
    if (ext && !R.keep) out->payload_off[n_total] = pay_total;
    if (R.keep) { rp->dev_tasks = touts; out->entries_dev = nullptr; }
    else for (auto &to : touts) free_task_out(c, to);
    c->pool.release(d_histo);
    if (pt_total_open) out->ms_total = pt.collect(PH_TOTAL);
    out->ms_parse = pt.collect(PH_PARSE); out->ms_exchange = pt.collect(PH_EXCH);
    out->ms_extract = pt.collect(PH_EXTRACT); out->ms_sort = pt.collect(PH_SORT); out->ms_count = pt.collect(PH_COUNT);
    out->ms_d2h = pt.collect(PH_D2H);
    return HSK_OK;
}

// ---- what run_pipeline and run_loopback both say around process_rank ---------------------------------------------
// May a call over `nranks` ranks with about `bytes` of packed reads per rank take the combining extraction?  The part both drivers share; what only
// one of them knows (the attempt's history, the task count and bucket sizes of one GPU) stays there.
// The combining extraction pays from a few hundred million k-mers on (a bucket order of the supermers comes first); tuning "combine_min_bytes" moves
// the limit (tests: 0).  This call's own estimate of the input (estimate_plan) decides where there is one; the context's memory of earlier calls
// (combine_off, agg_off) where there is none.
// (two-word keys: 40 <= K <= 55 -- the prefix bits sit in the most significant word, an item of 64 bases holds six k-mers and more: shorter
//  items would be more records per tile than the parse keeps, for 16 bytes that stand for very few k-mers)
// Several ranks (round 4): the supermers travel as byte runs with 16 of their minimizer bits, the OWNER of a task builds the items (hsk_combine.h,
// 1b); needs the grouped exchange and the byte-store placement, and every rank's consent (run_pipeline)
template <int NW>
static bool combine_allowed(const hsk_ctx *c, int nranks, u64 bytes)
{
    const int K = c->cfg.kmer_size;
    const bool pays = c->call.est.valid ? c->call.est.distinct_per_kmer * c->est_bias * (double)combine_ratio(c) <= 1.0 : !c->combine_off;
    return (NW == 1 || (NW == 2 && K >= 40 && K <= 55)) && !c->cfg.extension && pays && !agg_is_off(c, NW) && combine_enabled(c) && c->tune.parse_fast != 0 &&
           c->cfg.minimizer_size <= SCAN_MAX_M && bytes >= (u64)c->tune.combine_min_bytes && c->xcd_batch_ok &&
           (nranks == 1 || (c->tune.overlap != 0 && place_bytes_enabled(c, true)));
}
static ResultPriv *begin_result(hsk_result *out, int nw) { memset(out, 0, sizeof *out); ResultPriv *rp = new ResultPriv(); out->priv = rp; out->nw = nw; return rp; }
// virtual ranks: a rank's parse was timed on its own, its total is the sum of its phases
static void sum_phases(hsk_result &o, double ms_parse) { o.ms_parse = ms_parse; o.ms_total = o.ms_parse + o.ms_exchange + o.ms_extract + o.ms_sort + o.ms_count + o.ms_d2h; }

// ---- steps both drivers take (run_pipeline: one GPU or one rank over RCCL; run_loopback: virtual ranks) ------------------------------
struct CallInput { const u8 *d_packed; u64 packed_bytes; const u64 *d_roff; const u32 *d_rlen; u64 nreads; int64_t rid_base; };      // one rank's reads, in HBM
static std::vector<u32> identity_order(u32 n) { std::vector<u32> o(n); for (u32 i = 0; i < n; ++i) o[i] = i; return o; }

// Where the supermers of every task (`only`: of these alone) live in a store that is read in place: one segment per task from the store's totals and bases.
// vt_shift: the store's tasks are virtual ones, 2^vt_shift per task; a task's segments are those of its virtual tasks (which one: ExpSeg::byte_off, unused in item mode).
static void segs_from_store(const SupermerStore &st, u32 ntasks, u32 vt_shift, const std::vector<u8> *only, std::vector<TaskSegs> &segs)
{
    for (u32 v = 0; v < (ntasks << vt_shift); ++v) {
        const u32 t = v >> vt_shift;
        if (only && !(*only)[t]) continue;
        segs[t].nkmers += st.task_tot[3 * v + 2];
        if (st.task_tot[3 * v] == 0) continue;
        ExpSeg sg; sg.sup_off = st.task_base[3 * v]; sg.n_sup = st.task_tot[3 * v]; sg.kmer_off = 0; sg.tile_start = 0;
        sg.byte_off = vt_shift ? v & ((1u << vt_shift) - 1u) : st.task_base[3 * v + 1];
        segs[t].segs.push_back(sg);
    }
}

// ---- heavy-hitter tasks (a8): the sending side ----------------------------------------------------------------
// HeavyHitterClassifier (reference src/kmerops.cpp:1157-1199) on the GLOBAL k-mer counts, for every key width (the
// reference's ScatteredKmerList is generic over TKmer, kmerops.cpp:363-401); forced plain with EXTENSION or
// PLAIN_CLASSIFIER (kmerops.cpp:109-113).
static bool heavy_enabled(hsk_ctx *c, int nranks) { return nranks > 1 && c->cfg.extension == 0 && (c->cfg.flags & HSK_FLAG_PLAIN_CLASSIFIER) == 0; }
struct HeavySet {
    std::vector<u8> is_heavy; bool any = false;
    std::vector<u64> kmers;                              // k-mer instances of a heavy task over all ranks (they travel as lists: its owner counts them into total_kmers)
    explicit HeavySet(u32 ntasks) : is_heavy(ntasks, 0), kmers(ntasks, 0) {}
    void classify(const hsk_ctx *c, const std::vector<u64> &kg)      // kg[t]: the k-mer instances of task t over all ranks
    {
        std::vector<int32_t> types(kg.size(), 0);
        plan_classify(kg.data(), (int)kg.size(), c->cfg.unbalanced_ratio, types.data());
        for (size_t t = 0; t < kg.size(); ++t) if (types[t] == 1) { is_heavy[t] = 1; any = true; kmers[t] = kg[t]; }
    }
    // After the pre-aggregation.  bad[t]: some rank could not aggregate task t -- it travels as supermers after all, on every rank.  The others stay
    // heavy, and what they weigh in the dispatch (bytes[t]) is the size of their lists.  lists[0 .. nlists): [task] lists of the ranks this process holds.
    void settle(hsk_ctx *c, const std::vector<u64> &bad, std::vector<TaskOut> *lists, int nlists, u64 entry_bytes, std::vector<u64> &bytes)
    {
        any = false;
        for (size_t t = 0; t < is_heavy.size(); ++t) {
            if (!is_heavy[t]) continue;
            if (bad[t]) { is_heavy[t] = 0; for (int r = 0; r < nlists; ++r) free_task_out(c, lists[r][t]); continue; }
            any = true; c->stats.heavy_tasks++; bytes[t] = 0;
            for (int r = 0; r < nlists; ++r) bytes[t] += lists[r][t].n * entry_bytes;                   // ScatteredKmerList::get_size_bytes
        }
    }
};
// An owner's buffer of a heavy task: the ranks' lists in rank order.  n[p * stride]: entries of rank p's list; -> where it begins (p == nranks: the total)
static u64 heavy_list_off(const u64 *n, size_t stride, int p) { u64 o = 0; for (int q = 0; q < p; ++q) o += n[(size_t)q * stride]; return o; }

// the k-mers of the input that did not arrive as supermers: the instances the scan left out, and the heavy tasks this rank owns (they arrived as lists)
static void add_unsent_kmers(hsk_ctx *c, hsk_result *out, u64 dropped, const HeavySet &hv, const std::vector<int32_t> &owner, int rank)
{
    out->total_kmers += dropped; c->stats.dropped_kmers += (int64_t)dropped;
    for (size_t t = 0; t < hv.is_heavy.size(); ++t) if (hv.is_heavy[t] && owner[t] == rank) out->total_kmers += hv.kmers[t];
}

// the dispatcher on the global task sizes; `order`: the storage order of a rank's supermers, tasks grouped by owner
static int dispatch_owners(hsk_ctx *c, const std::vector<u64> &bytes, int nranks, std::vector<int32_t> &owner, std::vector<u32> &order)
{
    if (plan_dispatch(bytes.data(), (int)bytes.size(), nranks, c->cfg.plain_dispatcher != 0, c->cfg.dispatch_upper_coe, c->cfg.dispatch_step, owner.data()))
        return fail(c, HSK_ERR_DISPATCH, "%s", hsk_strerror(HSK_ERR_DISPATCH));      // (same input on every rank: all of them fail here; a failed call's blocks go back with its scope: ApiCall)
    std::stable_sort(order.begin(), order.end(), [&](u32 x, u32 y) { return owner[x] < owner[y]; });
    return HSK_OK;
}

// Every rank turns its OWN supermers of the heavy tasks into unfiltered {k-mer, count} lists (ScatteredKmerList,
// kmerops.cpp:363-398): only the heavy tasks are placed, then the ordinary expand / sort / aggregate kernels run with
// L = 1, U = max.  lists[t] stays in HBM; bad[t] is set where the aggregating finish could not handle the task (it is then
// sent as supermers like any other task -- on every rank, the flags are combined by the caller).
template <int NW>
static int heavy_preaggregate(hsk_ctx *c, ParseJob &job, const u8 *d_packed, u64 packed_bytes, const std::vector<u8> &is_heavy, std::vector<TaskOut> &lists, std::vector<u64> &bad)
{
    const u32 ntasks = job.ntasks;
    lists.assign(ntasks, TaskOut());
    std::vector<u32> order; std::vector<u8> skip(ntasks, 0);
    for (u32 t = 0; t < ntasks; ++t) if (is_heavy[t]) order.push_back(t);
    for (u32 t = 0; t < ntasks; ++t) if (!is_heavy[t]) { order.push_back(t); skip[t] = 1; }
    SupermerStore sth;
    int rc = parse_place(c, job, order, sth, &skip); if (rc) return rc;
    std::vector<TaskSegs> segs(ntasks);
    std::vector<int32_t> own(ntasks, -1); for (u32 t = 0; t < ntasks; ++t) if (is_heavy[t]) own[t] = 0;
    segs_from_store(sth, ntasks, 0, &is_heavy, segs);
    const hsk_config keep = c->cfg;
    c->cfg.lower_freq = 1; c->cfg.upper_freq = INT32_MAX; c->cfg.flags |= HSK_FLAG_KEEP_DEVICE;
    c->forbid_long_way = true;
    hsk_result tmp; ResultPriv *rp = begin_result(&tmp, NW);
    PhaseTimer pt(c);
    ProcExtra ex; ex.force_batch = true;
    rc = process_rank<NW>(c, ntasks, own, 0, segs, sth.sm_len, source_from_store(sth, d_packed, packed_bytes), nullptr, nullptr, &tmp, rp, pt, false, nullptr, &ex);
    c->cfg = keep; c->forbid_long_way = false;
    if (rc == HSK_OK) {
        for (u32 t = 0; t < ntasks; ++t) if (is_heavy[t] && t < rp->dev_tasks.size()) { lists[t] = rp->dev_tasks[t]; if (lists[t].failed) bad[t] = 1; }
        rp->dev_tasks.clear();                              // the lists are ours now
    }
    hsk_result_free(c, &tmp);
    free_store(c, sth);
    return rc;
}

// ---- the steps of run_pipeline ------------------------------------------------------------------------------------------------------
// The plan of the call, in hsk_ctx::call (read by the parse and by process_rank): the context's periodic second looks, the combining extraction or
// not, the task count, the virtual-task shift, the certain drops.  Several ranks agree on all of it in one all-reduce.
template <int NW>
static int plan_call(hsk_ctx *c, int nranks, u64 packed_bytes, u32 &ntasks)
{
    if ((c->agg_off || c->agg_off_wide) && ++c->agg_off_calls >= 8) { c->agg_off = c->agg_off_wide = false; c->agg_off_calls = 0; }      // (another look every eighth call: the input may have changed)
    if (c->combine_off && ++c->combine_off_calls >= c->combine_off_period) { c->combine_off = false; c->combine_off_calls = 0; c->combine_prefix_floor = 0; }      // (another look: the bin width starts from the default again as well)
    if (c->call.est.valid && c->agg_off && c->call.plan_attempt == 0) { c->agg_off = false; c->agg_off_calls = 0; }      // (process_rank decides again, from the estimate and the task sizes)
    c->call.combine_now = combine_allowed<NW>(c, nranks, packed_bytes) && !c->call.combine_left_now && !c->call.combine_veto && c->call.plan_attempt < 2;
    c->call.combine_veto = false;
    // the combining extraction wants buckets of ~12 k k-mers: the parse itself splits every task by the top minimizer bits (virtual
    // tasks, up to 16 per task and HSK_MAX_TASKS in all: ParseArgs::vt_shift), the bucket order does the rest (hsk_combine.h)
    c->call.vt_shift = 0;
    ntasks = c->cfg.ntasks ? (u32)c->cfg.ntasks : auto_ntasks(c, packed_bytes, nranks);
    if (c->comm.active()) {
        // every rank must use the same task count (the maximum of the local proposals) and the same plan (the combining extraction only if
        // every rank's own estimate says its input pays for it: the minimizer bits either travel from all ranks or from none)
        // ... and the certain drops: a rank whose own sample holds more than U copies of a homopolymer k-mer is right for all ranks (OR of the masks)
        u64 v[4] = {c->cfg.ntasks ? 0ULL : (u64)ntasks, c->call.combine_now ? 0ULL : 1ULL, (u64)(c->call.drop_mask_now & 1u), (u64)((c->call.drop_mask_now >> 1) & 1u)};
        int rc = c->comm.allreduce_max_u64(v, 4, c->stream, c->pool); if (rc) return fail(c, HSK_ERR_COMM, "allreduce(ntasks, plan) failed: %d", rc);
        if (!c->cfg.ntasks) ntasks = (u32)v[0];
        if (v[1]) c->call.combine_now = false;
        c->call.drop_mask_now = (v[2] ? 1u : 0u) | (v[3] ? 2u : 0u);
    }
    // (at most 768 virtual tasks: the item placement's LDS holds 16 bytes for each beside its 16384 records; more real tasks than that: the instance path)
    if (ntasks > 768 && nranks == 1) c->call.combine_now = false;
    if (c->call.combine_now && nranks == 1) { u32 sh = 0; while (sh < 4 && ((u64)ntasks << (sh + 1)) <= 768) ++sh; c->call.vt_shift = sh; }
    if (c->call.combine_now && c->call.est.valid && nranks == 1) {
        // a task has at most 2^14 buckets (CS_MAX_LOG2NB; 2^(10 + virtual-task bits)): few, large tasks make buckets whose distinct k-mers overflow the
        // 2048-slot tables again and again (partial pairs: the detour stops paying) -- predicted from the estimate instead of found out by a batch
        const u32 lg = (u32)std::min<int>(CS_MAX_LOG2NB, CS_MAX_LOCAL + (int)c->call.vt_shift);
        const double per_bucket = (double)packed_bytes * 4.0 / (double)ntasks / (double)(1u << lg);
        if (per_bucket > (double)combine_bucket_kmers(c) && c->call.est.distinct_per_kmer * per_bucket > 1400.0) { c->call.combine_now = false; c->call.vt_shift = 0; }
    }
    c->call.item_mode_now = c->call.combine_now && nranks == 1;      // one GPU: the store holds items (several ranks: byte runs + minimizer bits, the owners build the items)
    return HSK_OK;
}

// One GPU, reads arriving from pinned host memory, no payload: ingest, scan and placement as one pipeline over slabs.  done = false: not this
// call's way, or the pipeline fell back with the packed reads in HBM -- the two-step parse takes it from there.
static int parse_pipelined(hsk_ctx *c, const CallInput &in, int nranks, u32 ntasks, SupermerStore &st, std::vector<TaskSegs> &segs, bool &done)
{
    const u32 vts = c->call.vt_shift, nvt = ntasks << vts;       // what the parse calls tasks
    done = false;
    if (nranks != 1 || c->cfg.extension || !c->call.h2d_src || c->tune.ingest_pipeline == 0 || c->tune.parse_fast == 0 || c->cfg.minimizer_size > SCAN_MAX_M) return HSK_OK;
    const u8 *src = c->call.h2d_src; c->call.h2d_src = nullptr;
    std::vector<TaskSegs> segs_v;
    const int prc = parse_ingest_pipelined(c, src, in.d_packed, in.packed_bytes, in.d_roff, in.d_rlen, in.nreads, in.rid_base, nvt, st, vts ? segs_v : segs);
    if (prc == HSK_OK) {
        done = true;
        for (u32 v = 0; v < (u32)segs_v.size(); ++v) {          // a task's segments: those of its virtual tasks, as in segs_from_store (the ingest hands back one per slab)
            TaskSegs &ts = segs[v >> vts];
            for (ExpSeg sg : segs_v[v].segs) { sg.byte_off = v & ((1u << vts) - 1u); sg.kmer_off = 0; ts.segs.push_back(sg); }
            ts.nkmers += segs_v[v].nkmers;
        }
    }
    else if (prc == PARSE_FALLBACK && vts) { c->call.vt_shift = 0; c->call.combine_veto = true; return retry_plan("the pipelined ingest fell back"); }      // (the fallback parse knows no virtual tasks: the call again, without them)
    else if (prc != PARSE_FALLBACK) { c->call.vt_shift = 0; return prc; }
    else c->stats.parse_fallbacks++;
    return HSK_OK;
}

// Several ranks, between parse_count and parse_place: the ranks agree on the tasks' global sizes, on which tasks are heavy (a8: classified on the
// global k-mer counts, every rank pre-aggregates its own share into `hlists`), and from the sizes on owners and storage order.  A rank that fails
// must not return alone (its peers would wait for it in the next collective for ever).  Every all-reduce here carries the ranks' status as one more
// element; a failed rank (parse_rc: its parse_count) keeps taking part, with zeros, until the next one, then all ranks return together.
template <int NW>
static int agree_on_tasks(hsk_ctx *c, ParseJob &job, const CallInput &in, int nranks, u32 ntasks, int parse_rc, HeavySet &hv, std::vector<TaskOut> &hlists, std::vector<int32_t> &owner, std::vector<u32> &order)
{
    Comm &cm = c->comm;
    int local_rc = parse_rc;                             // first local failure since the last collective
    auto together = [&](int st_, const char *what) { return left_together(c, st_, what, local_rc, "another rank failed before the all-reduce of %s"); };
    std::vector<u64> bytes(ntasks, 0); int rc;
    if (!local_rc) for (u32 t = 0; t < ntasks; ++t) bytes[t] = job.task_tot[3 * t + 1] + job.task_tot[3 * t] * (c->cfg.extension ? 9 : 1);
    if (heavy_enabled(c, nranks)) {
        std::vector<u64> kg(ntasks, 0);
        if (!local_rc) for (u32 t = 0; t < ntasks; ++t) kg[t] = job.task_tot[3 * t + 2];
        rc = together(cm.allreduce_with_status(kg, RCCL_SUM, local_rc != 0, c->stream, c->pool), "task k-mers"); if (rc) return rc;
        hv.classify(c, kg);
    }
    if (hv.any) {
        std::vector<u64> bad(ntasks, 0);
        local_rc = heavy_preaggregate<NW>(c, job, in.d_packed, in.packed_bytes, hv.is_heavy, hlists, bad);
        if (!local_rc && test_fail(c, "heavy")) { local_rc = fail(c, HSK_ERR_OOM, "heavy-hitter lists (injected)"); bad.assign(ntasks, 0); }
        rc = together(cm.allreduce_with_status(bad, RCCL_MAX, local_rc != 0, c->stream, c->pool), "heavy flags"); if (rc) return rc;     // a task one rank could not aggregate travels as supermers everywhere
        hv.settle(c, bad, &hlists, 1, (u64)(NW + 1) * 8, bytes);
    }
    rc = together(cm.allreduce_with_status(bytes, RCCL_SUM, local_rc != 0, c->stream, c->pool), "task sizes"); if (rc) return rc;
    return dispatch_owners(c, bytes, nranks, owner, order);
}

// The reads are hashed once (parse_count); several ranks: the dispatcher needs the global task sizes before the storage order (tasks grouped
// by owner rank) is known (agree_on_tasks), then parse_place lays the supermers out.
template <int NW>
static int parse_two_steps(hsk_ctx *c, const CallInput &in, int nranks, u32 ntasks, HeavySet &hv, std::vector<TaskOut> &hlists, std::vector<int32_t> &owner, std::vector<u32> &order, SupermerStore &st, int &place_rc)
{
    const u32 vts = c->call.vt_shift, nvt = ntasks << vts;
    ParseJob job;
    struct Release { hsk_ctx *c; ParseJob &j; ~Release() { parse_release(c, j); } } release{c, job};      // (on every way out)
    int rc = parse_count(c, in.d_packed, in.packed_bytes, in.d_roff, in.d_rlen, in.nreads, in.rid_base, nvt, job);
    if (!rc && nranks > 1 && test_fail(c, "parse")) rc = fail(c, HSK_ERR_OOM, "parse tables (injected)");
    if (rc && nranks == 1) { c->call.vt_shift = 0; return rc; }
    if (vts && !job.scan.d_tile_sub && !job.scan.bins.items && !job.empty) { c->call.vt_shift = 0; c->call.combine_veto = true; return retry_plan("the parse left its fast path: no items"); }
    if (nranks > 1) { rc = agree_on_tasks<NW>(c, job, in, nranks, ntasks, rc, hv, hlists, owner, order); if (rc) return rc; }
    if (vts) rc = parse_place(c, job, identity_order(nvt), st, nullptr, false);
    else rc = parse_place(c, job, order, st, hv.any ? &hv.is_heavy : nullptr, nranks > 1);
    if (!rc && nranks > 1 && test_fail(c, "place")) rc = fail(c, HSK_ERR_OOM, "supermer store (injected)");
    if (rc && nranks == 1) return rc;
    place_rc = rc;                                           // several ranks: carried into the size-matrix all-reduce (exchange_or_feed)
    return HSK_OK;
}

// Several ranks, after the placement: the byte runs are packed (src: the store's bases), then either the feeder is planned from the size matrix --
// fed: the task groups travel while process_rank counts -- or, tuning "overlap=0", everything travels now: `xb` holds the owned tasks' supermers and
// the store is freed.  Afterwards segs[t] lists where the supermers of owned task t live.
static int exchange_or_feed(hsk_ctx *c, int place_rc, u32 ntasks, const std::vector<int32_t> &owner, const std::vector<u32> &order, SupermerStore &st, const BaseSource &src, GroupFeeder &feeder, bool &fed, ExchangeBuffers &xb, std::vector<TaskSegs> &segs)
{
    const int nranks = c->comm.nranks, rank = c->comm.rank;
    const int local_rc = place_rc ? place_rc : pack_store_bytes(c, st, src, c->tune.overlap == 0);
    if (c->tune.overlap == 0) {
        const int rc = exchange_supermers(c->comm, c->stream, c->pool, c->cfg.extension != 0, c->cfg.kmer_size, ntasks, owner, order, st.task_tot, st.task_base, st.sm_len, st.sm_bytes, st.sm_pos, st.sm_rid, xb, segs, local_rc != 0);
        if (rc > 0 && local_rc) return local_rc;
        if (rc) return fail(c, HSK_ERR_COMM, "supermer exchange failed: %d (%s)", rc, c->comm.last_error.c_str());
        free_store(c, st);
        return HSK_OK;
    }
    // size matrix: every rank contributes its row, the sum is the full matrix (+ the ranks' status: a rank whose placement or byte packing failed leaves together with its peers)
    std::vector<u64> M((size_t)nranks * ntasks * 3, 0);
    if (!local_rc) std::copy_n(st.task_tot.begin(), (size_t)ntasks * 3, M.begin() + (size_t)rank * ntasks * 3);
    M.push_back((!local_rc && (st.sm_sub16 != nullptr || st.tot_sup == 0)) ? 1 : 0);      // this rank's supermers carry their minimizer bits (or it has none to send)
    const int st_ = c->comm.allreduce_with_status(M, RCCL_SUM, local_rc != 0, c->stream, c->pool);
    if (st_) return left_together(c, st_, "size matrix", local_rc, "another rank failed before the supermer exchange");
    const bool all_sub = M.back() == (u64)nranks && c->call.combine_now; M.pop_back();
    const int rc = feeder.plan(c, nranks, rank, ntasks, owner, order, M, st.task_base, segs); if (rc) return rc;
    feeder.st = &st; feeder.lazy_pack = true; feeder.with_sub = all_sub; fed = true;
    return HSK_OK;
}

// The k-mer lists of the heavy tasks go to their owners: sizes by all-reduce, one grouped send/recv, the own share by device copy.  hin: the
// heavy tasks this rank owns, the lists of all ranks; hlists (this rank's lists) are freed.
template <int NW>
static int exchange_heavy_lists(hsk_ctx *c, const HeavySet &hv, const std::vector<int32_t> &owner, std::vector<TaskOut> &hlists, std::vector<HeavyIn> &hin)
{
    Comm &cm = c->comm;
    const int nranks = cm.nranks, rank = cm.rank;
    std::vector<u32> hv_tasks; for (u32 t = 0; t < (u32)hv.is_heavy.size(); ++t) if (hv.is_heavy[t]) hv_tasks.push_back(t);
    const size_t nh = hv_tasks.size();
    std::vector<u64> Hn((size_t)nranks * nh, 0);         // [rank][heavy task] entries of the rank's list
    for (size_t i = 0; i < nh; ++i) Hn[(size_t)rank * nh + i] = hlists[hv_tasks[i]].n;
    int rc = cm.allreduce_sum_u64(Hn.data(), Hn.size(), c->stream, c->pool);
    if (rc) return fail(c, HSK_ERR_COMM, "allreduce(heavy list sizes) failed: %d (%s)", rc, cm.last_error.c_str());
    const size_t ew = (size_t)(NW + 1) * 8;
    const bool injected = test_fail(c, "heavybuf");
    bool oom = injected;
    std::vector<char *> buf(nh, nullptr);                // [heavy task] the owner's buffer, on its owner
    for (size_t i = 0; i < nh; ++i) {
        if (owner[hv_tasks[i]] != rank) continue;
        HeavyIn h; h.task = hv_tasks[i]; h.n = heavy_list_off(&Hn[i], nh, nranks); h.d_entries = nullptr;
        if (h.n && !oom) { h.d_entries = (u64 *)c->pool.alloc(h.n * ew); if (!h.d_entries) oom = true; }
        hin.push_back(h); buf[i] = (char *)h.d_entries;
    }
    {   // every owner must have its receive buffers before anybody sends
        std::vector<u64> none;
        const int st_ = cm.allreduce_with_status(none, RCCL_MAX, oom, c->stream, c->pool);
        if (st_ > 0) free_heavy_in(c, hin);
        if (st_) return left_together(c, st_, "status", oom ? fail(c, HSK_ERR_OOM, injected ? "heavy-hitter receive buffers (injected)" : "heavy-hitter receive buffers") : 0, "another rank ran out of memory before the heavy-hitter exchange");
    }
    {
        P2PGroup grp(cm);
        for (size_t i = 0; i < nh && !grp.rc; ++i) {
            const TaskOut &l = hlists[hv_tasks[i]]; const int o = owner[hv_tasks[i]];
            if (o != rank) { if (l.n) grp.send(l.entries, l.n * ew, o, c->stream, "ncclSend(heavy list)"); continue; }
            for (int p = 0; p < nranks; ++p) {
                const u64 n = Hn[(size_t)p * nh + i];
                if (n && p != rank) grp.recv(buf[i] + heavy_list_off(&Hn[i], nh, p) * ew, n * ew, p, c->stream, "ncclRecv(heavy list)");
            }
        }
        if (grp.end()) return fail(c, HSK_ERR_COMM, "heavy-hitter list exchange failed: %s", cm.last_error.c_str());
    }
    for (size_t i = 0; i < nh; ++i) {                                   // own share: device copy
        const TaskOut &l = hlists[hv_tasks[i]];
        if (owner[hv_tasks[i]] == rank && l.n) HIPCHK(c, hipMemcpyAsync(buf[i] + heavy_list_off(&Hn[i], nh, rank) * ew, l.entries, l.n * ew, hipMemcpyDeviceToDevice, c->stream));
    }
    HIPCHK(c, hsk_sync(c, c->stream));
    for (auto &to : hlists) free_task_out(c, to);
    return HSK_OK;
}

// Leaving together, part two (part one: the all-reduces with status up to the first task group: agree_on_tasks, exchange_or_feed, exchange_heavy_lists).
// A rank whose count failed while the groups were travelling keeps its side of the exchange going (drain_after_failure); then the ranks tell each other how it went, and if one
// of them failed they all return an error -- the failed rank its own, the others HSK_ERR_COMM.  rc: process_rank's on entry, the call's afterwards; false: the transport itself is broken.
static bool agree_on_outcome(hsk_ctx *c, GroupFeeder &feeder, unsigned long long before_rank, hsk_result *out, int &rc)
{
    if (rc != HSK_OK) {
        char keep_msg[sizeof c->err]; memcpy(keep_msg, c->err, sizeof keep_msg);
        hsk_result_free(c, out);                                               // (its blocks are the rollback's: dropped first)
        const int drc = feeder.drain_after_failure(before_rank);
        if (drc) { rc = drc; return false; }
        memcpy(c->err, keep_msg, sizeof keep_msg);
    }
    std::vector<u64> none;
    const int st_ = c->comm.allreduce_with_status(none, RCCL_MAX, rc != HSK_OK, c->stream, c->pool);
    const int trc = left_together(c, st_, "final status", rc, "another rank failed while the supermers were travelling; this rank's result is dropped");
    if (st_) rc = trc;
    return st_ >= 0;
}

template <int NW>
static int run_pipeline(hsk_ctx *c, const u8 *d_packed, u64 packed_bytes, const u64 *d_roff, const u32 *d_rlen, u64 nreads, int64_t rid_base, hsk_result *out)
{
    const bool ext = c->cfg.extension != 0;
    const int nranks = c->comm.active() ? c->comm.nranks : 1;
    const int rank = c->comm.active() ? c->comm.rank : 0;
    const CallInput in{d_packed, packed_bytes, d_roff, d_rlen, nreads, rid_base};
    ResultPriv *rp = begin_result(out, NW);
    PhaseTimer pt(c);
    pt.begin(PH_TOTAL);
    u32 ntasks = 0;
    int rc = plan_call<NW>(c, nranks, packed_bytes, ntasks); if (rc) return rc;
    out->ntasks = (int32_t)ntasks;
    const u32 vts = c->call.vt_shift;
    std::vector<int32_t> owner(ntasks, 0); std::vector<u32> order = identity_order(ntasks);

    // ---- parse ------------------------------------------------------------------------------------
    SupermerStore st;
    HeavySet hv(ntasks);
    std::vector<TaskOut> hlists;                         // this rank's {k-mer, count} lists of the heavy tasks
    std::vector<HeavyIn> hin;                            // heavy tasks this rank owns: the lists of all ranks
    std::vector<TaskSegs> segs(ntasks);
    int place_rc = HSK_OK; bool pipelined = false;
    pt.begin(PH_PARSE);
    rc = parse_pipelined(c, in, nranks, ntasks, st, segs, pipelined); if (rc) return rc;
    if (!pipelined) { rc = parse_two_steps<NW>(c, in, nranks, ntasks, hv, hlists, owner, order, st, place_rc); if (rc) return rc; }
    pt.end(PH_PARSE);
    c->call.vt_shift = 0;
    tmark("parse enqueued (task totals read)");
    out->total_supermers = st.tot_sup; out->total_supermer_bytes = st.tot_bytes + st.tot_sup * (ext ? 9 : 1);

    // ---- exchange (multi-GPU) ---------------------------------------------------------------------
    // After this block `segs[t]` lists where the supermers of owned task t live, and `x` says in which arrays.
    TaskInput x{st.sm_len, source_from_store(st, d_packed, packed_bytes), st.sm_pos, st.sm_rid};
    ExchangeBuffers xb;
    GroupFeeder feeder; bool fed = false;
    pt.begin(PH_EXCH);
    if (nranks > 1) {
        rc = exchange_or_feed(c, place_rc, ntasks, owner, order, st, x.src, feeder, fed, xb, segs); if (rc) return rc;
        if (!fed) x = TaskInput{xb.len, source_from_bytes(xb.bytes, xb.nbytes), xb.pos, xb.rid};
    } else if (!pipelined) segs_from_store(st, ntasks, vts, nullptr, segs);
    if (hv.any) { rc = exchange_heavy_lists<NW>(c, hv, owner, hlists, hin); if (rc) return rc; }
    pt.end(PH_EXCH);

    ProcExtra ex; ex.heavy_in = &hin; ex.vt_shift = vts; if (nranks == 1 && st.sm_item) ex.items_store = &st;
    const unsigned long long before_rank = c->pool.mark();
    rc = process_rank<NW>(c, ntasks, owner, rank, segs, x.len, x.src, x.pos, x.rid, out, rp, pt, true, fed ? &feeder : nullptr, &ex);
    if (rc == HSK_OK) add_unsent_kmers(c, out, c->call.dropped_now, hv, owner, rank);      // (one GPU: no task is heavy)
    if (fed && feeder.live && !agree_on_outcome(c, feeder, before_rank, out, rc)) return rc;
    free_heavy_in(c, hin);
    if (nranks > 1 && !fed) xb.release(c->pool); else free_store(c, st);
    return rc;
}

// ------------------------------------------------------------------------------------------------
// virtual ranks on one GPU: the multi-GPU data path (probe, dispatch, owner-grouped parse, pack,
// all-to-all-v plan, multi-segment expand) with device-to-device copies in place of RCCL send/recv.
// This is how the exchange logic is exercised on a single-GPU box (tests/test_gpu_multirank.py).
// ------------------------------------------------------------------------------------------------
struct DevInput { u8 *packed = nullptr; u64 *roff = nullptr; u32 *rlen = nullptr; };
// what run_pipeline does for its rank from process_rank on, for virtual rank r: its supermers come from the feeder's groups or lie in `x`
template <int NW, class ParseMs>
static int count_virtual_rank(hsk_ctx *c, u32 ntasks, const std::vector<int32_t> &owner, int r, std::vector<TaskSegs> &segs, const TaskInput &x, GroupFeeder *feeder, const std::vector<HeavyIn> &hin, const HeavySet &hv, u64 dropped, const ParseMs &parse_ms, hsk_result *out)
{
    ResultPriv *rp = begin_result(out, NW); out->ntasks = (int32_t)ntasks;
    PhaseTimer pt(c); ProcExtra ex; ex.heavy_in = &hin;
    const int rc = process_rank<NW>(c, ntasks, owner, r, segs, x.len, x.src, x.pos, x.rid, out, rp, pt, false, feeder, &ex);
    if (rc == HSK_OK) { add_unsent_kmers(c, out, dropped, hv, owner, r); sum_phases(*out, parse_ms(r)); }
    return rc;
}

template <int NW>
static int run_loopback(hsk_ctx *c, int R, const DevInput *in, const u64 *packed_bytes, const u64 *nreads, hsk_result *outs, int32_t *owner_out, u32 *ntasks_out)
{
    const bool ext = c->cfg.extension != 0;
    u64 tot_bytes = 0; for (int r = 0; r < R; ++r) tot_bytes += packed_bytes[r];
    const u32 ntasks = c->cfg.ntasks ? (u32)c->cfg.ntasks : auto_ntasks(c, tot_bytes / (u64)R + 1, R);
    *ntasks_out = ntasks;
    std::vector<int64_t> rid_base(R, 0);
    for (int r = 1; r < R; ++r) rid_base[r] = rid_base[r - 1] + (int64_t)nreads[r - 1];      // MPI_Exscan of the read counts
    // the plan, as plan_call chooses it with several ranks: the sketch of a rank's reads (here: of the first virtual rank that has some)
    const bool scan_ok = c->tune.parse_fast != 0 && c->cfg.minimizer_size <= SCAN_MAX_M;
    if (R > 1 && scan_ok && c->cfg.kmer_size <= 57) {          // (without a plan to choose, the sketch still says which k-mers are certain to be dropped)
        int r0 = 0; while (r0 + 1 < R && nreads[r0] == 0) ++r0;
        int erc = estimate_plan(c, in[r0].packed, packed_bytes[r0], in[r0].roff, in[r0].rlen, nreads[r0], R); if (erc) return erc;
        c->call.drop_mask_now = certain_drop_mask(c);              // (a rank that is certain is right for all: the virtual ranks share the first one's)
        c->call.combine_now = combine_allowed<NW>(c, R, tot_bytes / (u64)R);
    }
    // 1. hash every rank's reads once (parse_count), sum the task sizes
    std::vector<u64> bytes(ntasks, 0), kg(ntasks, 0), dropped(R, 0);
    std::vector<ParseJob> jobs(R);
    // per-rank device time of the parse (hash + count, then placement + byte store): outs[r].ms_parse
    EvList tev(c);
    std::vector<hipEvent_t> e0(R), e1(R), e2(R), e3(R);
    for (int r = 0; r < R; ++r) { e0[r] = tev.get(); e1[r] = tev.get(); e2[r] = tev.get(); e3[r] = tev.get(); }
    auto parse_ms = [&](int r) { float a = 0, b = 0; (void)hipEventElapsedTime(&a, e0[r], e1[r]); (void)hipEventElapsedTime(&b, e2[r], e3[r]); return (double)a + (double)b; };
    for (int r = 0; r < R; ++r) {
        (void)hipEventRecord(e0[r], c->stream);
        int rc = parse_count(c, in[r].packed, packed_bytes[r], in[r].roff, in[r].rlen, nreads[r], rid_base[r], ntasks, jobs[r]);
        dropped[r] = c->call.dropped_now;
        (void)hipEventRecord(e1[r], c->stream);
        if (rc) return rc;
        for (u32 t = 0; t < ntasks; ++t) { bytes[t] += jobs[r].task_tot[3 * t + 1] + jobs[r].task_tot[3 * t] * (ext ? 9 : 1); kg[t] += jobs[r].task_tot[3 * t + 2]; }
    }
    // 1b. heavy-hitter tasks: classify on the global k-mer counts, every rank pre-aggregates its share; then the dispatch
    HeavySet hv(ntasks);
    std::vector<std::vector<TaskOut>> hlists(R);
    if (heavy_enabled(c, R)) hv.classify(c, kg);
    if (hv.any) {
        std::vector<u64> bad(ntasks, 0);
        for (int r = 0; r < R; ++r) { int rc = heavy_preaggregate<NW>(c, jobs[r], in[r].packed, packed_bytes[r], hv.is_heavy, hlists[r], bad); if (rc) return rc; }
        hv.settle(c, bad, hlists.data(), R, (u64)(NW + 1) * 8, bytes);
    }
    std::vector<int32_t> owner(ntasks, 0); std::vector<u32> order = identity_order(ntasks);
    { int rc = dispatch_owners(c, bytes, R, owner, order); if (rc) return rc; }
    if (owner_out) memcpy(owner_out, owner.data(), sizeof(int32_t) * ntasks);
    // 2. owner-grouped placement + byte materialisation on every rank
    std::vector<SupermerStore> st(R);
    std::vector<u64> M((size_t)R * ntasks * 3, 0);
    for (int r = 0; r < R; ++r) {
        (void)hipEventRecord(e2[r], c->stream);
        int rc = parse_place(c, jobs[r], order, st[r], hv.any ? &hv.is_heavy : nullptr, R > 1);
        parse_release(c, jobs[r]);
        if (rc) return rc;
        rc = pack_store_bytes(c, st[r], source_from_packed(in[r].packed, packed_bytes[r], st[r].sm_gpos), c->tune.overlap == 0); if (rc) return rc;
        (void)hipEventRecord(e3[r], c->stream);
        std::copy_n(st[r].task_tot.begin(), (size_t)ntasks * 3, M.begin() + (size_t)r * ntasks * 3);
    }
    // 2b. the k-mer lists of the heavy tasks go to their owners (device copies here, send/recv in exchange_heavy_lists)
    std::vector<std::vector<HeavyIn>> hin(R);
    if (hv.any) {
        std::vector<u64> n(R);
        for (u32 t = 0; t < ntasks; ++t) {
            if (!hv.is_heavy[t]) continue;
            for (int r = 0; r < R; ++r) n[r] = hlists[r][t].n;
            HeavyIn h; h.task = t; h.n = heavy_list_off(n.data(), 1, R); h.d_entries = nullptr;
            if (h.n) DALLOC(c, h.d_entries, u64 *, h.n * (NW + 1) * 8);
            for (int r = 0; r < R; ++r) if (n[r]) HIPCHK(c, hipMemcpyAsync(h.d_entries + heavy_list_off(n.data(), 1, r) * (NW + 1), hlists[r][t].entries, n[r] * (NW + 1) * 8, hipMemcpyDeviceToDevice, c->stream));
            hin[owner[t]].push_back(h);
        }
        HIPCHK(c, hsk_sync(c, c->stream));
        for (auto &v : hlists) for (auto &to : v) free_task_out(c, to);
    }
    // 3. the exchange: same plans as the RCCL path (hsk_comm.h), device copies instead of send/recv
    std::vector<std::vector<TaskSegs>> segs(R);
    int rc_all = HSK_OK;
    if (c->tune.overlap != 0) {
        // grouped exchange overlapped with the sort, driven as run_pipeline drives it; 4. every rank finishes its own tasks while its groups travel
        std::vector<GroupFeeder> fd(R); std::vector<std::vector<ExchangePlan>> pl_all(R);
        bool all_sub = c->call.combine_now;
        for (int r = 0; r < R; ++r) if (st[r].tot_sup && !st[r].sm_sub16) all_sub = false;
        for (int d = 0; d < R; ++d) { int rc = fd[d].plan(c, R, d, ntasks, owner, order, M, st[d].task_base, segs[d]); if (rc) return rc; pl_all[d] = fd[d].pl; fd[d].with_sub = all_sub; }
        for (int r = 0; r < R && rc_all == HSK_OK; ++r) {
            fd[r].st_all = &st; fd[r].pl_all = &pl_all; fd[r].lazy_pack = true;
            rc_all = count_virtual_rank<NW>(c, ntasks, owner, r, segs[r], TaskInput{nullptr, BaseSource(), nullptr, nullptr}, &fd[r], hin[r], hv, dropped[r], parse_ms, &outs[r]);
        }
        for (int r = 0; r < R; ++r) free_store(c, st[r]);
    } else {
        std::vector<ExchangePlan> pl(R); std::vector<ExchangeBuffers> xb(R);
        for (int d = 0; d < R; ++d) {
            plan_exchange(R, d, ntasks, owner, order, M, st[d].task_base, pl[d], segs[d]);
            if (!xb[d].alloc(c->pool, pl[d], ext)) return fail(c, HSK_ERR_OOM, "exchange buffers");
        }
        for (int d = 0; d < R; ++d) for (int sidx = 0; sidx < R; ++sidx) { int rc = copy_share(c, st[sidx], pl[sidx], sidx, xb[d], pl[d], d, ext, false, c->stream); if (rc) return rc; }
        HIPCHK(c, hsk_sync(c, c->stream));
        for (int r = 0; r < R; ++r) free_store(c, st[r]);
        // 4. every rank finishes its own tasks
        for (int r = 0; r < R && rc_all == HSK_OK; ++r) {
            rc_all = count_virtual_rank<NW>(c, ntasks, owner, r, segs[r], TaskInput{xb[r].len, source_from_bytes(xb[r].bytes, xb[r].nbytes), xb[r].pos, xb[r].rid}, nullptr, hin[r], hv, dropped[r], parse_ms, &outs[r]);
            xb[r].release(c->pool);
        }
        if (rc_all) return rc_all;
    }
    for (auto &v : hin) free_heavy_in(c, v);
    return rc_all;
}
