// hsk_host_pairs.h -- host side of hsk_result_pairs: read pairs that share k-mers, from the resident EXTENSION list (kernels: hsk_pairs.h).
// Part of the single translation unit hsk_api.hip (included in this order; everything here is file-local).
#pragma once

struct PairsPriv { void *host_rows = nullptr; void *dev_rows = nullptr; };

// The tasks of the range go through ONE launch per kernel over a device table of task descriptors (at most HSK_MAX_TASKS of them):
// the records of the whole range are one array, sorted once.  Two waits before the large buffers exist (the record count), one per
// sort (its histogram), one for the row count, one at the end.
static int pairs_impl(hsk_ctx *c, const ResultPriv *rp, int nw, int32_t task_lo, int32_t task_hi, u32 min_shared, bool on_device, hsk_pairs *out, PairsPriv *pp)
{
    std::vector<PairTask> tk;
    u64 nent = 0;
    for (int32_t t = task_lo; t < task_hi; ++t) {
        const TaskOut &to = rp->dev_tasks[t];
        if (!to.n) continue;
        if (!to.entries || !to.payoff || !to.pos || !to.rid) return fail(c, HSK_ERR_INTERNAL, "task %d of the resident result has entries but no payload arrays", t);
        if (to.npay >> PAIR_LOC_SHIFT) return fail(c, HSK_ERR_UNSUPPORTED, "task %d holds %llu payloads (2^%d at most)", t, (unsigned long long)to.npay, PAIR_LOC_SHIFT);
        PairTask p; p.entries = to.entries; p.payoff = to.payoff; p.pos = to.pos; p.rid = to.rid; p.ent_base = nent; p.n = to.n; p.npay = to.npay; p.pay_base = to.pay_base;
        tk.push_back(p); nent += to.n;
    }
    if (!nent) return HSK_OK;
    EvList ev(c);
    hipEvent_t e_start = ev.get(), e_expand = ev.get(), e_sort = ev.get(), e_reduce = ev.get(), e_end = ev.get();
    HIPCHK(c, hipEventRecord(e_start, c->stream));

    // ---- record counts: t_e per entry, exclusive 64-bit offsets, the total ---------------------------------------------------
    const u64 ctiles = (nent + PC_TILE - 1) / PC_TILE;
    PairTask *d_tasks; u64 *d_off, *d_loc, *d_ctile, *d_stat;
    DALLOC(c, d_tasks, PairTask *, tk.size() * sizeof(PairTask));
    DALLOC(c, d_off, u64 *, (nent + 1) * 8); DALLOC(c, d_loc, u64 *, nent * 8);
    DALLOC(c, d_ctile, u64 *, ctiles * 8); DALLOC(c, d_stat, u64 *, PAIR_STAT_WORDS * 8);
    HIPCHK(c, hipMemcpyAsync(d_tasks, tk.data(), tk.size() * sizeof(PairTask), hipMemcpyHostToDevice, c->stream));     // (tk lives until the waits below)
    HIPCHK(c, hipMemsetAsync(d_stat, 0, PAIR_STAT_WORDS * 8, c->stream));
    PairSumArgs sa; memset(&sa, 0, sizeof sa);
    sa.tasks = d_tasks; sa.ntasks = (u32)tk.size(); sa.nw = nw; sa.nent = nent; sa.tile_sum = d_ctile; sa.off = d_off; sa.loc = d_loc; sa.err = (u32 *)(d_stat + PAIR_STAT_ERR);
    hipLaunchKernelGGL(pair_tsum_kernel<false>, dim3((u32)ctiles), dim3(PAIR_THREADS), 0, c->stream, sa);
    hipLaunchKernelGGL(count_scan_kernel, dim3(1), dim3(CNT_THREADS), 0, c->stream, d_ctile, ctiles, d_stat + PAIR_STAT_RECORDS);
    hipLaunchKernelGGL(pair_tsum_kernel<true>, dim3((u32)ctiles), dim3(PAIR_THREADS), 0, c->stream, sa);
    HIPCHK(c, hipGetLastError());
    u64 *st = staging(c)->read_pairs;
    HIPCHK(c, hipMemcpyAsync(st, d_stat, PAIR_STAT_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hsk_sync(c, c->stream));
    if (st[PAIR_STAT_ERR]) return fail(c, HSK_ERR_INTERNAL, "the resident result is not a valid CSR (%s)", (st[PAIR_STAT_ERR] & PAIR_ERR_COUNT) ? "an entry's count is above 65535" : "an entry's payload slice lies outside its task's payload");
    const u64 records = st[PAIR_STAT_RECORDS];
    out->records = records;
    c->pool.release(d_ctile);
    float f = 0;
    if (!records) {
        HIPCHK(c, hipEventRecord(e_end, c->stream)); HIPCHK(c, hsk_sync(c, c->stream));
        if (hipEventElapsedTime(&f, e_start, e_end) == hipSuccess) out->ms_expand = out->ms_total = f;
        c->pool.release(d_tasks); c->pool.release(d_off); c->pool.release(d_loc); c->pool.release(d_stat);
        return HSK_OK;
    }

    // ---- expansion -------------------------------------------------------------------------------------------------------------
    // the working set: two key and two value buffers of `records` words (the sort's ping-pong), known before any of them is asked for
    u64 *kA = (u64 *)c->pool.alloc(records * 8 + 64), *kB = (u64 *)c->pool.alloc(records * 8 + 64), *vA = (u64 *)c->pool.alloc(records * 8 + 64), *vB = (u64 *)c->pool.alloc(records * 8 + 64);      // (+ 64: as every caller of the sort sizes them)
    if (!kA || !kB || !vA || !vB)
        return fail(c, HSK_ERR_OOM, "read pairs of tasks [%d, %d): %llu records need %llu bytes of device memory (two key and two value buffers) and the rows on top; ask for a narrower task range and combine the lists",
                    task_lo, task_hi, (unsigned long long)records, (unsigned long long)(records * 32));
    PairExpandArgs xa; memset(&xa, 0, sizeof xa);
    xa.tasks = d_tasks; xa.off = d_off; xa.loc = d_loc; xa.nent = nent; xa.records = records; xa.keys = kA; xa.vals = vA;
    const u64 xtiles = (records + PX_TILE - 1) / PX_TILE;
    if (xtiles > 0x7fffffffULL) return fail(c, HSK_ERR_UNSUPPORTED, "%llu records are more than one launch expands; ask for a narrower task range", (unsigned long long)records);
    hipLaunchKernelGGL(pair_expand_kernel, dim3((u32)xtiles), dim3(PAIR_THREADS), 0, c->stream, xa);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(e_expand, c->stream));
    c->pool.release(d_tasks); c->pool.release(d_off); c->pool.release(d_loc);

    // ---- sort: the library's key + payload radix sort over all 64 key bits; digits in which all records agree are skipped -----------
    SortScratch sc; int rc = alloc_sort_scratch(c, sc); if (rc) return rc;
    u64 *sk, *sv;
    rc = sort_task_device<1>(c, kA, kB, vA, vB, records, 32, sc, &sk, &sv, false); if (rc) return rc;
    if (records >= 2) {
        // The scatter passes the sort took.  sort_task_device (hsk_host_sort.h, which this stage leaves as it is) does not say; it reads the digit
        // histograms of its plan back to the start of the pinned staging block -- hh[p * 256 + d], the bases behind them at MAX_PASSES * 256 -- and
        // scatters by every digit p in which no value holds all n records.  The same plan and the same test on the same words give the number.
        // Should the sort ever stage its histograms elsewhere, the rows found here no longer add up to `records`: then -1 (not known) is
        // reported, not a wrong count.
        PassDesc plan[MAX_PASSES];
        const int npass = make_pass_plan(32, 1, c->cfg.radix_bits, plan, MAX_PASSES);
        const u64 *hh = (const u64 *)c->pinned;
        int passes = 0;
        for (int p = 0; p < npass && passes >= 0; ++p) {
            bool trivial = false; u64 sum = 0;
            for (int d = 0; d < 256; ++d) { sum += hh[p * 256 + d]; if (hh[p * 256 + d] == records) trivial = true; }
            if (sum != records) passes = -1; else if (!trivial) ++passes;
        }
        out->sort_passes = npass < 0 ? -1 : passes;
    }
    rc = check_device_error(c); if (rc) return rc;
    free_sort_scratch(c, sc);
    HIPCHK(c, hipEventRecord(e_sort, c->stream));

    // ---- run reducer: rows per tile, scan, write pass ------------------------------------------------------------------------------
    const u64 rtiles = (records + PR_TILE - 1) / PR_TILE;
    u64 *d_rtile, *d_rkeys; DALLOC(c, d_rtile, u64 *, rtiles * 8); DALLOC(c, d_rkeys, u64 *, rtiles * 8);
    PairReduceArgs ra; memset(&ra, 0, sizeof ra);
    ra.keys = sk; ra.vals = sv; ra.n = records; ra.min_shared = min_shared; ra.tile_cnt = d_rtile; ra.tile_keys = d_rkeys; ra.stats = d_stat;
    hipLaunchKernelGGL(pair_reduce_kernel<false>, dim3((u32)rtiles), dim3(PAIR_THREADS), 0, c->stream, ra);
    hipLaunchKernelGGL(count_scan_kernel, dim3(1), dim3(CNT_THREADS), 0, c->stream, d_rtile, rtiles, d_stat + PAIR_STAT_ROWS);
    hipLaunchKernelGGL(count_scan_kernel, dim3(1), dim3(CNT_THREADS), 0, c->stream, d_rkeys, rtiles, d_stat + PAIR_STAT_KEYS);      // (only its total is used)
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(st, d_stat, PAIR_STAT_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hsk_sync(c, c->stream));
    const u64 nrows = st[PAIR_STAT_ROWS];
    out->n = nrows; out->self_records = st[PAIR_STAT_SELF]; out->keys = st[PAIR_STAT_KEYS];
    u64 *d_rows = nullptr;
    if (nrows) {
        DALLOC(c, d_rows, u64 *, nrows * 32);
        ra.rows = d_rows;
        hipLaunchKernelGGL(pair_reduce_kernel<true>, dim3((u32)rtiles), dim3(PAIR_THREADS), 0, c->stream, ra);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(e_reduce, c->stream));
    c->pool.release(kA); c->pool.release(kB); c->pool.release(vA); c->pool.release(vB); c->pool.release(d_rtile); c->pool.release(d_rkeys); c->pool.release(d_stat);

    // ---- egress ----------------------------------------------------------------------------------------------------------------------
    if (nrows && !on_device) {
        pp->host_rows = c->hpool.alloc(nrows * 32);
        if (!pp->host_rows) return fail(c, HSK_ERR_OOM, "pinned host allocation of %llu bytes failed", (unsigned long long)(nrows * 32));
        HIPCHK(c, hipMemcpyAsync(pp->host_rows, d_rows, nrows * 32, hipMemcpyDeviceToHost, c->stream));
        c->stats.d2h_bytes += nrows * 32;
    }
    HIPCHK(c, hipEventRecord(e_end, c->stream));
    HIPCHK(c, hsk_sync(c, c->stream));
    if (nrows && !on_device) { c->pool.release(d_rows); d_rows = nullptr; }
    pp->dev_rows = d_rows;
    out->rows = (uint64_t *)pp->host_rows; out->rows_dev = d_rows;
    if (hipEventElapsedTime(&f, e_start, e_expand) == hipSuccess) out->ms_expand = f;
    if (hipEventElapsedTime(&f, e_expand, e_sort) == hipSuccess) out->ms_sort = f;
    if (hipEventElapsedTime(&f, e_sort, e_reduce) == hipSuccess) out->ms_reduce = f;
    if (hipEventElapsedTime(&f, e_reduce, e_end) == hipSuccess) out->ms_d2h = f;
    if (hipEventElapsedTime(&f, e_start, e_end) == hipSuccess) out->ms_total = f;
    return HSK_OK;
}

extern "C" int hsk_result_pairs(hsk_ctx *c, const hsk_result *res, int32_t task_lo, int32_t task_hi, uint32_t min_shared, int32_t on_device, hsk_pairs *out)
{
    if (!c || !res || !out) return HSK_ERR_INVALID_ARG;
    memset(out, 0, sizeof *out);
    if (!c->cfg.extension) return fail(c, HSK_ERR_INVALID_ARG, "hsk_result_pairs needs a context with EXTENSION: without it the list carries no (ReadId, PosInRead)");
    const ResultPriv *rp = (const ResultPriv *)res->priv;
    if (!(c->cfg.flags & HSK_FLAG_KEEP_DEVICE) || !rp || res->ntasks <= 0 || rp->dev_tasks.size() != (size_t)res->ntasks)
        return fail(c, HSK_ERR_INVALID_ARG, "hsk_result_pairs needs a result that was left on the device (HSK_FLAG_KEEP_DEVICE)");
    if (task_lo < 0 || task_hi < task_lo || task_hi > res->ntasks) return fail(c, HSK_ERR_INVALID_ARG, "task range [%d, %d) outside [0, %d]", task_lo, task_hi, res->ntasks);
    if (min_shared == 0) return fail(c, HSK_ERR_INVALID_ARG, "min_shared must be at least 1");
    PairsPriv *pp = new PairsPriv();
    const int rc = ApiCall(c, "hsk_result_pairs").run([&] { return pairs_impl(c, rp, res->nw, task_lo, task_hi, min_shared, on_device != 0, out, pp); });
    if (rc != HSK_OK) {                                   // (the device blocks went back with the call's rollback)
        if (pp->host_rows) c->hpool.release(pp->host_rows);
        delete pp;
        memset(out, 0, sizeof *out);
        return rc;
    }
    out->priv = pp;
    return HSK_OK;
}

extern "C" void hsk_pairs_free(hsk_ctx *c, hsk_pairs *p)
{
    if (!p) return;
    PairsPriv *pp = (PairsPriv *)p->priv;
    if (pp) {
        if (c) { if (pp->host_rows) c->hpool.release(pp->host_rows); c->pool.release(pp->dev_rows); }
        else if (pp->host_rows) (void)hipHostFree(pp->host_rows);
        delete pp;
    }
    memset(p, 0, sizeof *p);
}
