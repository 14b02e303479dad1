// hsk_host_pairdiag.h -- host side of hsk_result_pair_diagonals: the seed bins of every oriented read pair, and the best-supported one
// (kernels: hsk_pairdiag.h, and the expansion of hsk_pairs.h).  The range, the record count and the argument checks are those of
// hsk_host_pairs.h.  Part of the single translation unit hsk_api.hip (included in this order; everything here is file-local).
#pragma once

// The final list to pinned host memory, or left on the device in a block the result owns; the call's last wait.
static int diags_egress(hsk_ctx *c, u64 *d_rows, u64 nrows, bool on_device, hipEvent_t e_end, PairClock &ck, hsk_pair_diags *out, PairsPriv *pp)
{
    const u64 bytes = nrows * DIAG_ROW_WORDS * 8;
    if (nrows && !on_device) {
        pp->host_rows = c->hpool.alloc(bytes);
        if (!pp->host_rows) return fail(c, HSK_ERR_OOM, "pinned host allocation of %llu bytes failed", (unsigned long long)bytes);
        ck.t.begin(PT_D2H);
        HIPCHK(c, hipMemcpyAsync(pp->host_rows, d_rows, bytes, hipMemcpyDeviceToHost, c->stream));
        ck.t.end(PT_D2H);
        c->stats.d2h_bytes += bytes;
    }
    HIPCHK(c, hipEventRecord(e_end, c->stream));
    HIPCHK(c, hsk_sync(c, c->stream));
    ck.take();
    if (!nrows || !on_device) { c->pool.release(d_rows); d_rows = nullptr; }
    pp->dev_rows = d_rows;
    out->n = nrows; out->rows = (uint64_t *)pp->host_rows; out->rows_dev = d_rows;
    out->ms_expand = ck.ms[PT_EXPAND]; out->ms_sort = ck.ms[PT_SORT]; out->ms_reduce = ck.ms[PT_REDUCE]; out->ms_d2h = ck.ms[PT_D2H];
    return HSK_OK;
}

// One pass over the records of the whole range (no slices: include/hsk.h says why).  Waits: two for the record count, one for the sort's
// histogram, one for the bin count, one for the row count of the selection (not with all_bins), one at the end.
static int pair_diags_impl(hsk_ctx *c, const ResultPriv *rp, const StrandsPriv *sp, int nw, int32_t task_lo, int32_t task_hi, u64 diag_w, u32 min_support, bool all_bins,
                           bool on_device, hsk_pair_diags *out, PairsPriv *pp)
{
    PairRange r;
    int rc = pairs_range_tasks(c, rp, task_lo, task_hi, r, sp); if (rc) return rc;
    if (!r.nent) return HSK_OK;
    EvList ev(c);
    hipEvent_t e_start = ev.get(), e_end = ev.get();
    PairClock ck(c);
    HIPCHK(c, hipEventRecord(e_start, c->stream));
    rc = pairs_count_records(c, nw, r, ck); if (rc) return rc;
    const u64 records = r.records;
    out->records = records;
    float f = 0;
    if (!records) {
        HIPCHK(c, hipEventRecord(e_end, c->stream)); HIPCHK(c, hsk_sync(c, c->stream));
        if (hipEventElapsedTime(&f, e_start, e_end) == hipSuccess) out->ms_expand = out->ms_total = f;
        pairs_release_range(c, r, true);
        return HSK_OK;
    }
    u64 *st = staging(c)->read_pairs;
    const u64 xtiles = (records + PX_TILE - 1) / PX_TILE;
    if (xtiles > 0x7fffffffULL) return fail(c, HSK_ERR_UNSUPPORTED, "%llu records are more than one launch expands; ask for a narrower task range and join the all-bins lists", (unsigned long long)records);

    // ---- expansion: the bound of the positions, then two-word keys { sort word of the bin, pair key } and the values ------------------
    // the working set: two key buffers of 2 * records words and two value buffers of records words (the sort's ping-pong)
    u64 *kA = (u64 *)c->pool.alloc(records * 16 + 64), *kB = (u64 *)c->pool.alloc(records * 16 + 64), *vA = (u64 *)c->pool.alloc(records * 8 + 64), *vB = (u64 *)c->pool.alloc(records * 8 + 64);
    if (!kA || !kB || !vA || !vB)
        return fail(c, HSK_ERR_OOM, "read pair diagonals of tasks [%d, %d): %llu records need %llu bytes of device memory (two buffers of two-word keys and two value buffers) and the bin rows on top; ask for a narrower task range and join the all-bins lists",
                    task_lo, task_hi, (unsigned long long)records, (unsigned long long)(records * 48));
    DiagMaxArgs mx; memset(&mx, 0, sizeof mx);
    mx.tasks = r.d_tasks; mx.off = r.d_off; mx.loc = r.d_loc; mx.nent = r.nent; mx.nw = nw; mx.maxpos = r.d_stat + DIAG_STAT_MAXPOS;      // (zero since the count pass)
    PairExpandArgs xa; memset(&xa, 0, sizeof xa);
    xa.tasks = r.d_tasks; xa.off = r.d_off; xa.loc = r.d_loc; xa.nent = r.nent; xa.records = records; xa.keys = kA; xa.vals = vA; xa.diag_w = diag_w; xa.maxpos = r.d_stat + DIAG_STAT_MAXPOS;
    ck.t.begin(PT_EXPAND);
    hipLaunchKernelGGL(diag_maxpos_kernel, dim3((u32)std::min<u64>((r.nent + PAIR_THREADS - 1) / PAIR_THREADS, 1u << 16)), dim3(PAIR_THREADS), 0, c->stream, mx);
    hipLaunchKernelGGL((pair_expand_kernel<true, true>), dim3((u32)xtiles), dim3(PAIR_THREADS), 0, c->stream, xa);
    HIPCHK(c, hipGetLastError());
    ck.t.end(PT_EXPAND);
    pairs_release_range(c, r, false);

    // ---- sort: the library's key + payload radix sort over both key words; digits in which all records agree are skipped ---------------
    ck.t.begin(PT_SORT);
    SortScratch sc; rc = alloc_sort_scratch(c, sc); if (rc) return rc;
    u64 *sk, *sv;
    rc = sort_task_device<2>(c, kA, kB, vA, vB, records, 64, sc, &sk, &sv, false); if (rc) return rc;
    out->sort_passes = 0;
    if (records >= 2) {
        // the scatter passes the sort took, from the histograms it left in the pinned staging block (as pairs_window reads them: -1 where
        // they do not add up to `records`)
        PassDesc plan[MAX_PASSES];
        const int npass = make_pass_plan(64, 2, c->cfg.radix_bits, plan, MAX_PASSES);
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
    ck.t.end(PT_SORT);

    // ---- level 1: bin rows per tile, scans, write pass -----------------------------------------------------------------------------------
    const u64 rtiles = (records + DR_TILE - 1) / DR_TILE;
    u64 *d_rtile, *d_rkeys, *d_rbins;
    DALLOC(c, d_rtile, u64 *, rtiles * 8); DALLOC(c, d_rkeys, u64 *, rtiles * 8); DALLOC(c, d_rbins, u64 *, rtiles * 8);
    DiagReduceArgs ra; memset(&ra, 0, sizeof ra);
    ra.keys = sk; ra.vals = sv; ra.n = records; ra.diag_w = diag_w; ra.maxpos = r.d_stat + DIAG_STAT_MAXPOS; ra.min_support = all_bins ? min_support : 1;
    ra.tile_cnt = d_rtile; ra.tile_keys = d_rkeys; ra.tile_bins = d_rbins; ra.stats = r.d_stat;
    ck.t.begin(PT_REDUCE);
    hipLaunchKernelGGL(diag_reduce_kernel<false>, dim3((u32)rtiles), dim3(PAIR_THREADS), 0, c->stream, ra);
    hipLaunchKernelGGL(count_scan_kernel, dim3(1), dim3(CNT_THREADS), 0, c->stream, d_rtile, rtiles, r.d_stat + PAIR_STAT_ROWS);
    hipLaunchKernelGGL(count_scan_kernel, dim3(1), dim3(CNT_THREADS), 0, c->stream, d_rkeys, rtiles, r.d_stat + PAIR_STAT_KEYS);      // (only their totals are used)
    hipLaunchKernelGGL(count_scan_kernel, dim3(1), dim3(CNT_THREADS), 0, c->stream, d_rbins, rtiles, r.d_stat + DIAG_STAT_BINS);
    HIPCHK(c, hipGetLastError());
    ck.t.end(PT_REDUCE);
    HIPCHK(c, hipMemcpyAsync(st, r.d_stat, PAIR_STAT_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hsk_sync(c, c->stream));
    ck.take();
    const u64 nbrows = st[PAIR_STAT_ROWS];
    out->self_records = st[PAIR_STAT_SELF]; out->keys = st[PAIR_STAT_KEYS]; out->bins = st[DIAG_STAT_BINS];
    if (nbrows > records || out->bins > records || out->keys > out->bins || out->self_records > records)
        return fail(c, HSK_ERR_INTERNAL, "the bin reducer counted %llu rows, %llu bins and %llu keys in %llu records", (unsigned long long)nbrows, (unsigned long long)out->bins, (unsigned long long)out->keys, (unsigned long long)records);
    u64 *d_bins = nullptr;
    if (nbrows) {
        DALLOC(c, d_bins, u64 *, nbrows * DIAG_ROW_WORDS * 8);
        ra.rows = d_bins;
        ck.t.begin(PT_REDUCE);
        hipLaunchKernelGGL(diag_reduce_kernel<true>, dim3((u32)rtiles), dim3(PAIR_THREADS), 0, c->stream, ra);
        HIPCHK(c, hipGetLastError());
        ck.t.end(PT_REDUCE);
    }
    c->pool.release(kA); c->pool.release(kB); c->pool.release(vA); c->pool.release(vB);
    c->pool.release(d_rtile); c->pool.release(d_rkeys); c->pool.release(d_rbins);

    // ---- level 2: the best bin of every key (all_bins: level 1 has written the list) -------------------------------------------------------
    u64 *d_rows = d_bins, nrows = nbrows;
    if (!all_bins && nbrows) {
        const u64 stiles = (nbrows + DS_TILE - 1) / DS_TILE;      // (at most xtiles: a launch holds them)
        u64 *d_stile; DALLOC(c, d_stile, u64 *, stiles * 8);
        DiagSelectArgs sa; memset(&sa, 0, sizeof sa);
        sa.bins = d_bins; sa.n = nbrows; sa.min_support = min_support; sa.tile_cnt = d_stile;
        ck.t.begin(PT_REDUCE);
        hipLaunchKernelGGL(diag_select_kernel<false>, dim3((u32)stiles), dim3(PAIR_THREADS), 0, c->stream, sa);
        hipLaunchKernelGGL(count_scan_kernel, dim3(1), dim3(CNT_THREADS), 0, c->stream, d_stile, stiles, r.d_stat + PAIR_STAT_ROWS);
        HIPCHK(c, hipGetLastError());
        ck.t.end(PT_REDUCE);
        HIPCHK(c, hipMemcpyAsync(st, r.d_stat + PAIR_STAT_ROWS, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hsk_sync(c, c->stream));
        ck.take();
        nrows = st[0];
        if (nrows > out->keys) return fail(c, HSK_ERR_INTERNAL, "the selection counted %llu rows for %llu keys", (unsigned long long)nrows, (unsigned long long)out->keys);
        d_rows = nullptr;
        if (nrows) {
            DALLOC(c, d_rows, u64 *, nrows * DIAG_ROW_WORDS * 8);
            sa.rows = d_rows;
            ck.t.begin(PT_REDUCE);
            hipLaunchKernelGGL(diag_select_kernel<true>, dim3((u32)stiles), dim3(PAIR_THREADS), 0, c->stream, sa);
            HIPCHK(c, hipGetLastError());
            ck.t.end(PT_REDUCE);
        }
        c->pool.release(d_bins); c->pool.release(d_stile);      // (behind the selection on the stream)
    }
    c->pool.release(r.d_stat); r.d_stat = nullptr;
    rc = diags_egress(c, d_rows, nrows, on_device, e_end, ck, out, pp); if (rc) return rc;
    if (hipEventElapsedTime(&f, e_start, e_end) == hipSuccess) out->ms_total = f;
    return HSK_OK;
}

extern "C" int hsk_result_pair_diagonals(hsk_ctx *c, const hsk_result *res, const hsk_strands *strands, int32_t task_lo, int32_t task_hi, uint64_t diag_bin, uint32_t min_support,
                                         int32_t all_bins, int32_t on_device, hsk_pair_diags *out)
{
    const char *name = "hsk_result_pair_diagonals";
    if (!c || !res || !out) return HSK_ERR_INVALID_ARG;
    memset(out, 0, sizeof *out);
    if (!strands) return fail(c, HSK_ERR_INVALID_ARG, "%s: strands is NULL", name);
    if (diag_bin == 0 || diag_bin > DIAG_MAX_WIDTH) return fail(c, HSK_ERR_INVALID_ARG, "%s: diag_bin must be 1 .. 2^31 (%llu given)", name, (unsigned long long)diag_bin);
    if (min_support == 0) return fail(c, HSK_ERR_INVALID_ARG, "min_support must be at least 1");
    const ResultPriv *rp; const StrandsPriv *sp;
    int rc = pairs_check_args(c, res, strands, task_lo, task_hi, name, &rp, &sp); if (rc) return rc;
    PairsPriv *pp = new PairsPriv();
    rc = ApiCall(c, name).run([&] { return pair_diags_impl(c, rp, sp, res->nw, task_lo, task_hi, diag_bin, min_support, all_bins != 0, on_device != 0, out, pp); });
    if (rc != HSK_OK) {                                   // (the device blocks went back with the call's rollback)
        if (pp->host_rows) c->hpool.release(pp->host_rows);
        delete pp;
        memset(out, 0, sizeof *out);
        return rc;
    }
    out->priv = pp;
    return HSK_OK;
}

extern "C" void hsk_pair_diags_free(hsk_ctx *c, hsk_pair_diags *p)
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
