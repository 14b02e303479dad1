// hsk_host_reduce.h -- host side of hsk_overlaps_reduce and hsk_reduced_free: the string graph of a list of overlap rows in HBM (kernels:
// hsk_reduce.h; the definition: include/hsk.h and hsk_strgraph.h).  The call's events, the count-and-emit driver, the sort, the egress of the
// rows and the scope of the call are those of hsk_host_pairs.h.
// Part of the single translation unit hsk_api.hip (included behind hsk_host_extend.h; everything here is file-local).
#pragma once

// the kept rows as every row list holds them, and the class bytes and the contained bits on the side that was asked for
struct ReducedPriv { PairsPriv rows; void *cls_host = nullptr, *cls_dev = nullptr, *con_host = nullptr, *con_dev = nullptr; };

// Host rows and host lengths go up for the call.  Waits: the call's block behind the arc count -- every refusal is known there, and the
// dovetails between live reads size the arc records --; the sort's histogram; the kept-row count, which also brings the arcs, the largest
// degree and the wave path's vertices; the end, which brings the rows per class.  A list without such dovetails is not sorted and not reduced.
static int reduce_impl(hsk_ctx *c, const hsk_overlaps *in, const void *rlen, u64 nreads, int64_t rid_base, bool lens_on_device, const hsk_reduce_opts *o, bool on_device,
                       hsk_reduced *out, ReducedPriv *rp)
{
    const char *fn = "hsk_overlaps_reduce";
    const u64 n = in->n, nv = 2 * nreads, cwords = (nreads + 31) / 32;
    const u32 wave_degree = o->wave_degree ? o->wave_degree : RD_DEFAULT_WAVE_DEGREE;
    out->input_rows = n; out->nreads = nreads; out->wave_degree = wave_degree;
    PairCall pc(c);
    PairClock &ck = pc.ck;
    int rc = pc.start(c); if (rc) return rc;
    u64 *d_in = (u64 *)in->rows_dev;
    if (n && !d_in) {
        DALLOC(c, d_in, u64 *, n * XD_ROW_WORDS * 8);
        HIPCHK(c, hipMemcpyAsync(d_in, in->rows, n * XD_ROW_WORDS * 8, hipMemcpyHostToDevice, c->stream));        // (pageable or pinned: the list outlives the call's last wait)
        c->stats.h2d_bytes += n * XD_ROW_WORDS * 8;
    }
    u32 *d_len = nullptr;
    if (!lens_on_device) {
        DALLOC(c, d_len, u32 *, nreads * 4 + 64);
        if (nreads) HIPCHK(c, hipMemcpyAsync(d_len, rlen, nreads * 4, hipMemcpyHostToDevice, c->stream));
        c->stats.h2d_bytes += nreads * 4;
    }
    u8 *d_cls; u32 *d_con; unsigned long long *d_stat;
    DALLOC(c, d_cls, u8 *, n + 64); DALLOC(c, d_con, u32 *, cwords * 4 + 64); DALLOC(c, d_stat, unsigned long long *, RD_STAT_WORDS * 8);
    HIPCHK(c, hipMemsetAsync(d_con, 0, cwords * 4 + 64, c->stream));
    HIPCHK(c, hipMemsetAsync(d_stat, 0, RD_STAT_WORDS * 8, c->stream));
    ReduceArgs a; memset(&a, 0, sizeof a);
    a.rows = d_in; a.n = n; a.rlen = lens_on_device ? (const u32 *)rlen : d_len; a.nreads = nreads; a.rid_base = rid_base;
    a.cls = d_cls; a.contained = d_con; a.cwords = cwords; a.fuzz = o->fuzz; a.wave_degree = o->wave_degree == 0xffffffffu ? 1ULL << 40 : wave_degree; a.stat = d_stat;
    u64 kept = 0, arcs = 0, wave_vertices = 0, max_degree = 0;
    u64 *d_rows = nullptr;
    if (n) {
        const u64 tiles = (n + EC_TILE - 1) / EC_TILE;
        static_assert(RD_STAT_CLASS * 8 <= sizeof(PinnedTail::read_pairs), "the words the call waits for fit their staging words");
        ck.t.begin(PT_EXPAND);
        hipLaunchKernelGGL(reduce_classify_kernel, dim3((u32)((n + RD_THREADS - 1) / RD_THREADS)), dim3(RD_THREADS), 0, c->stream, a);
        HIPCHK(c, hipGetLastError());
        ck.t.end(PT_EXPAND);
        CountEmit ce(c, ck, PT_EXPAND, tiles, 1);
        static const int word[1] = {RD_STAT_ROWS};
        const u64 *st;
        rc = ce.count((u64 *)d_stat, RD_STAT_CLASS, word, &st, [&] {
            a.tile_cnt = ce.tile[0];
            hipLaunchKernelGGL(reduce_arcs_kernel<false>, dim3((u32)tiles), dim3(RM_THREADS), 0, c->stream, a);
        });
        if (rc) return rc;
        if (st[RD_STAT_ERR_RID])
            return fail(c, HSK_ERR_INVALID_ARG, "%s: %llu of %llu rows name a read outside [%lld, %lld), the reads whose lengths were given", fn, (unsigned long long)st[RD_STAT_ERR_RID], (unsigned long long)n,
                        (long long)rid_base, (long long)(rid_base + (int64_t)nreads));
        if (st[RD_STAT_ERR_LEN])
            return fail(c, HSK_ERR_INVALID_ARG, "%s: the coordinates and the ends bits of %llu of %llu rows do not agree with the lengths given: these are not the lengths of the reads the rows were computed from", fn,
                        (unsigned long long)st[RD_STAT_ERR_LEN], (unsigned long long)n);
        const u64 dov = st[RD_STAT_ROWS], narcs = 2 * dov;
        if (dov > n) return fail(c, HSK_ERR_INTERNAL, "%s: %llu dovetails among %llu rows", fn, (unsigned long long)dov, (unsigned long long)n);
        if (dov) {
            // the working set, known before any of it is asked for (+ 64: as every caller of the sort sizes them)
            RecordPass p;
            p.kA = (u64 *)c->pool.alloc(narcs * 8 + 64); p.kB = (u64 *)c->pool.alloc(narcs * 8 + 64); p.vA = (u64 *)c->pool.alloc(narcs * 8 + 64); p.vB = (u64 *)c->pool.alloc(narcs * 8 + 64);
            u64 *d_off = (u64 *)c->pool.alloc((nv + 1) * 8);
            if (!p.kA || !p.kB || !p.vA || !p.vB || !d_off)
                return fail(c, HSK_ERR_OOM, "%s: %llu rows with %llu dovetails between live reads need %llu bytes of device memory: 64 per dovetail (two arc records, sorted in two buffers) and 8 x (2 x %llu reads + 1)", fn,
                            (unsigned long long)n, (unsigned long long)dov, (unsigned long long)(dov * 64 + (nv + 1) * 8), (unsigned long long)nreads);
            a.keys = p.kA; a.vals = p.vA; a.narcs = narcs;
            rc = ce.emit(true, [&] { hipLaunchKernelGGL(reduce_arcs_kernel<true>, dim3((u32)tiles), dim3(RM_THREADS), 0, c->stream, a); });
            if (rc) return rc;
            ck.t.begin(PT_SORT);
            SortScratch sc; rc = alloc_sort_scratch(c, sc); if (rc) return rc;
            rc = sort_task_device<1>(c, p.kA, p.kB, p.vA, p.vB, narcs, 32, sc, &p.keys, &p.vals, false, &p.passes); if (rc) return rc;
            rc = check_device_error(c); if (rc) return rc;
            free_sort_scratch(c, sc);
            ck.t.end(PT_SORT);
            ck.t.begin(PT_REDUCE);
            a.keys = p.keys; a.vals = p.vals; a.vals_out = p.vals == p.vA ? p.vB : p.vA; a.off = d_off;
            const dim3 agrid((u32)((narcs + RD_THREADS - 1) / RD_THREADS)), block(RD_THREADS);
            hipLaunchKernelGGL(reduce_dups_kernel, agrid, block, 0, c->stream, a);
            a.vals = a.vals_out; a.vals_out = nullptr;   // (duplicates out: what the offsets and the reduction read)
            hipLaunchKernelGGL(reduce_offsets_kernel, dim3((u32)((nv + 1 + RD_THREADS - 1) / RD_THREADS)), block, 0, c->stream, a);
            hipLaunchKernelGGL(reduce_lane_kernel, agrid, block, 0, c->stream, a);
            if (o->wave_degree != 0xffffffffu) hipLaunchKernelGGL(reduce_wave_kernel, dim3((u32)std::min<u64>(nv, 1u << 14)), block, 0, c->stream, a);
            HIPCHK(c, hipGetLastError());
            ck.t.end(PT_REDUCE);
            p.release(c); c->pool.release(d_off);
        } else { rc = ce.emit(false, [] {}); if (rc) return rc; }
        // the kept rows, in the input's order
        ExtendCompactArgs ca; memset(&ca, 0, sizeof ca);
        ca.in = d_in; ca.keep = d_cls; ca.n = n;
        CountEmit cc(c, ck, PT_REDUCE, tiles, 1);
        static const int kword[1] = {RD_STAT_KEPT};
        rc = cc.count((u64 *)d_stat, RD_STAT_CLASS, kword, &st, [&] {
            ca.tile_cnt = cc.tile[0];
            hipLaunchKernelGGL((extend_compact_kernel<false, true>), dim3((u32)tiles), dim3(RM_THREADS), 0, c->stream, ca);
        });
        if (rc) return rc;
        kept = st[RD_STAT_KEPT]; arcs = st[RD_STAT_ARCS]; wave_vertices = st[RD_STAT_WAVE]; max_degree = st[RD_STAT_MAXDEG];
        if (kept > dov) return fail(c, HSK_ERR_INTERNAL, "%s: %llu rows kept of %llu dovetails", fn, (unsigned long long)kept, (unsigned long long)dov);
        if (kept) {
            d_rows = (u64 *)c->pool.alloc(kept * XD_ROW_WORDS * 8);
            if (!d_rows) return fail(c, HSK_ERR_OOM, "%s: the %llu kept rows of %llu need %llu bytes of device memory", fn, (unsigned long long)kept, (unsigned long long)n, (unsigned long long)(kept * XD_ROW_WORDS * 8));
            ca.rows = d_rows;
        }
        rc = cc.emit(kept != 0, [&] { hipLaunchKernelGGL((extend_compact_kernel<true, true>), dim3((u32)tiles), dim3(RM_THREADS), 0, c->stream, ca); });
        if (rc) return rc;
        ck.t.begin(PT_REDUCE);
        hipLaunchKernelGGL(reduce_census_kernel, dim3((u32)std::min<u64>((n + RD_THREADS - 1) / RD_THREADS, 2048)), dim3(RD_THREADS), 0, c->stream, a);
        HIPCHK(c, hipGetLastError());
        ck.t.end(PT_REDUCE);
    }
    u64 fin_stat[RD_STAT_WORDS];                         // (read behind the last wait)
    HIPCHK(c, hipMemcpyAsync(fin_stat, d_stat, sizeof fin_stat, hipMemcpyDeviceToHost, c->stream));
    if (!on_device) {
        rp->cls_host = c->hpool.alloc(n); rp->con_host = c->hpool.alloc(cwords * 4);
        if (!rp->cls_host || !rp->con_host) return fail(c, HSK_ERR_OOM, "%s: pinned host allocation of %llu bytes failed", fn, (unsigned long long)(n + cwords * 4));
        ck.t.begin(PT_D2H);
        if (n) HIPCHK(c, hipMemcpyAsync(rp->cls_host, d_cls, n, hipMemcpyDeviceToHost, c->stream));
        if (cwords) HIPCHK(c, hipMemcpyAsync(rp->con_host, d_con, cwords * 4, hipMemcpyDeviceToHost, c->stream));
        ck.t.end(PT_D2H);
        c->stats.d2h_bytes += n + cwords * 4;
    }
    PairList fin; fin.rows = d_rows; fin.n = kept; fin.owned = true;
    rc = pairs_egress(c, fin, XD_ROW_WORDS * 8, on_device, pc, &rp->rows); if (rc) return rc;
    if (on_device) { rp->cls_dev = d_cls; rp->con_dev = d_con; }
    else { c->pool.release(d_cls); c->pool.release(d_con); }
    c->pool.release(d_stat); c->pool.release(d_len);
    if (!in->rows_dev) c->pool.release(d_in);
    out->n = kept; out->rows = (uint64_t *)rp->rows.host_rows; out->rows_dev = rp->rows.dev_rows;
    out->row_class = (uint8_t *)rp->cls_host; out->row_class_dev = rp->cls_dev; out->contained = (uint32_t *)rp->con_host; out->contained_dev = rp->con_dev;
    for (int k = 0; k < SG_CLASSES; ++k) out->class_rows[k] = fin_stat[RD_STAT_CLASS + k];
    out->contained_reads = fin_stat[RD_STAT_CONTAINED]; out->arcs = arcs; out->wave_vertices = wave_vertices; out->max_degree = max_degree;
    out->ms_classify = ck.ms[PT_EXPAND]; out->ms_sort = ck.ms[PT_SORT]; out->ms_reduce = ck.ms[PT_REDUCE]; out->ms_d2h = ck.ms[PT_D2H]; out->ms_total = pc.total();
    return HSK_OK;
}

static void reduced_priv_free(hsk_ctx *c, ReducedPriv *rp, bool device_too)
{
    if (c) {
        if (rp->rows.host_rows) c->hpool.release(rp->rows.host_rows);
        if (rp->cls_host) c->hpool.release(rp->cls_host);
        if (rp->con_host) c->hpool.release(rp->con_host);
        if (device_too) { c->pool.release(rp->rows.dev_rows); c->pool.release(rp->cls_dev); c->pool.release(rp->con_dev); }
    } else {
        if (rp->rows.host_rows) (void)hipHostFree(rp->rows.host_rows);
        if (rp->cls_host) (void)hipHostFree(rp->cls_host);
        if (rp->con_host) (void)hipHostFree(rp->con_host);
    }
    delete rp;
}

extern "C" int hsk_overlaps_reduce(hsk_ctx *c, const hsk_overlaps *in, const void *read_len, uint64_t nreads, int64_t rid_base, int32_t lens_on_device, const hsk_reduce_opts *o,
                                   int32_t on_device, hsk_reduced *out)
{
    const char *fn = "hsk_overlaps_reduce";
    if (!c) return HSK_ERR_INVALID_ARG;
    if (out) memset(out, 0, sizeof *out);
    if (!in || !o || !out) return fail(c, HSK_ERR_INVALID_ARG, "%s: a NULL pointer among the rows, the options and the result", fn);
    const u64 n = in->n;
    if (nreads && !read_len) return fail(c, HSK_ERR_INVALID_ARG, "%s: %llu rows, %llu reads and a NULL pointer for read_len", fn, (unsigned long long)n, (unsigned long long)nreads);
    if (n && !in->rows_dev && !in->rows) return fail(c, HSK_ERR_INVALID_ARG, "%s: %llu rows and neither rows nor rows_dev", fn, (unsigned long long)n);
    if (n && ((uintptr_t)in->rows_dev & 15)) return fail(c, HSK_ERR_INVALID_ARG, "%s: rows_dev of the %llu rows is not 16-byte aligned", fn, (unsigned long long)n);
    if (rid_base < 0 || nreads > (1ULL << 31) || (u64)rid_base + nreads > (1ULL << 31))
        return fail(c, HSK_ERR_INVALID_ARG, "%s: read ids [%lld, %lld + %llu) do not lie below 2^31 (%llu rows)", fn, (long long)rid_base, (long long)rid_base, (unsigned long long)nreads, (unsigned long long)n);
    if (n >> 32) return fail(c, HSK_ERR_INVALID_ARG, "%s: %llu rows are 2^32 or more: the row index travels in 32 bits", fn, (unsigned long long)n);
    ReducedPriv *rp = new ReducedPriv();
    const int rc = ApiCall(c, fn).run([&] { return reduce_impl(c, in, read_len, nreads, rid_base, lens_on_device != 0, o, on_device != 0, out, rp); });
    if (rc != HSK_OK) {                                   // (the device blocks went back with the call's rollback)
        reduced_priv_free(c, rp, false);
        memset(out, 0, sizeof *out);
        return rc;
    }
    out->priv = rp;
    return HSK_OK;
}

extern "C" void hsk_reduced_free(hsk_ctx *c, hsk_reduced *r)
{
    if (!r) return;
    if (r->priv) reduced_priv_free(c, (ReducedPriv *)r->priv, true);
    memset(r, 0, sizeof *r);
}
