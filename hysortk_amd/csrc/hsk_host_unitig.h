// hsk_host_unitig.h -- host side of hsk_overlaps_unitigs and hsk_unitigs_free: the unitigs of a list of string graph edges in HBM (kernels:
// hsk_unitig_kernels.h; the definition: include/hsk.h and hsk_unitig.h).  The arc records, their sort and the offsets are those of
// hsk_host_reduce.h; the call's events, the count-and-emit driver, the egress of the rows and the scope of the call those of hsk_host_pairs.h.
// Part of the single translation unit hsk_api.hip (included behind hsk_host_reduce.h; everything here is file-local).
#pragma once

struct UnitigsPriv { PairsPriv rows, table; };

// Host rows, host bits and host lengths go up for the call.  Waits: the call's block behind the arc count -- every refusal is known there --;
// the sort's histogram; the unitig and member counts, which size the two row lists; one per row list at the end.  The number of ranking
// rounds is fixed by what the host holds before the first launch: a chain has at most min(nreads, n + 1) vertices, so
// ut_rounds(min(nreads, n + 1)) steps bring every window to its head or around its cycle; the cut and as many steps again rank the cycles.
static int unitigs_impl(hsk_ctx *c, const hsk_overlaps *in, const void *contained, bool contained_on_device, const void *rlen, u64 nreads, int64_t rid_base, bool lens_on_device,
                        bool on_device, hsk_unitigs *out, UnitigsPriv *up)
{
    const char *fn = "hsk_overlaps_unitigs";
    const u64 n = in->n, nv = 2 * nreads, cwords = (nreads + 31) / 32, narcs = 2 * n;
    out->input_rows = n; out->nreads = nreads;
    PairCall pc(c);
    PairClock &ck = pc.ck;
    int rc = pc.start(c); if (rc) return rc;
    u64 *d_in = (u64 *)in->rows_dev;
    if (n && !d_in) {
        DALLOC(c, d_in, u64 *, n * XD_ROW_WORDS * 8);
        HIPCHK(c, hipMemcpyAsync(d_in, in->rows, n * XD_ROW_WORDS * 8, hipMemcpyHostToDevice, c->stream));        // (pageable or pinned: the list outlives the call's last wait)
        c->stats.h2d_bytes += n * XD_ROW_WORDS * 8;
    }
    u32 *d_len = nullptr, *d_con = nullptr;
    if (!lens_on_device) {
        DALLOC(c, d_len, u32 *, nreads * 4 + 64);
        if (nreads) HIPCHK(c, hipMemcpyAsync(d_len, rlen, nreads * 4, hipMemcpyHostToDevice, c->stream));
        c->stats.h2d_bytes += nreads * 4;
    }
    if (!contained || !contained_on_device) {
        DALLOC(c, d_con, u32 *, cwords * 4 + 64);
        if (!contained) HIPCHK(c, hipMemsetAsync(d_con, 0, cwords * 4 + 64, c->stream));
        else if (cwords) { HIPCHK(c, hipMemcpyAsync(d_con, contained, cwords * 4, hipMemcpyHostToDevice, c->stream)); c->stats.h2d_bytes += cwords * 4; }
    }
    u8 *d_cls; unsigned long long *d_stat;
    DALLOC(c, d_cls, u8 *, n + 64); DALLOC(c, d_stat, unsigned long long *, (UT_STAT_WORDS + RD_STAT_WORDS) * 8);
    HIPCHK(c, hipMemsetAsync(d_stat, 0, (UT_STAT_WORDS + RD_STAT_WORDS) * 8, c->stream));
    UnitigArgs a; memset(&a, 0, sizeof a);
    a.rows = d_in; a.n = n; a.rlen = lens_on_device ? (const u32 *)rlen : d_len; a.nreads = nreads; a.rid_base = rid_base;
    a.cls = d_cls; a.contained = d_con ? d_con : (const u32 *)contained; a.stat = d_stat;
    ReduceArgs ra; memset(&ra, 0, sizeof ra);            // what the kernels of hsk_reduce.h read
    ra.rows = d_in; ra.n = n; ra.rlen = a.rlen; ra.nreads = nreads; ra.rid_base = rid_base; ra.cls = d_cls; ra.contained = const_cast<u32 *>(a.contained); ra.cwords = cwords;
    ra.wave_degree = 1ULL << 40; ra.stat = d_stat + UT_STAT_WORDS;
    RecordPass p;
    if (n) {
        const u64 tiles = (n + EC_TILE - 1) / EC_TILE;
        static_assert(UT_STAT_UNITIGS * 8 <= sizeof(PinnedTail::read_pairs), "the words the call waits for fit their staging words");
        ck.t.begin(PT_EXPAND);
        hipLaunchKernelGGL(unitig_classify_kernel, dim3((u32)((n + UT_THREADS - 1) / UT_THREADS)), dim3(UT_THREADS), 0, c->stream, a);
        HIPCHK(c, hipGetLastError());
        ck.t.end(PT_EXPAND);
        CountEmit ce(c, ck, PT_EXPAND, tiles, 1);
        static const int word[1] = {UT_STAT_ROWS};
        const u64 *st;
        rc = ce.count((u64 *)d_stat, UT_STAT_UNITIGS, word, &st, [&] {
            ra.tile_cnt = ce.tile[0];
            hipLaunchKernelGGL(reduce_arcs_kernel<false>, dim3((u32)tiles), dim3(RM_THREADS), 0, c->stream, ra);
        });
        if (rc) return rc;
        if (st[UT_STAT_ERR_RID])
            return fail(c, HSK_ERR_INVALID_ARG, "%s: %llu of %llu rows name a read outside [%lld, %lld), the reads whose lengths were given", fn, (unsigned long long)st[UT_STAT_ERR_RID], (unsigned long long)n,
                        (long long)rid_base, (long long)(rid_base + (int64_t)nreads));
        if (st[UT_STAT_ERR_LEN])
            return fail(c, HSK_ERR_INVALID_ARG, "%s: the coordinates and the ends bits of %llu of %llu rows do not agree with the lengths given: these are not the lengths of the reads the rows were computed from", fn,
                        (unsigned long long)st[UT_STAT_ERR_LEN], (unsigned long long)n);
        if (st[UT_STAT_ERR_DOVE])
            return fail(c, HSK_ERR_INVALID_ARG, "%s: %llu of %llu rows are no dovetails: this is not a list of string graph edges", fn, (unsigned long long)st[UT_STAT_ERR_DOVE], (unsigned long long)n);
        if (st[UT_STAT_ERR_CONT])
            return fail(c, HSK_ERR_INVALID_ARG, "%s: %llu of %llu rows name a read whose contained bit is set: these are not the bits of the graph the rows are edges of", fn,
                        (unsigned long long)st[UT_STAT_ERR_CONT], (unsigned long long)n);
        if (st[UT_STAT_ROWS] != n) return fail(c, HSK_ERR_INTERNAL, "%s: %llu dovetails among %llu good rows", fn, (unsigned long long)st[UT_STAT_ROWS], (unsigned long long)n);
        // the arc records (+ 64: as every caller of the sort sizes them)
        p.kA = (u64 *)c->pool.alloc(narcs * 8 + 64); p.kB = (u64 *)c->pool.alloc(narcs * 8 + 64); p.vA = (u64 *)c->pool.alloc(narcs * 8 + 64); p.vB = (u64 *)c->pool.alloc(narcs * 8 + 64);
        if (!p.kA || !p.kB || !p.vA || !p.vB)
            return fail(c, HSK_ERR_OOM, "%s: %llu rows need %llu bytes of device memory for their arcs: 64 per row (two arc records, sorted in two buffers)", fn, (unsigned long long)n, (unsigned long long)(n * 64));
        ra.keys = p.kA; ra.vals = p.vA; ra.narcs = narcs;
        rc = ce.emit(true, [&] { hipLaunchKernelGGL(reduce_arcs_kernel<true>, dim3((u32)tiles), dim3(RM_THREADS), 0, c->stream, ra); });
        if (rc) return rc;
        ck.t.begin(PT_SORT);
        SortScratch sc; rc = alloc_sort_scratch(c, sc); if (rc) return rc;
        rc = sort_task_device<1>(c, p.kA, p.kB, p.vA, p.vB, narcs, 32, sc, &p.keys, &p.vals, false, &p.passes); if (rc) return rc;
        rc = check_device_error(c); if (rc) return rc;
        free_sort_scratch(c, sc);
        ck.t.end(PT_SORT);
    }
    u64 nunitigs = 0, nmembers = 0, rounds = 0;
    u64 *d_table = nullptr, *d_layout = nullptr;
    if (nv) {
        // per vertex: offsets 8, degree, target and pred 12, representative 8, unitig and first row 12, two states of 32
        const u64 per_vertex = 8 + 12 + 8 + 12 + 64;
        u64 *d_off = (u64 *)c->pool.alloc((nv + 1) * 8), *d_rep = (u64 *)c->pool.alloc(nv * 8), *d_first = (u64 *)c->pool.alloc(nv * 8);
        u32 *d_deg = (u32 *)c->pool.alloc(nv * 4), *d_cand = (u32 *)c->pool.alloc(nv * 4), *d_pred = (u32 *)c->pool.alloc(nv * 4), *d_uid = (u32 *)c->pool.alloc(nv * 4);
        UtState *d_sa = (UtState *)c->pool.alloc(nv * sizeof(UtState)), *d_sb = (UtState *)c->pool.alloc(nv * sizeof(UtState));
        if (!d_off || !d_rep || !d_first || !d_deg || !d_cand || !d_pred || !d_uid || !d_sa || !d_sb)
            return fail(c, HSK_ERR_OOM, "%s: %llu rows over %llu reads need %llu bytes of device memory for the ranking: %llu per vertex, two vertices per read", fn, (unsigned long long)n,
                        (unsigned long long)nreads, (unsigned long long)(nv * per_vertex + 8), (unsigned long long)per_vertex);
        const dim3 vgrid((u32)((nv + UT_THREADS - 1) / UT_THREADS)), block(UT_THREADS);
        ck.t.begin(PT_REDUCE);
        ra.keys = p.keys; ra.vals = p.vals; ra.narcs = n ? narcs : 0; ra.off = d_off;
        hipLaunchKernelGGL(reduce_offsets_kernel, dim3((u32)((nv + 1 + RD_THREADS - 1) / RD_THREADS)), dim3(RD_THREADS), 0, c->stream, ra);
        a.keys = p.keys; a.vals = p.vals; a.narcs = ra.narcs; a.off = d_off; a.deg = d_deg; a.cand = d_cand; a.pred = d_pred; a.rep = d_rep; a.uid = d_uid; a.ufirst = d_first;
        hipLaunchKernelGGL(unitig_out_kernel, vgrid, block, 0, c->stream, a);
        p.release(c); c->pool.release(d_off);            // (behind the launch on the stream: what is left of the arcs is per vertex)
        a.keys = a.vals = a.off = nullptr;
        a.nxt = d_sa;
        hipLaunchKernelGGL(unitig_link_kernel, vgrid, block, 0, c->stream, a);
        UtState *cur = d_sa, *nxt = d_sb;
        const u32 steps = n ? ut_rounds(std::min<u64>(nreads, n + 1)) : 0;
        for (int phase = 0; phase < 2 && steps; ++phase) {
            if (phase) { a.cur = cur; a.nxt = cur; hipLaunchKernelGGL(unitig_cut_kernel, vgrid, block, 0, c->stream, a); }
            for (u32 k = 0; k < steps; ++k, ++rounds) {
                a.cur = cur; a.nxt = nxt;
                hipLaunchKernelGGL(unitig_round_kernel, vgrid, block, 0, c->stream, a);
                std::swap(cur, nxt);
            }
        }
        HIPCHK(c, hipGetLastError());
        ck.t.end(PT_REDUCE);
        a.cur = cur; a.nxt = nullptr;
        CountEmit ch(c, ck, PT_MERGE, vgrid.x, 2);
        static const int hword[2] = {0, 1};
        const u64 *st;
        rc = ch.count((u64 *)d_stat + UT_STAT_UNITIGS, 2, hword, &st, [&] {
            a.tile_heads = ch.tile[0]; a.tile_reads = ch.tile[1];
            hipLaunchKernelGGL(unitig_heads_kernel<false>, vgrid, block, 0, c->stream, a);
        });
        if (rc) return rc;
        nunitigs = st[0]; nmembers = st[1];
        if (nunitigs > nmembers || nmembers > nreads) return fail(c, HSK_ERR_INTERNAL, "%s: %llu unitigs of %llu members over %llu reads", fn, (unsigned long long)nunitigs, (unsigned long long)nmembers, (unsigned long long)nreads);
        if (nunitigs) {
            d_table = (u64 *)c->pool.alloc(nunitigs * 32); d_layout = (u64 *)c->pool.alloc(nmembers * 32);
            if (!d_table || !d_layout) return fail(c, HSK_ERR_OOM, "%s: the %llu unitigs of %llu rows and their %llu members need %llu bytes of device memory", fn, (unsigned long long)nunitigs, (unsigned long long)n,
                                                   (unsigned long long)nmembers, (unsigned long long)((nunitigs + nmembers) * 32));
        }
        a.table = d_table; a.layout = d_layout; a.nunitigs = nunitigs; a.nmembers = nmembers;
        rc = ch.emit(true, [&] {
            hipLaunchKernelGGL(unitig_heads_kernel<true>, vgrid, block, 0, c->stream, a);
            hipLaunchKernelGGL(unitig_layout_kernel, vgrid, block, 0, c->stream, a);
            hipLaunchKernelGGL(unitig_census_kernel, dim3(std::min<u32>(vgrid.x, 2048)), block, 0, c->stream, a);
        });
        if (rc) return rc;
        c->pool.release(d_rep); c->pool.release(d_first); c->pool.release(d_deg); c->pool.release(d_cand); c->pool.release(d_pred); c->pool.release(d_uid);
        c->pool.release(d_sa); c->pool.release(d_sb);
    }
    u64 fin_stat[UT_STAT_WORDS];                         // (read behind the last wait)
    HIPCHK(c, hipMemcpyAsync(fin_stat, d_stat, sizeof fin_stat, hipMemcpyDeviceToHost, c->stream));
    PairList lay; lay.rows = d_layout; lay.n = nmembers; lay.owned = true;
    rc = pairs_egress(c, lay, 32, on_device, pc, &up->rows);
    if (rc) { (void)hsk_sync(c, c->stream); return rc; }  // (the copy into fin_stat may still be on its way)
    PairList tab; tab.rows = d_table; tab.n = nunitigs; tab.owned = true;
    rc = pairs_egress(c, tab, 32, on_device, pc, &up->table); if (rc) return rc;
    if (fin_stat[UT_STAT_BROKEN])
        return fail(c, HSK_ERR_INTERNAL, "%s: %llu checks that cannot fail did, over %llu rows: the layout would have holes", fn, (unsigned long long)fin_stat[UT_STAT_BROKEN], (unsigned long long)n);
    c->pool.release(d_cls); c->pool.release(d_stat); c->pool.release(d_len); c->pool.release(d_con);
    if (!in->rows_dev) c->pool.release(d_in);
    out->members = nmembers; out->rows = (uint64_t *)up->rows.host_rows; out->rows_dev = up->rows.dev_rows;
    out->unitigs = nunitigs; out->table = (uint64_t *)up->table.host_rows; out->table_dev = up->table.dev_rows;
    out->singletons = fin_stat[UT_STAT_SINGLE]; out->circular = fin_stat[UT_STAT_CIRCULAR]; out->longest = fin_stat[UT_STAT_LONGEST]; out->links = fin_stat[UT_STAT_LINKS];
    out->branch_vertices = fin_stat[UT_STAT_BRANCH]; out->live_reads = fin_stat[UT_STAT_LIVE]; out->arcs = fin_stat[UT_STAT_ARCS]; out->rounds = rounds;
    out->ms_arcs = ck.ms[PT_EXPAND]; out->ms_sort = ck.ms[PT_SORT]; out->ms_rank = ck.ms[PT_REDUCE]; out->ms_emit = ck.ms[PT_MERGE]; out->ms_d2h = ck.ms[PT_D2H]; out->ms_total = pc.total();
    return HSK_OK;
}

static void unitigs_priv_free(hsk_ctx *c, UnitigsPriv *up, bool device_too)
{
    for (PairsPriv *pp : {&up->rows, &up->table}) {
        if (c) {
            if (pp->host_rows) c->hpool.release(pp->host_rows);
            if (device_too) c->pool.release(pp->dev_rows);
        } else if (pp->host_rows) (void)hipHostFree(pp->host_rows);
    }
    delete up;
}

extern "C" int hsk_overlaps_unitigs(hsk_ctx *c, const hsk_overlaps *edges, const void *contained, int32_t contained_on_device, const void *read_len, uint64_t nreads, int64_t rid_base,
                                    int32_t lens_on_device, const hsk_unitig_opts *o, int32_t on_device, hsk_unitigs *out)
{
    const char *fn = "hsk_overlaps_unitigs";
    if (!c) return HSK_ERR_INVALID_ARG;
    if (out) memset(out, 0, sizeof *out);
    if (!edges || !o || !out) return fail(c, HSK_ERR_INVALID_ARG, "%s: a NULL pointer among the rows, the options and the result", fn);
    const u64 n = edges->n;
    if (nreads && !read_len) return fail(c, HSK_ERR_INVALID_ARG, "%s: %llu rows, %llu reads and a NULL pointer for read_len", fn, (unsigned long long)n, (unsigned long long)nreads);
    if (n && !edges->rows_dev && !edges->rows) return fail(c, HSK_ERR_INVALID_ARG, "%s: %llu rows and neither rows nor rows_dev", fn, (unsigned long long)n);
    if (n && ((uintptr_t)edges->rows_dev & 15)) return fail(c, HSK_ERR_INVALID_ARG, "%s: rows_dev of the %llu rows is not 16-byte aligned", fn, (unsigned long long)n);
    if (contained && contained_on_device && ((uintptr_t)contained & 3)) return fail(c, HSK_ERR_INVALID_ARG, "%s: the contained bits of the %llu rows' reads are not 4-byte aligned", fn, (unsigned long long)n);
    if (rid_base < 0 || nreads > (1ULL << 31) || (u64)rid_base + nreads > (1ULL << 31))
        return fail(c, HSK_ERR_INVALID_ARG, "%s: read ids [%lld, %lld + %llu) do not lie below 2^31 (%llu rows)", fn, (long long)rid_base, (long long)rid_base, (unsigned long long)nreads, (unsigned long long)n);
    if (n >> 32) return fail(c, HSK_ERR_INVALID_ARG, "%s: %llu rows are 2^32 or more: the row index travels in 32 bits", fn, (unsigned long long)n);
    UnitigsPriv *up = new UnitigsPriv();
    const int rc = ApiCall(c, fn).run([&] { return unitigs_impl(c, edges, contained, contained_on_device != 0, read_len, nreads, rid_base, lens_on_device != 0, on_device != 0, out, up); });
    if (rc != HSK_OK) {                                   // (the device blocks went back with the call's rollback)
        unitigs_priv_free(c, up, false);
        memset(out, 0, sizeof *out);
        return rc;
    }
    out->priv = up;
    return HSK_OK;
}

extern "C" void hsk_unitigs_free(hsk_ctx *c, hsk_unitigs *u)
{
    if (!u) return;
    if (u->priv) unitigs_priv_free(c, (UnitigsPriv *)u->priv, true);
    memset(u, 0, sizeof *u);
}
