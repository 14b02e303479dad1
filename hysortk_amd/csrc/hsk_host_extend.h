// hsk_host_extend.h -- host side of hsk_pair_diags_extend, hsk_pair_diags_extend_gapped and hsk_overlaps_free: the ungapped and the banded,
// gapped x-drop overlap of every diagonal row's seed, with the reads in HBM (kernels: hsk_extend.h, hsk_extend_gapped.h; the definitions:
// include/hsk.h, hsk_xdrop.h and hsk_gapped.h).  Both calls share extend_check (the arguments), extend_impl (uploads, the call's block, the
// refusals, the filter, the egress) and the scope of pairs_api_call; they differ in the kernels that walk.  The call's events, the
// count-and-emit driver, the egress and the scope of a call that returns a row list are those of hsk_host_pairs.h.
// Part of the single translation unit hsk_api.hip (included behind hsk_host_pairdiag.h; everything here is file-local).
#pragma once

// the gapped call's walk: its scores and band, and the lanes that take one row
struct GappedWalk { GpScore sc; int lanes; };

static void launch_gapped(hsk_ctx *c, const ExtendArgs &a, const GappedWalk &g)
{
    GappedArgs ga; ga.e = a; ga.sc = g.sc;
    const u64 groups = EG_THREADS / g.lanes;
    const dim3 grid((u32)((a.n + groups - 1) / groups)), block(EG_THREADS);
    switch (g.lanes) {
    case 8: hipLaunchKernelGGL(extend_gapped_kernel<8>, grid, block, 0, c->stream, ga); break;
    case 16: hipLaunchKernelGGL(extend_gapped_kernel<16>, grid, block, 0, c->stream, ga); break;
    case 32: hipLaunchKernelGGL(extend_gapped_kernel<32>, grid, block, 0, c->stream, ga); break;
    default: hipLaunchKernelGGL(extend_gapped_kernel<64>, grid, block, 0, c->stream, ga); break;
    }
}

// Host rows and host reads go up for the call (as hsk_pair_diags_merge and hsk_result_strands upload theirs).  Waits: the call's block behind
// the lane path -- the long-row count sizes the wave launch, and every refusal is known there, since the lane path checks every row --;
// with a filter the kept-row count; the end, which also brings the column sum behind the wave path.  The gapped call (g != nullptr) walks in
// one kernel, a group of g->lanes lanes per row: no long-row list, and the block's first word is the sum of the live cells.
static int extend_impl(hsk_ctx *c, const hsk_pair_diags *in, const void *packed, u64 packed_bytes, const void *roff, const void *rlen, u64 nreads, int64_t rid_base, bool reads_on_device,
                       const hsk_extend_opts *o, const GappedWalk *g, const char *fn, bool on_device, hsk_overlaps *out, PairsPriv *pp)
{
    const u64 n = in->n;
    out->input_rows = n;
    if (!n) return HSK_OK;
    const bool filter = o->min_score != 0 || o->min_length != 0;
    PairCall pc(c);
    PairClock &ck = pc.ck;
    int rc = pc.start(c); if (rc) return rc;
    u64 *d_in = (u64 *)in->rows_dev;
    if (!d_in) {
        DALLOC(c, d_in, u64 *, n * DIAG_ROW_WORDS * 8);
        HIPCHK(c, hipMemcpyAsync(d_in, in->rows, n * DIAG_ROW_WORDS * 8, hipMemcpyHostToDevice, c->stream));      // (pageable or pinned: the list outlives the call's last wait)
        c->stats.h2d_bytes += n * DIAG_ROW_WORDS * 8;
    }
    u8 *d_packed = nullptr; u64 *d_roff = nullptr; u32 *d_rlen = nullptr;
    if (!reads_on_device) {
        DALLOC(c, d_packed, u8 *, packed_bytes + 64); DALLOC(c, d_roff, u64 *, nreads * 8 + 64); DALLOC(c, d_rlen, u32 *, nreads * 4 + 64);
        if (packed_bytes) HIPCHK(c, hipMemcpyAsync(d_packed, packed, packed_bytes, hipMemcpyHostToDevice, c->stream));
        if (nreads) {
            HIPCHK(c, hipMemcpyAsync(d_roff, roff, nreads * 8, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(d_rlen, rlen, nreads * 4, hipMemcpyHostToDevice, c->stream));
        }
        c->stats.h2d_bytes += packed_bytes + nreads * 12;
    }
    u64 *d_out, *d_long = nullptr; u8 *d_keep = nullptr; unsigned long long *d_stat;
    DALLOC(c, d_out, u64 *, n * XD_ROW_WORDS * 8); DALLOC(c, d_stat, unsigned long long *, EXT_STAT_WORDS * 8);
    if (!g) DALLOC(c, d_long, u64 *, n * 8);
    if (filter) DALLOC(c, d_keep, u8 *, n);
    HIPCHK(c, hipMemsetAsync(d_stat, 0, EXT_STAT_WORDS * 8, c->stream));
    ExtendArgs a; memset(&a, 0, sizeof a);
    a.rows = d_in; a.n = n;
    a.packed = reads_on_device ? (const u8 *)packed : d_packed; a.packed_bytes = packed_bytes;
    a.roff = reads_on_device ? (const u64 *)roff : d_roff; a.rlen = reads_on_device ? (const u32 *)rlen : d_rlen; a.nreads = nreads; a.rid_base = rid_base;
    a.k = c->cfg.kmer_size; a.match = o->match; a.mismatch = o->mismatch; a.xdrop = o->xdrop;
    a.wave_span = o->wave_span == 0 ? EXT_DEFAULT_WAVE_SPAN : (o->wave_span == 0xffffffffu ? 1ULL << 40 : o->wave_span);
    a.min_score = o->min_score; a.min_length = o->min_length; a.filter = filter ? 1 : 0;
    a.out = d_out; a.keep = d_keep; a.long_rows = d_long; a.stat = d_stat;
    ck.t.begin(PT_EXPAND);
    if (g) launch_gapped(c, a, *g);
    else hipLaunchKernelGGL(extend_lane_kernel, dim3((u32)((n + EL_THREADS - 1) / EL_THREADS)), dim3(EL_THREADS), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    ck.t.end(PT_EXPAND);
    u64 *st = staging(c)->read_pairs;
    static_assert(EXT_STAT_WORDS * 8 <= sizeof(PinnedTail::read_pairs), "the call's block fits its staging words");
    HIPCHK(c, hipMemcpyAsync(st, d_stat, EXT_STAT_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hsk_sync(c, c->stream));
    ck.take();
    if (st[EXT_STAT_ERR_RID])
        return fail(c, HSK_ERR_INVALID_ARG, "%s: %llu of %llu rows name a read outside [%lld, %lld), the reads that were given", fn, (unsigned long long)st[EXT_STAT_ERR_RID], (unsigned long long)n,
                    (long long)rid_base, (long long)(rid_base + (int64_t)nreads));
    if (st[EXT_STAT_ERR_INDEX])
        return fail(c, HSK_ERR_INVALID_ARG, "%s: %llu of %llu rows name a read of the index that lies outside the %llu packed bytes", fn, (unsigned long long)st[EXT_STAT_ERR_INDEX], (unsigned long long)n,
                    (unsigned long long)packed_bytes);
    if (st[EXT_STAT_ERR_FIT])
        return fail(c, HSK_ERR_INVALID_ARG, "%s: the seed of %llu of %llu rows does not fit its reads (position + K lies behind a read's end): these are not the reads the rows were computed from", fn,
                    (unsigned long long)st[EXT_STAT_ERR_FIT], (unsigned long long)n);
    if (g && st[EXT_STAT_ERR_SPAN])
        return fail(c, HSK_ERR_INVALID_ARG, "%s: the two reads of %llu of %llu rows have 2^22 bases or more together: a banded extension takes la + lb < 2^22", fn,
                    (unsigned long long)st[EXT_STAT_ERR_SPAN], (unsigned long long)n);
    if (st[EXT_STAT_ERR_SEED])
        return fail(c, HSK_ERR_INVALID_ARG, "%s: the K columns of the seed of %llu of %llu rows do not all match: these are not the reads the rows were computed from", fn,
                    (unsigned long long)st[EXT_STAT_ERR_SEED], (unsigned long long)n);
    const u64 nlong = g ? 0 : st[EXT_STAT_LONG];
    u64 columns = st[EXT_STAT_COLUMNS], cells = g ? st[EXT_STAT_CELLS] : 0;
    if (nlong > n) return fail(c, HSK_ERR_INTERNAL, "%s: %llu long rows among %llu rows", fn, (unsigned long long)nlong, (unsigned long long)n);
    if (nlong) {
        a.nlong = nlong;
        ck.t.begin(PT_EXPAND);
        hipLaunchKernelGGL(extend_wave_kernel, dim3((u32)std::min<u64>((nlong + EW_WAVES - 1) / EW_WAVES, 1u << 16)), dim3(EW_THREADS), 0, c->stream, a);
        HIPCHK(c, hipGetLastError());
        ck.t.end(PT_EXPAND);
    }
    c->pool.release(d_long);
    PairList fin; fin.rows = d_out; fin.n = n; fin.owned = true;
    if (filter) {
        const u64 tiles = (n + EC_TILE - 1) / EC_TILE;
        ExtendCompactArgs ca; memset(&ca, 0, sizeof ca);
        ca.in = d_out; ca.keep = d_keep; ca.n = n;
        CountEmit ce(c, ck, PT_EXPAND, tiles, 1);
        static const int word[1] = {EXT_STAT_KEPT};
        const u64 *tot;
        rc = ce.count((u64 *)d_stat, EXT_STAT_WORDS, word, &tot, [&] {
            ca.tile_cnt = ce.tile[0];
            hipLaunchKernelGGL(extend_compact_kernel<false>, dim3((u32)tiles), dim3(RM_THREADS), 0, c->stream, ca);
        });
        if (rc) return rc;
        const u64 kept = tot[EXT_STAT_KEPT];
        columns = tot[EXT_STAT_COLUMNS];
        if (g) cells = tot[EXT_STAT_CELLS];
        if (kept > n) return fail(c, HSK_ERR_INTERNAL, "%s: the filter kept %llu of %llu rows", fn, (unsigned long long)kept, (unsigned long long)n);
        u64 *d_rows = nullptr;
        if (kept) { DALLOC(c, d_rows, u64 *, kept * XD_ROW_WORDS * 8); ca.rows = d_rows; }
        rc = ce.emit(kept != 0, [&] { hipLaunchKernelGGL(extend_compact_kernel<true>, dim3((u32)tiles), dim3(RM_THREADS), 0, c->stream, ca); });
        if (rc) return rc;
        c->pool.release(d_out); c->pool.release(d_keep);
        fin.rows = d_rows; fin.n = kept;
    } else if (nlong) HIPCHK(c, hipMemcpyAsync(st, d_stat, EXT_STAT_WORDS * 8, hipMemcpyDeviceToHost, c->stream));      // (the column sum behind the wave path: read behind the last wait)
    const u64 nrows = fin.n;
    rc = pairs_egress(c, fin, XD_ROW_WORDS * 8, on_device, pc, pp); if (rc) return rc;
    if (!filter && nlong) columns = st[EXT_STAT_COLUMNS];
    c->pool.release(d_stat);
    if (!in->rows_dev) c->pool.release(d_in);
    c->pool.release(d_packed); c->pool.release(d_roff); c->pool.release(d_rlen);
    out->n = nrows; out->rows = (uint64_t *)pp->host_rows; out->rows_dev = pp->dev_rows;
    out->dropped = n - nrows; out->columns = columns; out->wave_rows = nlong; out->cells = cells;
    out->ms_extend = ck.ms[PT_EXPAND]; out->ms_d2h = ck.ms[PT_D2H]; out->ms_total = pc.total();
    return HSK_OK;
}

// the arguments both calls share; rows_per_block: the fewest rows a workgroup of the call's walking kernel takes
static int extend_check(hsk_ctx *c, const char *fn, const hsk_pair_diags *in, const void *packed, uint64_t packed_bytes, const void *roff, const void *rlen, uint64_t nreads, int64_t rid_base,
                        int32_t reads_on_device, const void *o, u64 rows_per_block, hsk_overlaps *out)
{
    if (out) memset(out, 0, sizeof *out);
    if (!in || !o || !out) return fail(c, HSK_ERR_INVALID_ARG, "%s: a NULL pointer among the rows, the options and the result", fn);
    const u64 n = in->n;
    if ((nreads && (!roff || !rlen)) || (packed_bytes && !packed))
        return fail(c, HSK_ERR_INVALID_ARG, "%s: %llu rows, %llu reads in %llu packed bytes and a NULL pointer among packed, read_byte_off and read_len", fn, (unsigned long long)n,
                    (unsigned long long)nreads, (unsigned long long)packed_bytes);
    if (n && !in->rows_dev && !in->rows) return fail(c, HSK_ERR_INVALID_ARG, "%s: %llu rows and neither rows nor rows_dev", fn, (unsigned long long)n);
    if (n && ((uintptr_t)in->rows_dev & 15)) return fail(c, HSK_ERR_INVALID_ARG, "%s: rows_dev of the %llu rows is not 16-byte aligned", fn, (unsigned long long)n);
    if ((n + rows_per_block - 1) / rows_per_block > 0x7fffffffULL) return fail(c, HSK_ERR_INVALID_ARG, "%s: %llu rows are more than one launch extends", fn, (unsigned long long)n);
    if (rid_base < 0 || nreads > (1ULL << 31) || (u64)rid_base + nreads > (1ULL << 31))
        return fail(c, HSK_ERR_INVALID_ARG, "%s: read ids [%lld, %lld + %llu) do not lie below 2^31 (%llu rows)", fn, (long long)rid_base, (long long)rid_base, (unsigned long long)nreads, (unsigned long long)n);
    if (reads_on_device && ((uintptr_t)packed & 3) != 0) return fail(c, HSK_ERR_INVALID_ARG, "%s: packed must be 4-byte aligned on the device (%llu rows)", fn, (unsigned long long)n);
    return HSK_OK;
}

extern "C" int hsk_pair_diags_extend(hsk_ctx *c, const hsk_pair_diags *in, const void *packed, uint64_t packed_bytes, const void *roff, const void *rlen,
                                     uint64_t nreads, int64_t rid_base, int32_t reads_on_device, const hsk_extend_opts *o, int32_t on_device, hsk_overlaps *out)
{
    const char *fn = "hsk_pair_diags_extend";
    if (!c) return HSK_ERR_INVALID_ARG;
    const int rc = extend_check(c, fn, in, packed, packed_bytes, roff, rlen, nreads, rid_base, reads_on_device, o, EL_THREADS, out); if (rc) return rc;
    const u64 n = in->n;
    if (o->match < 1 || o->match > (1 << 15)) return fail(c, HSK_ERR_INVALID_ARG, "%s: match must be 1 .. 2^15 (%d given, %llu rows)", fn, o->match, (unsigned long long)n);
    if (o->mismatch < 0 || o->mismatch > (1 << 15)) return fail(c, HSK_ERR_INVALID_ARG, "%s: mismatch must be 0 .. 2^15 (%d given, %llu rows)", fn, o->mismatch, (unsigned long long)n);
    if (o->xdrop > 0x7fffffffu) return fail(c, HSK_ERR_INVALID_ARG, "%s: xdrop must be 0 .. 2^31 - 1 (%u given, %llu rows)", fn, o->xdrop, (unsigned long long)n);
    return pairs_api_call(c, fn, out, [&](PairsPriv *pp) { return extend_impl(c, in, packed, packed_bytes, roff, rlen, nreads, rid_base, reads_on_device != 0, o, nullptr, fn, on_device != 0, out, pp); });
}

extern "C" int hsk_pair_diags_extend_gapped(hsk_ctx *c, const hsk_pair_diags *in, const void *packed, uint64_t packed_bytes, const void *roff, const void *rlen,
                                            uint64_t nreads, int64_t rid_base, int32_t reads_on_device, const hsk_gapped_opts *o, int32_t on_device, hsk_overlaps *out)
{
    const char *fn = "hsk_pair_diags_extend_gapped";
    if (!c) return HSK_ERR_INVALID_ARG;
    const int rc = extend_check(c, fn, in, packed, packed_bytes, roff, rlen, nreads, rid_base, reads_on_device, o, EG_THREADS / 64, out); if (rc) return rc;
    const u64 n = in->n;
    if (o->match < 1 || o->match > 255) return fail(c, HSK_ERR_INVALID_ARG, "%s: match must be 1 .. 255 (%d given, %llu rows)", fn, o->match, (unsigned long long)n);
    if (o->mismatch < 0 || o->mismatch > 255) return fail(c, HSK_ERR_INVALID_ARG, "%s: mismatch must be 0 .. 255 (%d given, %llu rows)", fn, o->mismatch, (unsigned long long)n);
    if (o->gap < 0 || o->gap > 255) return fail(c, HSK_ERR_INVALID_ARG, "%s: gap must be 0 .. 255 (%d given, %llu rows)", fn, o->gap, (unsigned long long)n);
    if (o->xdrop > 0x7fffffffu) return fail(c, HSK_ERR_INVALID_ARG, "%s: xdrop must be 0 .. 2^31 - 1 (%u given, %llu rows)", fn, o->xdrop, (unsigned long long)n);
    if (o->band > (u32)GP_MAX_BAND) return fail(c, HSK_ERR_INVALID_ARG, "%s: band must be 0 .. %d (%u given, %llu rows)", fn, GP_MAX_BAND, o->band, (unsigned long long)n);
    if (o->group != 0 && o->group != 8 && o->group != 16 && o->group != 32 && o->group != 64)
        return fail(c, HSK_ERR_INVALID_ARG, "%s: group must be 0, 8, 16, 32 or 64 (%u given, %llu rows)", fn, o->group, (unsigned long long)n);
    if (o->group != 0 && o->band > o->group - 1)
        return fail(c, HSK_ERR_INVALID_ARG, "%s: a group of %u lanes holds bands up to %u (band %u given, %llu rows)", fn, o->group, o->group - 1, o->band, (unsigned long long)n);
    GappedWalk g;
    g.sc = gp_score(o->match, o->mismatch, o->gap, o->xdrop, o->band);
    g.lanes = o->group ? (int)o->group : (o->band < 8 ? 8 : o->band < 16 ? 16 : o->band < 32 ? 32 : 64);
    hsk_extend_opts eo; memset(&eo, 0, sizeof eo);
    eo.match = o->match; eo.mismatch = o->mismatch; eo.xdrop = o->xdrop; eo.min_score = o->min_score; eo.min_length = o->min_length;
    return pairs_api_call(c, fn, out, [&](PairsPriv *pp) { return extend_impl(c, in, packed, packed_bytes, roff, rlen, nreads, rid_base, reads_on_device != 0, &eo, &g, fn, on_device != 0, out, pp); });
}

extern "C" void hsk_overlaps_free(hsk_ctx *c, hsk_overlaps *p)
{
    if (!p) return;
    pairs_priv_free(c, p->priv);
    memset(p, 0, sizeof *p);
}
