// hsk_host_pairdiag.h -- host side of hsk_result_pair_diagonals: the seed bins of every oriented read pair, and the best-supported one
// (kernels: hsk_pairdiag.h, and the expansion of hsk_pairs.h).  The range, the record pass, the count-and-emit driver, the egress and the
// argument checks are those of hsk_host_pairs.h.  Part of the single translation unit hsk_api.hip (included in this order; everything
// here is file-local).
#pragma once

// One pass over the records of the whole range (no slices: include/hsk.h says why).  Waits: two for the record count, one for the sort's
// histogram, one for the bin count, one for the row count of the selection (not with all_bins), one at the end.
static int pair_diags_impl(hsk_ctx *c, const ResultPriv *rp, const StrandsPriv *sp, int nw, int32_t task_lo, int32_t task_hi, u64 diag_w, u32 min_support, bool all_bins,
                           bool on_device, hsk_pair_diags *out, PairsPriv *pp)
{
    static const PassTexts tx = {"read pair diagonals", "(two buffers of two-word keys and two value buffers) and the bin rows on top; ask for a narrower task range and join the all-bins lists",
                                 " and join the all-bins lists"};
    PairRange r; PairCall pc(c); bool go;
    PairClock &ck = pc.ck;
    int rc = pairs_begin(c, rp, sp, nw, task_lo, task_hi, r, pc, out, &go); if (rc || !go) return rc;
    const u64 records = r.records;
    u64 *const d_maxpos = r.d_stat + DIAG_STAT_MAXPOS;  // (zero since the count pass)

    // ---- expansion: the bound of the positions, then two-word keys { sort word of the bin, pair key } and the values; the sort -----------
    RecordPass p;
    rc = pairs_record_pass<2>(c, r, records, true, task_lo, task_hi, tx, ck, p, [&](u32 xtiles) -> int {
        DiagMaxArgs mx; memset(&mx, 0, sizeof mx);
        mx.tasks = r.d_tasks; mx.off = r.d_off; mx.loc = r.d_loc; mx.nent = r.nent; mx.nw = nw; mx.maxpos = d_maxpos;
        PairExpandArgs xa; memset(&xa, 0, sizeof xa);
        xa.tasks = r.d_tasks; xa.off = r.d_off; xa.loc = r.d_loc; xa.nent = r.nent; xa.records = records; xa.keys = p.kA; xa.vals = p.vA; xa.diag_w = diag_w; xa.maxpos = d_maxpos;
        hipLaunchKernelGGL(diag_maxpos_kernel, dim3((u32)std::min<u64>((r.nent + PAIR_THREADS - 1) / PAIR_THREADS, 1u << 16)), dim3(PAIR_THREADS), 0, c->stream, mx);
        hipLaunchKernelGGL((pair_expand_kernel<true, true>), dim3(xtiles), dim3(PAIR_THREADS), 0, c->stream, xa);
        return HSK_OK;
    });
    if (rc) return rc;
    out->sort_passes = p.passes;

    // ---- level 1: bin rows per tile, scans, write pass -----------------------------------------------------------------------------------
    const u64 rtiles = (records + DR_TILE - 1) / DR_TILE;
    DiagReduceArgs ra; memset(&ra, 0, sizeof ra);
    ra.keys = p.keys; ra.vals = p.vals; ra.n = records; ra.diag_w = diag_w; ra.maxpos = d_maxpos; ra.min_support = all_bins ? min_support : 1; ra.stats = r.d_stat;
    CountEmit l1(c, ck, PT_REDUCE, rtiles, 3);
    static const int word1[3] = {PAIR_STAT_ROWS, PAIR_STAT_KEYS, DIAG_STAT_BINS};
    const u64 *st;
    rc = l1.count(r.d_stat, PAIR_STAT_WORDS, word1, &st, [&] {
        ra.tile_cnt = l1.tile[0]; ra.tile_keys = l1.tile[1]; ra.tile_bins = l1.tile[2];
        hipLaunchKernelGGL(diag_reduce_kernel<false>, dim3((u32)rtiles), dim3(PAIR_THREADS), 0, c->stream, ra);
    });
    if (rc) return rc;
    const u64 nbrows = st[PAIR_STAT_ROWS];
    out->self_records = st[PAIR_STAT_SELF]; out->keys = st[PAIR_STAT_KEYS]; out->bins = st[DIAG_STAT_BINS];
    if (nbrows > records || out->bins > records || out->keys > out->bins || out->self_records > records)
        return fail(c, HSK_ERR_INTERNAL, "the bin reducer counted %llu rows, %llu bins and %llu keys in %llu records", (unsigned long long)nbrows, (unsigned long long)out->bins, (unsigned long long)out->keys, (unsigned long long)records);
    u64 *d_bins = nullptr;
    if (nbrows) { DALLOC(c, d_bins, u64 *, nbrows * DIAG_ROW_WORDS * 8); ra.rows = d_bins; }
    rc = l1.emit(nbrows != 0, [&] { hipLaunchKernelGGL(diag_reduce_kernel<true>, dim3((u32)rtiles), dim3(PAIR_THREADS), 0, c->stream, ra); });
    if (rc) return rc;
    p.release(c);

    // ---- level 2: the best bin of every key (all_bins: level 1 has written the list) -------------------------------------------------------
    PairList fin; fin.rows = d_bins; fin.n = nbrows;
    if (!all_bins && nbrows) {
        const u64 stiles = (nbrows + DS_TILE - 1) / DS_TILE;      // (at most the expansion's tiles: a launch holds them)
        DiagSelectArgs sa; memset(&sa, 0, sizeof sa);
        sa.bins = d_bins; sa.n = nbrows; sa.min_support = min_support;
        CountEmit l2(c, ck, PT_REDUCE, stiles, 1);
        static const int word2[1] = {0};
        rc = l2.count(r.d_stat + PAIR_STAT_ROWS, 1, word2, &st, [&] {
            sa.tile_cnt = l2.tile[0];
            hipLaunchKernelGGL(diag_select_kernel<false>, dim3((u32)stiles), dim3(PAIR_THREADS), 0, c->stream, sa);
        });
        if (rc) return rc;
        fin.n = st[0]; fin.rows = nullptr;
        if (fin.n > out->keys) return fail(c, HSK_ERR_INTERNAL, "the selection counted %llu rows for %llu keys", (unsigned long long)fin.n, (unsigned long long)out->keys);
        if (fin.n) { DALLOC(c, fin.rows, u64 *, fin.n * DIAG_ROW_WORDS * 8); sa.rows = fin.rows; }
        rc = l2.emit(fin.n != 0, [&] { hipLaunchKernelGGL(diag_select_kernel<true>, dim3((u32)stiles), dim3(PAIR_THREADS), 0, c->stream, sa); });
        if (rc) return rc;
        c->pool.release(d_bins);                         // (behind the selection on the stream)
    }
    c->pool.release(r.d_stat); r.d_stat = nullptr;
    const u64 nrows = fin.n;
    rc = pairs_egress(c, fin, DIAG_ROW_WORDS * 8, on_device, pc, pp); if (rc) return rc;
    pairs_store(out, nrows, pp, pc);
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
    const int rc = pairs_check_args(c, res, strands, task_lo, task_hi, name, &rp, &sp); if (rc) return rc;
    return pairs_api_call(c, name, out, [&](PairsPriv *pp) { return pair_diags_impl(c, rp, sp, res->nw, task_lo, task_hi, diag_bin, min_support, all_bins != 0, on_device != 0, out, pp); });
}

extern "C" void hsk_pair_diags_free(hsk_ctx *c, hsk_pair_diags *p)
{
    if (!p) return;
    pairs_priv_free(c, p->priv);
    memset(p, 0, sizeof *p);
}
