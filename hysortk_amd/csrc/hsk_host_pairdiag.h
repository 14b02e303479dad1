// hsk_host_pairdiag.h -- host side of hsk_result_pair_diagonals, hsk_result_pair_diagonals_sliced and hsk_pair_diags_merge: the seed bins of
// every oriented read pair, and the best-supported one (kernels: hsk_pairdiag.h, hsk_rowmerge.h, and the expansion of hsk_pairs.h).  The
// range, the record pass, the count-and-emit driver, the slice plan, the stack of lists and its merges, the egress and the argument checks
// are those of hsk_host_pairs.h.  Part of the single translation unit hsk_api.hip (included in this order; everything here is file-local).
#pragma once

static const PassTexts diag_texts = {"read pair diagonals", "(two buffers of two-word keys and two value buffers) and the bin rows on top; ask for a narrower task range and join the all-bins lists",
                                     " and join the all-bins lists"};

// Expand a record window with the two-word key { sort word of the bin, pair key }, sort it, reduce it to bin rows (level 1) that stay on
// the device.  The whole range is the window { 0, nent, 0, records }.  The first window (rec0 == 0) also enqueues the bound of the
// positions, once for the range: every window's sort word is relative to it.  `last`: no window follows.  One wait for the sort's
// histogram and one for the bin count.  acc: self_records adds up, sort_passes is the most; keys and bins are this window's.
static int diag_window(hsk_ctx *c, PairRange &r, const PairWindow &w, bool last, int nw, u64 diag_w, u32 min_support, int32_t task_lo, int32_t task_hi, PairClock &ck, hsk_pair_diags *acc, PairList *list)
{
    const u64 records = w.records;
    u64 *const d_maxpos = r.d_stat + DIAG_STAT_MAXPOS;  // (zero since the count pass)
    RecordPass p;
    int rc = pairs_record_pass<2>(c, r, records, last, task_lo, task_hi, diag_texts, ck, p, [&](u32 xtiles) -> int {
        PairExpandArgs xa; memset(&xa, 0, sizeof xa);
        xa.tasks = r.d_tasks; xa.off = r.d_off; xa.loc = r.d_loc; xa.nent = w.ent1; xa.records = records; xa.keys = p.kA; xa.vals = p.vA; xa.diag_w = diag_w; xa.maxpos = d_maxpos;
        xa.rec0 = w.rec0; xa.ent0 = w.ent0;
        if (w.rec0) HIPCHK(c, hipMemsetAsync(r.d_stat, 0, DIAG_STAT_MAXPOS * 8, c->stream));      // (self_records of the slice before; the bound stays)
        else {
            DiagMaxArgs mx; memset(&mx, 0, sizeof mx);
            mx.tasks = r.d_tasks; mx.off = r.d_off; mx.loc = r.d_loc; mx.nent = r.nent; mx.nw = nw; mx.maxpos = d_maxpos;
            hipLaunchKernelGGL(diag_maxpos_kernel, dim3((u32)std::min<u64>((r.nent + PAIR_THREADS - 1) / PAIR_THREADS, 1u << 16)), dim3(PAIR_THREADS), 0, c->stream, mx);
        }
        hipLaunchKernelGGL((pair_expand_kernel<true, true>), dim3(xtiles), dim3(PAIR_THREADS), 0, c->stream, xa);
        return HSK_OK;
    });
    if (rc) return rc;
    acc->sort_passes = std::max<int32_t>(acc->sort_passes, p.passes);      // (the most over the slices)

    // ---- level 1: bin rows per tile, scans, write pass -----------------------------------------------------------------------------------
    const u64 rtiles = (records + DR_TILE - 1) / DR_TILE;
    DiagReduceArgs ra; memset(&ra, 0, sizeof ra);
    ra.keys = p.keys; ra.vals = p.vals; ra.n = records; ra.diag_w = diag_w; ra.maxpos = d_maxpos; ra.min_support = min_support; ra.stats = r.d_stat;
    CountEmit l1(c, ck, PT_REDUCE, rtiles, 3);
    static const int word1[3] = {PAIR_STAT_ROWS, PAIR_STAT_KEYS, DIAG_STAT_BINS};
    const u64 *st;
    rc = l1.count(r.d_stat, PAIR_STAT_WORDS, word1, &st, [&] {
        ra.tile_cnt = l1.tile[0]; ra.tile_keys = l1.tile[1]; ra.tile_bins = l1.tile[2];
        hipLaunchKernelGGL(diag_reduce_kernel<false>, dim3((u32)rtiles), dim3(PAIR_THREADS), 0, c->stream, ra);
    });
    if (rc) return rc;
    const u64 nbrows = st[PAIR_STAT_ROWS], self = st[PAIR_STAT_SELF];
    acc->self_records += self; acc->keys = st[PAIR_STAT_KEYS]; acc->bins = st[DIAG_STAT_BINS];
    if (nbrows > records || acc->bins > records || acc->keys > acc->bins || self > records)
        return fail(c, HSK_ERR_INTERNAL, "the bin reducer counted %llu rows, %llu bins and %llu keys in %llu records", (unsigned long long)nbrows, (unsigned long long)acc->bins, (unsigned long long)acc->keys, (unsigned long long)records);
    u64 *d_bins = nullptr;
    if (nbrows) { DALLOC(c, d_bins, u64 *, nbrows * DIAG_ROW_WORDS * 8); ra.rows = d_bins; }
    rc = l1.emit(nbrows != 0, [&] { hipLaunchKernelGGL(diag_reduce_kernel<true>, dim3((u32)rtiles), dim3(PAIR_THREADS), 0, c->stream, ra); });
    if (rc) return rc;
    p.release(c);
    list->rows = d_bins; list->n = nbrows; list->level = 0; list->owned = true;
    return HSK_OK;
}

// Level 2: the best bin of every key of an ascending all-bins list on the device; `allb` goes back behind the selection if the call owns
// it.  d_word: a device word of the call for the row count; max_keys: what the count may not exceed.  One wait.
static int diag_select(hsk_ctx *c, PairClock &ck, u64 *d_word, PairList &allb, u32 min_support, u64 max_keys, PairList *fin)
{
    *fin = allb;
    if (!allb.n) return HSK_OK;
    const u64 stiles = (allb.n + DS_TILE - 1) / DS_TILE;
    if (stiles > 0x7fffffffULL) return fail(c, HSK_ERR_UNSUPPORTED, "%llu bin rows are more than one launch selects from", (unsigned long long)allb.n);
    DiagSelectArgs sa; memset(&sa, 0, sizeof sa);
    sa.bins = allb.rows; sa.n = allb.n; sa.min_support = min_support;
    CountEmit l2(c, ck, PT_REDUCE, stiles, 1);
    static const int word2[1] = {0};
    const u64 *st;
    int rc = l2.count(d_word, 1, word2, &st, [&] {
        sa.tile_cnt = l2.tile[0];
        hipLaunchKernelGGL(diag_select_kernel<false>, dim3((u32)stiles), dim3(PAIR_THREADS), 0, c->stream, sa);
    });
    if (rc) return rc;
    fin->n = st[0]; fin->rows = nullptr; fin->owned = true;
    if (fin->n > max_keys) return fail(c, HSK_ERR_INTERNAL, "the selection counted %llu rows for %llu keys", (unsigned long long)fin->n, (unsigned long long)max_keys);
    if (fin->n) { DALLOC(c, fin->rows, u64 *, fin->n * DIAG_ROW_WORDS * 8); sa.rows = fin->rows; }
    rc = l2.emit(fin->n != 0, [&] { hipLaunchKernelGGL(diag_select_kernel<true>, dim3((u32)stiles), dim3(PAIR_THREADS), 0, c->stream, sa); });
    if (rc) return rc;
    if (allb.owned) c->pool.release(allb.rows);          // (behind the selection on the stream)
    allb.rows = nullptr; allb.n = 0;
    return HSK_OK;
}

// sliced == false (hsk_result_pair_diagonals), or a budget of at least `records`: one pass over the records of the whole range.  Waits: two
// for the record count, one for the sort's histogram, one for the bin count, one for the row count of the selection (not with all_bins),
// one at the end.  Else (hsk_result_pair_diagonals_sliced): one more wait for the plan, every slice a window of its own -- its all-bins
// list computed with min_support 1 -- and the lists meet on a PairStack of six-word rows: one wait per merge.  The last merge applies
// min_support with all_bins; without, the merges keep every row and the selection over the joined list applies it.  keys and bins are the
// last merge's counts.
static int pair_diags_impl(hsk_ctx *c, const ResultPriv *rp, const StrandsPriv *sp, int nw, int32_t task_lo, int32_t task_hi, u64 diag_w, u32 min_support, bool all_bins,
                           bool on_device, bool sliced, u64 max_records, hsk_pair_diags *out, hsk_pairs_slices *info, PairsPriv *pp)
{
    PairRange r; PairCall pc(c); bool go;
    PairClock &ck = pc.ck;
    info->slices = 1;
    int rc = pairs_begin(c, rp, sp, nw, task_lo, task_hi, r, pc, out, &go); if (rc || !go) return rc;
    const u64 records = r.records;
    u64 budget = records;
    if (sliced) budget = max_records ? max_records : pairs_auto_budget(c, 48);
    PairList allb, fin;
    u64 *d_word = r.d_stat + PAIR_STAT_ROWS;              // the selection's row count (the single pass: as it always was)
    std::vector<PairWindow> win;
    if (budget < records) { rc = pairs_plan_windows(c, r, budget, win); if (rc) return rc; }
    if (win.size() <= 1) {                               // the budget holds everything, or one entry has all the records: the reducer's own counts stand
        const PairWindow w = {0, r.nent, 0, records};
        rc = diag_window(c, r, w, true, nw, diag_w, all_bins ? min_support : 1, task_lo, task_hi, ck, out, &allb); if (rc) return rc;
        info->peak_records = records;
    } else {
        PairStack<DiagRow> stk;
        hsk_pair_diags acc; memset(&acc, 0, sizeof acc);
        for (size_t i = 0; i < win.size(); ++i) {
            const bool last = i + 1 == win.size();
            PairList l;
            rc = diag_window(c, r, win[i], last, nw, diag_w, 1, task_lo, task_hi, ck, &acc, &l); if (rc) return rc;
            info->peak_records = std::max<u64>(info->peak_records, win[i].records);
            rc = stk.push(c, l, !last, ck); if (rc) return rc;
        }
        PairMergeCounts cnt;
        rc = stk.finish(c, all_bins ? min_support : 1, ck, &allb, &cnt); if (rc) return rc;
        out->self_records = acc.self_records; out->sort_passes = acc.sort_passes; out->keys = cnt.keys; out->bins = cnt.bins;
        info->slices = win.size(); info->merges = stk.ms.merges; info->merged_rows = stk.ms.merged_rows;
    }
    if (all_bins) fin = allb;
    else { rc = diag_select(c, ck, d_word, allb, min_support, out->keys, &fin); if (rc) return rc; }
    c->pool.release(r.d_stat); r.d_stat = nullptr;
    const u64 nrows = fin.n;
    rc = pairs_egress(c, fin, DIAG_ROW_WORDS * 8, on_device, pc, pp); if (rc) return rc;
    pairs_store(out, nrows, pp, pc);
    info->ms_merge = ck.ms[PT_MERGE];
    return HSK_OK;
}

static int pair_diags_entry(hsk_ctx *c, const hsk_result *res, const hsk_strands *strands, int32_t task_lo, int32_t task_hi, uint64_t diag_bin, uint32_t min_support,
                            int32_t all_bins, int32_t on_device, bool sliced, uint64_t max_records, hsk_pair_diags *out, hsk_pairs_slices *info, const char *name)
{
    if (!c || !res || !out) return HSK_ERR_INVALID_ARG;
    memset(out, 0, sizeof *out);
    hsk_pairs_slices local; if (!info) info = &local;
    memset(info, 0, sizeof *info);
    if (!strands) return fail(c, HSK_ERR_INVALID_ARG, "%s: strands is NULL", name);
    if (diag_bin == 0 || diag_bin > DIAG_MAX_WIDTH) return fail(c, HSK_ERR_INVALID_ARG, "%s: diag_bin must be 1 .. 2^31 (%llu given)", name, (unsigned long long)diag_bin);
    if (min_support == 0) return fail(c, HSK_ERR_INVALID_ARG, "min_support must be at least 1");
    const ResultPriv *rp; const StrandsPriv *sp;
    int rc = pairs_check_args(c, res, strands, task_lo, task_hi, name, &rp, &sp); if (rc) return rc;
    rc = pairs_api_call(c, name, out, [&](PairsPriv *pp) {
        return pair_diags_impl(c, rp, sp, res->nw, task_lo, task_hi, diag_bin, min_support, all_bins != 0, on_device != 0, sliced, max_records, out, info, pp);
    });
    if (rc != HSK_OK) memset(info, 0, sizeof *info);
    return rc;
}

extern "C" int hsk_result_pair_diagonals(hsk_ctx *c, const hsk_result *res, const hsk_strands *strands, int32_t task_lo, int32_t task_hi, uint64_t diag_bin, uint32_t min_support,
                                         int32_t all_bins, int32_t on_device, hsk_pair_diags *out)
{
    return pair_diags_entry(c, res, strands, task_lo, task_hi, diag_bin, min_support, all_bins, on_device, false, 0, out, nullptr, "hsk_result_pair_diagonals");
}

extern "C" int hsk_result_pair_diagonals_sliced(hsk_ctx *c, const hsk_result *res, const hsk_strands *strands, int32_t task_lo, int32_t task_hi, uint64_t diag_bin, uint32_t min_support,
                                                int32_t all_bins, int32_t on_device, uint64_t max_records, hsk_pair_diags *out, hsk_pairs_slices *info)
{
    return pair_diags_entry(c, res, strands, task_lo, task_hi, diag_bin, min_support, all_bins, on_device, true, max_records, out, info, "hsk_result_pair_diagonals_sliced");
}

// The several-list contract of the all-bins lists on the GPU: pairs_stack_parts on six-word rows; the last merge counts keys and bins
// (a single list goes through a merge with nothing for that) and applies min_support with all_bins; without, the selection applies it.
static int pair_diags_merge_impl(hsk_ctx *c, const hsk_pair_diags *const *parts, int32_t nparts, u32 min_support, bool all_bins, bool on_device, hsk_pair_diags *out, PairsPriv *pp)
{
    PairCall pc(c);
    PairClock &ck = pc.ck;
    int rc = pc.start(c); if (rc) return rc;
    PairStack<DiagRow> stk;
    rc = pairs_stack_parts(c, parts, nparts, ck, stk, out); if (rc) return rc;
    PairList allb, fin; PairMergeCounts cnt;
    rc = stk.finish(c, all_bins ? min_support : 1, ck, &allb, &cnt); if (rc) return rc;
    out->keys = cnt.keys; out->bins = cnt.bins;
    if (all_bins) fin = allb;
    else {
        u64 *d_word = nullptr;
        if (allb.n) DALLOC(c, d_word, u64 *, 8);
        rc = diag_select(c, ck, d_word, allb, min_support, cnt.keys, &fin); if (rc) return rc;
        c->pool.release(d_word);
    }
    const u64 nrows = fin.n;
    rc = pairs_egress(c, fin, DIAG_ROW_WORDS * 8, on_device, pc, pp); if (rc) return rc;
    pairs_store(out, nrows, pp, pc);
    out->ms_reduce = ck.ms[PT_MERGE] + ck.ms[PT_REDUCE];  // (the merges and the selection are this call's reduction)
    return HSK_OK;
}

extern "C" int hsk_pair_diags_merge(hsk_ctx *c, const hsk_pair_diags *const *parts, int32_t nparts, uint32_t min_support, int32_t all_bins, int32_t on_device, hsk_pair_diags *out)
{
    if (!c || !out) return HSK_ERR_INVALID_ARG;
    memset(out, 0, sizeof *out);
    const int chk = pairs_merge_check(c, "hsk_pair_diags_merge", parts, nparts, min_support, "min_support"); if (chk) return chk;
    return pairs_api_call(c, "hsk_pair_diags_merge", out, [&](PairsPriv *pp) { return pair_diags_merge_impl(c, parts, nparts, min_support, all_bins != 0, on_device != 0, out, pp); });
}

extern "C" void hsk_pair_diags_free(hsk_ctx *c, hsk_pair_diags *p)
{
    if (!p) return;
    pairs_priv_free(c, p->priv);
    memset(p, 0, sizeof *p);
}
