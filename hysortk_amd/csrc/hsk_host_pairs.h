// hsk_host_pairs.h -- host side of hsk_result_pairs, hsk_result_pairs_sliced, hsk_result_pairs_oriented and hsk_pairs_merge: read pairs that
// share k-mers, from the resident EXTENSION list (kernels: hsk_pairs.h, hsk_pairplan.h, hsk_rowmerge.h).  The slice plan, the merge of two lists, the stack of
// lists and the several-list call are templates over the rows: hsk_host_pairdiag.h uses them for the six-word rows of the diagonals.
// Part of the single translation unit hsk_api.hip (included in this order; everything here is file-local).
#pragma once

struct PairsPriv { void *host_rows = nullptr; void *dev_rows = nullptr; };
// hsk_strands (hsk_host_strand.h): one block of bit words for all tasks of the result; task t's npay[t] bits start at word word0[t]
struct StrandsPriv { u64 *bits = nullptr; std::vector<u64> word0, npay; };

// The phases of a call, summed over its slices and merges.  Every event pair is closed before the host waits, and taken behind the wait.
enum { PT_EXPAND = 0, PT_SORT, PT_REDUCE, PT_MERGE, PT_D2H, PT_N };
struct PairClock {
    PhaseTimer t; double ms[PT_N] = {0, 0, 0, 0, 0};
    explicit PairClock(hsk_ctx *c) : t(c) {}
    void take() { for (int ph = 0; ph < PT_N; ++ph) ms[ph] += t.collect(ph); }
    ~PairClock() { take(); }                             // (a call that failed: the events go back to the context)
};

// The events and the phase clock of a call; start() when there is work, finish() is the call's last wait.
struct PairCall {
    EvList ev; hipEvent_t e_start = nullptr, e_end = nullptr; PairClock ck;
    explicit PairCall(hsk_ctx *c) : ev(c), ck(c) {}
    int start(hsk_ctx *c) { e_start = ev.get(); e_end = ev.get(); HIPCHK(c, hipEventRecord(e_start, c->stream)); return HSK_OK; }
    int finish(hsk_ctx *c) { HIPCHK(c, hipEventRecord(e_end, c->stream)); HIPCHK(c, hsk_sync(c, c->stream)); ck.take(); return HSK_OK; }
    float total() const { float f = 0; return hipEventElapsedTime(&f, e_start, e_end) == hipSuccess ? f : 0; }
};

// The tasks of a range that have entries, the record count of each entry and what the count pass leaves on the device for the expansion.
struct PairRange {
    std::vector<PairTask> tk;
    u64 nent = 0, records = 0;
    PairTask *d_tasks = nullptr; u64 *d_off = nullptr, *d_loc = nullptr, *d_stat = nullptr;
};

// sp: the strand bits of the result's payload slots (hsk_result_pairs_oriented), or NULL
static int pairs_range_tasks(hsk_ctx *c, const ResultPriv *rp, int32_t task_lo, int32_t task_hi, PairRange &r, const StrandsPriv *sp = nullptr)
{
    for (int32_t t = task_lo; t < task_hi; ++t) {
        const TaskOut &to = rp->dev_tasks[t];
        if (!to.n) continue;
        if (!to.entries || !to.payoff || !to.pos || !to.rid) return fail(c, HSK_ERR_INTERNAL, "task %d of the resident result has entries but no payload arrays", t);
        if (to.npay >> PAIR_LOC_SHIFT) return fail(c, HSK_ERR_UNSUPPORTED, "task %d holds %llu payloads (2^%d at most)", t, (unsigned long long)to.npay, PAIR_LOC_SHIFT);
        PairTask p; p.entries = to.entries; p.payoff = to.payoff; p.pos = to.pos; p.rid = to.rid; p.ent_base = r.nent; p.n = to.n; p.npay = to.npay; p.pay_base = to.pay_base;
        p.strand = sp ? sp->bits + sp->word0[t] : nullptr;
        r.tk.push_back(p); r.nent += to.n;
    }
    return HSK_OK;
}

// ---- record counts: t_e per entry, exclusive 64-bit offsets, the total: once for the range, whatever follows; two waits ------------
static int pairs_count_records(hsk_ctx *c, int nw, PairRange &r, PairClock &ck)
{
    const u64 nent = r.nent, ctiles = (nent + PC_TILE - 1) / PC_TILE;
    u64 *d_ctile;
    DALLOC(c, r.d_tasks, PairTask *, r.tk.size() * sizeof(PairTask));
    DALLOC(c, r.d_off, u64 *, (nent + 1) * 8); DALLOC(c, r.d_loc, u64 *, nent * 8);
    DALLOC(c, d_ctile, u64 *, ctiles * 8); DALLOC(c, r.d_stat, u64 *, PAIR_STAT_WORDS * 8);
    ck.t.begin(PT_EXPAND);
    HIPCHK(c, hipMemcpyAsync(r.d_tasks, r.tk.data(), r.tk.size() * sizeof(PairTask), hipMemcpyHostToDevice, c->stream));     // (tk lives until the wait below)
    HIPCHK(c, hipMemsetAsync(r.d_stat, 0, PAIR_STAT_WORDS * 8, c->stream));
    PairSumArgs sa; memset(&sa, 0, sizeof sa);
    sa.tasks = r.d_tasks; sa.ntasks = (u32)r.tk.size(); sa.nw = nw; sa.nent = nent; sa.tile_sum = d_ctile; sa.off = r.d_off; sa.loc = r.d_loc; sa.err = (u32 *)(r.d_stat + PAIR_STAT_ERR);
    hipLaunchKernelGGL(pair_tsum_kernel<false>, dim3((u32)ctiles), dim3(PAIR_THREADS), 0, c->stream, sa);
    hipLaunchKernelGGL(count_scan_kernel, dim3(1), dim3(CNT_THREADS), 0, c->stream, d_ctile, ctiles, r.d_stat + PAIR_STAT_RECORDS);
    hipLaunchKernelGGL(pair_tsum_kernel<true>, dim3((u32)ctiles), dim3(PAIR_THREADS), 0, c->stream, sa);
    HIPCHK(c, hipGetLastError());
    ck.t.end(PT_EXPAND);
    u64 *st = staging(c)->read_pairs;
    HIPCHK(c, hipMemcpyAsync(st, r.d_stat, PAIR_STAT_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hsk_sync(c, c->stream));
    ck.take();
    if (st[PAIR_STAT_ERR]) return fail(c, HSK_ERR_INTERNAL, "the resident result is not a valid CSR (%s)", (st[PAIR_STAT_ERR] & PAIR_ERR_COUNT) ? "an entry's count is above 65535" : "an entry's payload slice lies outside its task's payload");
    r.records = st[PAIR_STAT_RECORDS];
    c->pool.release(d_ctile);
    return HSK_OK;
}

static void pairs_release_range(hsk_ctx *c, PairRange &r, bool stat)
{
    c->pool.release(r.d_tasks); c->pool.release(r.d_off); c->pool.release(r.d_loc); r.d_tasks = nullptr; r.d_off = r.d_loc = nullptr;
    if (stat) { c->pool.release(r.d_stat); r.d_stat = nullptr; }
}

// What every call over a task range starts with: the tasks, the call's events, the record count.  *go: there are records to expand; else
// `out` is complete (no entry in the range, or no pair among its entries) and nothing of the range is left on the device.
template <typename Out>
static int pairs_begin(hsk_ctx *c, const ResultPriv *rp, const StrandsPriv *sp, int nw, int32_t task_lo, int32_t task_hi, PairRange &r, PairCall &pc, Out *out, bool *go)
{
    *go = false;
    int rc = pairs_range_tasks(c, rp, task_lo, task_hi, r, sp); if (rc) return rc;
    if (!r.nent) return HSK_OK;
    rc = pc.start(c); if (rc) return rc;
    rc = pairs_count_records(c, nw, r, pc.ck); if (rc) return rc;
    out->records = r.records;
    if (r.records) { *go = true; return HSK_OK; }
    rc = pc.finish(c); if (rc) return rc;
    out->ms_expand = out->ms_total = pc.total();
    pairs_release_range(c, r, true);
    return HSK_OK;
}

// ---- one pass over records: the sort's ping-pong buffers, the expansion, the sort ---------------------------------------------------
struct RecordPass {
    u64 *kA = nullptr, *kB = nullptr, *vA = nullptr, *vB = nullptr;      // NW * records key words and records value words each
    u64 *keys = nullptr, *vals = nullptr;                // the sorted side
    int passes = 0;                                      // scatter passes of the sort
    void release(hsk_ctx *c) { c->pool.release(kA); c->pool.release(kB); c->pool.release(vA); c->pool.release(vB); }
};
struct PassTexts { const char *what, *need, *launch; };  // where the refusals of the two calls differ

// Keys of NW words.  expand(xtiles) enqueues the expansion into kA / vA (PT_EXPAND); `release_range`: no pass follows -- what the count
// pass left goes back as soon as the expansion is enqueued.  Then the library's key + payload radix sort over all key bits (PT_SORT);
// digits in which all records agree are skipped.  One wait (the sort's histogram).  The caller releases the buffers behind its reducer.
template <int NW, typename Expand>
static int pairs_record_pass(hsk_ctx *c, PairRange &r, u64 records, bool release_range, int32_t task_lo, int32_t task_hi, const PassTexts &tx, PairClock &ck, RecordPass &p, Expand &&expand)
{
    const u64 xtiles = (records + PX_TILE - 1) / PX_TILE;
    const bool launch = xtiles <= 0x7fffffffULL;         // (refused in front of the buffers for two-word keys, behind them for one: as each call always did)
    if (NW == 2 && !launch) return fail(c, HSK_ERR_UNSUPPORTED, "%llu records are more than one launch expands; ask for a narrower task range%s", (unsigned long long)records, tx.launch);
    // the working set, known before any of it is asked for (+ 64: as every caller of the sort sizes them)
    p.kA = (u64 *)c->pool.alloc(records * 8 * NW + 64); p.kB = (u64 *)c->pool.alloc(records * 8 * NW + 64); p.vA = (u64 *)c->pool.alloc(records * 8 + 64); p.vB = (u64 *)c->pool.alloc(records * 8 + 64);
    if (!p.kA || !p.kB || !p.vA || !p.vB)
        return fail(c, HSK_ERR_OOM, "%s of tasks [%d, %d): %llu records need %llu bytes of device memory %s", tx.what, task_lo, task_hi, (unsigned long long)records, (unsigned long long)(records * (16 * NW + 16)), tx.need);
    if (!launch) return fail(c, HSK_ERR_UNSUPPORTED, "%llu records are more than one launch expands; ask for a narrower task range%s", (unsigned long long)records, tx.launch);
    ck.t.begin(PT_EXPAND);
    int rc = expand((u32)xtiles); if (rc) return rc;
    HIPCHK(c, hipGetLastError());
    ck.t.end(PT_EXPAND);
    if (release_range) pairs_release_range(c, r, false);
    ck.t.begin(PT_SORT);
    SortScratch sc; rc = alloc_sort_scratch(c, sc); if (rc) return rc;
    rc = sort_task_device<NW>(c, p.kA, p.kB, p.vA, p.vB, records, 32 * NW, sc, &p.keys, &p.vals, false, &p.passes); if (rc) return rc;
    rc = check_device_error(c); if (rc) return rc;
    free_sort_scratch(c, sc);
    ck.t.end(PT_SORT);
    return HSK_OK;
}

// ---- count tiles, scan, read the totals, (the caller: check them, allocate the rows), emit ---------------------------------------------
// k tile arrays of ntiles words.  count(): the caller's COUNT launch, one count_scan_kernel per array -- array i's total into word
// word[i] of the caller's block d_tot -- the block's first nwords words to the staging word, ONE wait; *tot is read on the spot.
// emit(): the caller's EMIT launch (if there are rows) in the same phase, and the tile arrays go back behind it on the stream.
struct CountEmit {
    hsk_ctx *c; PairClock &ck; int phase; u64 ntiles; int k;
    u64 *tile[3] = {nullptr, nullptr, nullptr};
    CountEmit(hsk_ctx *c_, PairClock &ck_, int phase_, u64 ntiles_, int k_) : c(c_), ck(ck_), phase(phase_), ntiles(ntiles_), k(k_) {}
    template <typename Launch>
    int count(u64 *d_tot, int nwords, const int *word, const u64 **tot, Launch &&launch)
    {
        for (int i = 0; i < k; ++i) DALLOC(c, tile[i], u64 *, ntiles * 8);
        ck.t.begin(phase);
        launch();
        for (int i = 0; i < k; ++i) hipLaunchKernelGGL(count_scan_kernel, dim3(1), dim3(CNT_THREADS), 0, c->stream, tile[i], ntiles, d_tot + word[i]);      // (of all but the first, only the total is used)
        HIPCHK(c, hipGetLastError());
        ck.t.end(phase);
        u64 *st = staging(c)->read_pairs;
        HIPCHK(c, hipMemcpyAsync(st, d_tot, (size_t)nwords * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hsk_sync(c, c->stream));
        ck.take();
        *tot = st;
        return HSK_OK;
    }
    template <typename Launch>
    int emit(bool rows, Launch &&launch)
    {
        if (rows) {
            ck.t.begin(phase);
            launch();
            HIPCHK(c, hipGetLastError());
            ck.t.end(phase);
        }
        for (int i = 0; i < k; ++i) { c->pool.release(tile[i]); tile[i] = nullptr; }
        return HSK_OK;
    }
};

// a row list in HBM: a slice's, a caller's part, or a merge's
struct PairList { u64 *rows = nullptr; u64 n = 0; int level = 0; bool owned = true; };
struct PairWindow { u64 ent0, ent1, rec0, records; };   // entries [ent0, ent1) = records [rec0, rec0 + records) of the range; records > 0

// Expand a record window, sort it, reduce it to rows that stay on the device.  The whole range is the window { 0, nent, 0, records }.
// `last`: no window follows.  One wait per sort (its histogram) and one for the row count.  The window's record buffers are released
// before the routine returns.
static int pairs_window(hsk_ctx *c, PairRange &r, const PairWindow &w, bool last, bool oriented, u32 min_shared, int32_t task_lo, int32_t task_hi, PairClock &ck, hsk_pairs *acc, PairList *list)
{
    static const PassTexts tx = {"read pairs", "(two key and two value buffers) and the rows on top; ask for a narrower task range and combine the lists, or let hsk_result_pairs_sliced expand fewer records at a time",
                                 ", or let hsk_result_pairs_sliced expand fewer at a time"};
    const u64 records = w.records;
    RecordPass p;
    int rc = pairs_record_pass<1>(c, r, records, last, task_lo, task_hi, tx, ck, p, [&](u32 xtiles) -> int {
        PairExpandArgs xa; memset(&xa, 0, sizeof xa);
        xa.tasks = r.d_tasks; xa.off = r.d_off; xa.loc = r.d_loc; xa.nent = w.ent1; xa.records = records; xa.keys = p.kA; xa.vals = p.vA; xa.rec0 = w.rec0; xa.ent0 = w.ent0;
        if (w.rec0) HIPCHK(c, hipMemsetAsync(r.d_stat, 0, PAIR_STAT_WORDS * 8, c->stream));      // (self_records of the slice before)
        if (oriented) hipLaunchKernelGGL(pair_expand_kernel<true>, dim3(xtiles), dim3(PAIR_THREADS), 0, c->stream, xa);      // (bit 63 of the key: the strands' XOR)
        else hipLaunchKernelGGL(pair_expand_kernel<false>, dim3(xtiles), dim3(PAIR_THREADS), 0, c->stream, xa);
        return HSK_OK;
    });
    if (rc) return rc;
    acc->sort_passes = std::max<int32_t>(acc->sort_passes, p.passes);      // (the most over the slices)

    // ---- run reducer: rows per tile, scan, write pass ------------------------------------------------------------------------------
    const u64 rtiles = (records + PR_TILE - 1) / PR_TILE;
    PairReduceArgs ra; memset(&ra, 0, sizeof ra);
    ra.keys = p.keys; ra.vals = p.vals; ra.n = records; ra.min_shared = min_shared; ra.stats = r.d_stat;
    CountEmit ce(c, ck, PT_REDUCE, rtiles, 2);
    static const int word[2] = {PAIR_STAT_ROWS, PAIR_STAT_KEYS};
    const u64 *st;
    rc = ce.count(r.d_stat, PAIR_STAT_WORDS, word, &st, [&] {
        ra.tile_cnt = ce.tile[0]; ra.tile_keys = ce.tile[1];
        hipLaunchKernelGGL(pair_reduce_kernel<false>, dim3((u32)rtiles), dim3(PAIR_THREADS), 0, c->stream, ra);
    });
    if (rc) return rc;
    const u64 nrows = st[PAIR_STAT_ROWS];
    acc->self_records += st[PAIR_STAT_SELF]; acc->keys = st[PAIR_STAT_KEYS];
    u64 *d_rows = nullptr;
    if (nrows) { DALLOC(c, d_rows, u64 *, nrows * 32); ra.rows = d_rows; }
    rc = ce.emit(nrows != 0, [&] { hipLaunchKernelGGL(pair_reduce_kernel<true>, dim3((u32)rtiles), dim3(PAIR_THREADS), 0, c->stream, ra); });
    if (rc) return rc;
    p.release(c);
    if (last) { c->pool.release(r.d_stat); r.d_stat = nullptr; }
    list->rows = d_rows; list->n = nrows; list->level = 0; list->owned = true;
    return HSK_OK;
}

// ---- merges ------------------------------------------------------------------------------------------------------------------------
struct PairMergeStat { u64 merges = 0, merged_rows = 0; };
struct PairMergeCounts { u64 keys = 0, bins = 0; };      // of a merged list before the filter: distinct keys; rows (the six-word lists only)

// What a merge of two row lists needs to know about the rows -- their width, the tile of the merge kernel, how many tile arrays its COUNT
// pass fills (the kept rows first, then the counts before the filter) -- is the row's shape in hsk_rowmerge.h: PairRow, the four-word rows
// of the pair lists, and DiagRow, the six-word all-bins rows of the diagonals.
static_assert(PairRow::WORDS == PAIR_ROW_WORDS && DiagRow::WORDS == DIAG_ROW_WORDS, "the merge and the reducers agree on the rows");

template <typename R>
static void row_merge_launch(hsk_ctx *c, bool emit, u32 tiles, const PairList &A, const PairList &B, u32 min_count, u64 *const *tile, u64 *rows)
{
    RowMergeArgs<R> ma; memset(&ma, 0, sizeof ma);
    ma.a = A.rows; ma.na = A.n; ma.b = B.rows; ma.nb = B.n; ma.min_count = min_count; ma.rows = rows;
    for (int i = 0; i < R::NTILE; ++i) ma.tile[i] = tile[i];
    if (emit) hipLaunchKernelGGL((row_merge_kernel<R, true>), dim3(tiles), dim3(MP_THREADS), 0, c->stream, ma);
    else hipLaunchKernelGGL((row_merge_kernel<R, false>), dim3(tiles), dim3(MP_THREADS), 0, c->stream, ma);
}

// One merge (CountEmit: COUNT, the scans, EMIT) of two lists on the device into a block of its own; one wait, for the row count.  *cnt: the
// counts before the filter.  The inputs are left to the caller.
template <typename R>
static int pairs_merge_two(hsk_ctx *c, const PairList &A, const PairList &B, u32 min_shared, PairClock &ck, PairMergeStat &ms, PairList *out, PairMergeCounts *cnt)
{
    out->rows = nullptr; out->n = 0; out->owned = true; out->level = std::max(A.level, B.level) + 1;
    *cnt = PairMergeCounts();
    const u64 total = A.n + B.n;
    if (!total) return HSK_OK;
    const u64 tiles = (total + R::TILE - 1) / R::TILE;
    if (tiles > 0x7fffffffULL) return fail(c, HSK_ERR_UNSUPPORTED, "%llu rows are more than one launch merges", (unsigned long long)total);
    u64 *d_tot; DALLOC(c, d_tot, u64 *, R::NTILE * 8);
    CountEmit ce(c, ck, PT_MERGE, tiles, R::NTILE);
    static const int word[3] = {0, 1, 2};
    const u64 *st;
    int rc = ce.count(d_tot, R::NTILE, word, &st, [&] { row_merge_launch<R>(c, false, (u32)tiles, A, B, min_shared, ce.tile, nullptr); });
    if (rc) return rc;
    const u64 nrows = st[0];
    cnt->keys = st[1]; cnt->bins = R::NTILE > 2 ? st[2] : 0;       // (PairRow: the rows before the filter are its keys)
    if (nrows > total || cnt->keys > total || cnt->bins > total) return fail(c, HSK_ERR_INTERNAL, "the merge of %llu rows counted %llu", (unsigned long long)total, (unsigned long long)std::max(nrows, std::max(cnt->keys, cnt->bins)));
    if (nrows) DALLOC(c, out->rows, u64 *, nrows * R::WORDS * 8);
    rc = ce.emit(nrows != 0, [&] { row_merge_launch<R>(c, true, (u32)tiles, A, B, min_shared, ce.tile, out->rows); });
    if (rc) return rc;
    out->n = nrows;
    c->pool.release(d_tot);
    ms.merges++; ms.merged_rows += total;
    return HSK_OK;
}

// The lists of the slices (or the caller's parts) in the order of a binary counter: a list enters at level 0, and while the two lists
// on top have the same level they become one list of the next level.  A row is read by at most ceil(log2(lists)) + 1 merges, and no
// list grows by one slice at a time.  finish() merges what is left, top first; the LAST merge applies the filter and counts the list
// before it.  R: the rows (PairRow, DiagRow).  A single PairRow list's counts are known without a merge: keys = its rows.
template <typename R>
struct PairStack {
    std::vector<PairList> v;
    PairMergeStat ms;
    static void drop(hsk_ctx *c, PairList &l) { if (l.owned) c->pool.release(l.rows); l.rows = nullptr; l.n = 0; }
    int merge_top(hsk_ctx *c, u32 min_shared, bool final, PairClock &ck, PairMergeCounts *cnt)
    {
        PairList B = v.back(); v.pop_back();
        PairList A = v.back(); v.pop_back();
        PairList o;
        if (!final && (!A.n || !B.n)) {                 // nothing to join: the other list moves up as it is
            o = A.n ? A : B; o.level = std::max(A.level, B.level) + 1;
            drop(c, A.n ? B : A);
        } else {
            const int rc = pairs_merge_two<R>(c, A, B, min_shared, ck, ms, &o, cnt); if (rc) return rc;
            drop(c, A); drop(c, B);                      // (behind the merge on the stream)
        }
        v.push_back(o);
        return HSK_OK;
    }
    // `more`: lists follow (the last one is left to finish(), which knows that its merges end the list)
    int push(hsk_ctx *c, const PairList &l, bool more, PairClock &ck)
    {
        v.push_back(l);
        PairMergeCounts cnt;
        while (more && v.size() >= 2 && v[v.size() - 1].level == v[v.size() - 2].level) { const int rc = merge_top(c, 1, false, ck, &cnt); if (rc) return rc; }
        return HSK_OK;
    }
    int finish(hsk_ctx *c, u32 min_shared, PairClock &ck, PairList *fin, PairMergeCounts *cnt)
    {
        *fin = PairList(); *cnt = PairMergeCounts();
        if (v.empty()) return HSK_OK;
        if (v.size() == 1) {
            if ((min_shared > 1 || R::COUNT_ONE) && v[0].n) v.push_back(PairList());      // one list: the filter (and the count) is a merge with nothing
            else { *fin = v[0]; cnt->keys = v[0].n; v.clear(); return HSK_OK; }
        }
        while (v.size() > 1) { const int rc = merge_top(c, v.size() == 2 ? min_shared : 1, v.size() == 2, ck, cnt); if (rc) return rc; }
        *fin = v[0]; v.clear();
        return HSK_OK;
    }
};

// ---- egress: the final list (rows of row_bytes bytes) to pinned host memory, or left on the device in a block the result owns; the
// call's last wait.  pp holds the two pointers; pairs_store() puts them and the call's times into the ABI struct.
static int pairs_egress(hsk_ctx *c, PairList &fin, u64 row_bytes, bool on_device, PairCall &pc, PairsPriv *pp)
{
    const u64 bytes = fin.n * row_bytes;
    u64 *d_rows = fin.rows;
    if (bytes && !on_device) {
        pp->host_rows = c->hpool.alloc(bytes);
        if (!pp->host_rows) return fail(c, HSK_ERR_OOM, "pinned host allocation of %llu bytes failed", (unsigned long long)bytes);
        pc.ck.t.begin(PT_D2H);
        HIPCHK(c, hipMemcpyAsync(pp->host_rows, d_rows, bytes, hipMemcpyDeviceToHost, c->stream));
        pc.ck.t.end(PT_D2H);
        c->stats.d2h_bytes += bytes;
    } else if (bytes && !fin.owned) {                    // a caller's list that came through hsk_pairs_merge as it is: the result gets a copy of its own
        u64 *cp; DALLOC(c, cp, u64 *, bytes);
        HIPCHK(c, hipMemcpyAsync(cp, d_rows, bytes, hipMemcpyDeviceToDevice, c->stream));
        d_rows = cp; fin.owned = true;
    }
    const int rc = pc.finish(c); if (rc) return rc;
    if (!bytes || !on_device) { if (fin.owned) c->pool.release(d_rows); d_rows = nullptr; }
    fin.rows = nullptr;
    pp->dev_rows = d_rows;
    return HSK_OK;
}

template <typename Out>
static void pairs_store(Out *out, u64 nrows, const PairsPriv *pp, const PairCall &pc)
{
    out->n = nrows; out->rows = (uint64_t *)pp->host_rows; out->rows_dev = pp->dev_rows;
    out->ms_expand = pc.ck.ms[PT_EXPAND]; out->ms_sort = pc.ck.ms[PT_SORT]; out->ms_reduce = pc.ck.ms[PT_REDUCE]; out->ms_d2h = pc.ck.ms[PT_D2H];
    out->ms_total = pc.total();
}

// What hsk_result_pairs_sliced expands at a time when the caller leaves it to the library (include/hsk.h): 1/96 of the device memory the
// context can still get -- what the runtime reports free plus what the context's pool holds unused -- in records: a third of it for the
// 32 bytes a record takes, the rest for the row lists and the merges.
// `bytes`: what a record takes while its slice is sorted (32 here; 48 for the two-word keys of hsk_result_pair_diagonals_sliced: 1/144).
static u64 pairs_auto_budget(hsk_ctx *c, u64 bytes = 32)
{
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); fr = 0; }
    const u64 b = ((u64)fr + c->pool.bytes_cached) / (3 * bytes);
    return b ? b : 1;
}

// The plan of a sliced call: every cut of the range's entries under the budget and the record offset at it, in one launch and one wait
// (one lane cuts the whole range on the device, pair_plan_kernel: reading a cut back per slice would wait once per slice).  win: the
// slices that hold records (a run of entries without any in front of a large entry is none), in the order of the entries.
static int pairs_plan_windows(hsk_ctx *c, const PairRange &r, u64 budget, std::vector<PairWindow> &win)
{
    const u64 records = r.records;
    const u64 cap = pair_plan_max_slices(r.nent, records, budget);
    u64 *d_cut; DALLOC(c, d_cut, u64 *, (2 * cap + 1) * 8);
    PairPlanArgs pa; memset(&pa, 0, sizeof pa);
    pa.off = r.d_off; pa.nent = r.nent; pa.max_records = budget; pa.cut = d_cut; pa.cap = cap; pa.ncut = d_cut + 2 * cap;
    hipLaunchKernelGGL(pair_plan_kernel, dim3(1), dim3(1), 0, c->stream, pa);
    HIPCHK(c, hipGetLastError());
    std::vector<u64> cut(2 * cap + 1);
    HIPCHK(c, hipMemcpyAsync(cut.data(), d_cut, cut.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hsk_sync(c, c->stream));
    c->pool.release(d_cut);
    const u64 ncut = cut[2 * cap];
    if (ncut == 0 || ncut > cap || cut[2 * (ncut - 1)] != r.nent || cut[2 * (ncut - 1) + 1] != records)
        return fail(c, HSK_ERR_INTERNAL, "the slice plan of %llu entries does not end at the last one", (unsigned long long)r.nent);
    u64 e0 = 0, r0 = 0;
    for (u64 i = 0; i < ncut; ++i) {
        const u64 e1 = cut[2 * i], r1 = cut[2 * i + 1];
        if (e1 <= e0 || r1 < r0) return fail(c, HSK_ERR_INTERNAL, "the slice plan does not advance at entry %llu", (unsigned long long)e0);
        if (r1 > r0) { const PairWindow w = {e0, e1, r0, r1 - r0}; win.push_back(w); }
        e0 = e1; r0 = r1;
    }
    return HSK_OK;
}

// The tasks of the range go through ONE launch per kernel over a device table of task descriptors (at most HSK_MAX_TASKS of them).
// sliced == false (hsk_result_pairs): the records of the whole range are one array, sorted once.  Two waits before the large buffers exist
// (the record count), one per sort (its histogram), one for the row count, one at the end.
// sliced == true (hsk_result_pairs_sliced): the same while the records fit the budget; else one more wait for the plan -- one lane cuts the
// whole range on the device (pair_plan_kernel), since reading a cut back per slice would wait once per slice -- then every slice is a window
// of its own, and the lists meet on a PairStack: one wait per merge, for its row count.
static int pairs_impl(hsk_ctx *c, const ResultPriv *rp, const StrandsPriv *sp, int nw, int32_t task_lo, int32_t task_hi, u32 min_shared, bool on_device, bool sliced, u64 max_records,
                      hsk_pairs *out, hsk_pairs_slices *info, PairsPriv *pp)
{
    PairRange r; PairCall pc(c); bool go;
    PairClock &ck = pc.ck;
    const bool oriented = sp != nullptr;               // (hsk_result_pairs_oriented: only the key of a record differs)
    info->slices = 1;
    int rc = pairs_begin(c, rp, sp, nw, task_lo, task_hi, r, pc, out, &go); if (rc || !go) return rc;
    const u64 records = r.records;
    u64 budget = records;
    if (sliced) budget = max_records ? max_records : pairs_auto_budget(c);
    PairList fin;
    if (budget >= records) {
        const PairWindow w = {0, r.nent, 0, records};
        rc = pairs_window(c, r, w, true, oriented, min_shared, task_lo, task_hi, ck, out, &fin); if (rc) return rc;
        info->peak_records = records;
    } else {
        std::vector<PairWindow> win;
        rc = pairs_plan_windows(c, r, budget, win); if (rc) return rc;
        PairStack<PairRow> stk;
        hsk_pairs acc; memset(&acc, 0, sizeof acc);
        for (size_t i = 0; i < win.size(); ++i) {
            const bool last = i + 1 == win.size();
            PairList l;
            rc = pairs_window(c, r, win[i], last, oriented, 1, task_lo, task_hi, ck, &acc, &l); if (rc) return rc;
            info->peak_records = std::max<u64>(info->peak_records, win[i].records);
            rc = stk.push(c, l, !last, ck); if (rc) return rc;
        }
        PairMergeCounts cnt;
        rc = stk.finish(c, min_shared, ck, &fin, &cnt); if (rc) return rc;
        out->self_records = acc.self_records; out->sort_passes = acc.sort_passes; out->keys = cnt.keys;
        info->slices = win.size(); info->merges = stk.ms.merges; info->merged_rows = stk.ms.merged_rows;
    }
    rc = pairs_egress(c, fin, 32, on_device, pc, pp); if (rc) return rc;
    pairs_store(out, fin.n, pp, pc);
    info->ms_merge = ck.ms[PT_MERGE];
    return HSK_OK;
}

// What every call that reads a resident EXTENSION result checks before it opens its scope; *rpo: the result's private part.
static int pairs_check_resident(hsk_ctx *c, const hsk_result *res, const char *name, const ResultPriv **rpo)
{
    if (!c->cfg.extension) return fail(c, HSK_ERR_INVALID_ARG, "%s needs a context with EXTENSION: without it the list carries no (ReadId, PosInRead)", name);
    const ResultPriv *rp = (const ResultPriv *)res->priv;
    if (!(c->cfg.flags & HSK_FLAG_KEEP_DEVICE) || !rp || res->ntasks <= 0 || rp->dev_tasks.size() != (size_t)res->ntasks)
        return fail(c, HSK_ERR_INVALID_ARG, "%s needs a result that was left on the device (HSK_FLAG_KEEP_DEVICE)", name);
    *rpo = rp;
    return HSK_OK;
}

// ... and a task range of it, with or without the strands of its payload slots (*spo NULL without)
static int pairs_check_args(hsk_ctx *c, const hsk_result *res, const hsk_strands *strands, int32_t task_lo, int32_t task_hi, const char *name, const ResultPriv **rpo, const StrandsPriv **spo)
{
    const ResultPriv *rp;
    const int rc = pairs_check_resident(c, res, name, &rp); if (rc) return rc;
    if (task_lo < 0 || task_hi < task_lo || task_hi > res->ntasks) return fail(c, HSK_ERR_INVALID_ARG, "task range [%d, %d) outside [0, %d]", task_lo, task_hi, res->ntasks);
    const StrandsPriv *sp = strands ? (const StrandsPriv *)strands->priv : nullptr;
    if (strands) {                                        // do the bits belong to this result?
        if (!sp || strands->ntasks != res->ntasks || sp->npay.size() != (size_t)res->ntasks)
            return fail(c, HSK_ERR_INVALID_ARG, "%s: the strands are of %d tasks, the result has %d", name, sp ? strands->ntasks : 0, res->ntasks);
        for (int32_t t = 0; t < res->ntasks; ++t)
            if (sp->npay[t] != rp->dev_tasks[t].npay)
                return fail(c, HSK_ERR_INVALID_ARG, "%s: the strands do not belong to this result (task %d: %llu payload slots, the result has %llu)", name, t,
                            (unsigned long long)sp->npay[t], (unsigned long long)rp->dev_tasks[t].npay);
    }
    *rpo = rp; *spo = sp;
    return HSK_OK;
}

// A call that returns a row list: the list's private part, the call's scope (ApiCall), and nothing left behind when it fails.
template <typename Out, typename Impl>
static int pairs_api_call(hsk_ctx *c, const char *name, Out *out, Impl &&impl)
{
    PairsPriv *pp = new PairsPriv();
    const int rc = ApiCall(c, name).run([&] { return impl(pp); });
    if (rc != HSK_OK) {                                   // (the device blocks went back with the call's rollback)
        if (pp->host_rows) c->hpool.release(pp->host_rows);
        delete pp;
        memset(out, 0, sizeof *out);
        return rc;
    }
    out->priv = pp;
    return HSK_OK;
}

static void pairs_priv_free(hsk_ctx *c, void *priv)
{
    PairsPriv *pp = (PairsPriv *)priv;
    if (!pp) return;
    if (c) { if (pp->host_rows) c->hpool.release(pp->host_rows); c->pool.release(pp->dev_rows); }
    else if (pp->host_rows) (void)hipHostFree(pp->host_rows);
    delete pp;
}

static int pairs_entry(hsk_ctx *c, const hsk_result *res, const hsk_strands *strands, int32_t task_lo, int32_t task_hi, uint32_t min_shared, int32_t on_device, bool sliced, uint64_t max_records,
                       hsk_pairs *out, hsk_pairs_slices *info, const char *name)
{
    if (!c || !res || !out) return HSK_ERR_INVALID_ARG;
    memset(out, 0, sizeof *out);
    hsk_pairs_slices local; if (!info) info = &local;
    memset(info, 0, sizeof *info);
    const ResultPriv *rp; const StrandsPriv *sp;
    const int chk = pairs_check_args(c, res, strands, task_lo, task_hi, name, &rp, &sp); if (chk) return chk;
    if (min_shared == 0) return fail(c, HSK_ERR_INVALID_ARG, "min_shared must be at least 1");
    const int rc = pairs_api_call(c, name, out, [&](PairsPriv *pp) { return pairs_impl(c, rp, sp, res->nw, task_lo, task_hi, min_shared, on_device != 0, sliced, max_records, out, info, pp); });
    if (rc != HSK_OK) memset(info, 0, sizeof *info);
    return rc;
}

extern "C" int hsk_result_pairs(hsk_ctx *c, const hsk_result *res, int32_t task_lo, int32_t task_hi, uint32_t min_shared, int32_t on_device, hsk_pairs *out)
{
    return pairs_entry(c, res, nullptr, task_lo, task_hi, min_shared, on_device, false, 0, out, nullptr, "hsk_result_pairs");
}

extern "C" int hsk_result_pairs_sliced(hsk_ctx *c, const hsk_result *res, int32_t task_lo, int32_t task_hi, uint32_t min_shared, int32_t on_device, uint64_t max_records,
                                       hsk_pairs *out, hsk_pairs_slices *info)
{
    return pairs_entry(c, res, nullptr, task_lo, task_hi, min_shared, on_device, true, max_records, out, info, "hsk_result_pairs_sliced");
}

// hsk_result_pairs_sliced with the relative strand of the two occurrences in bit 63 of every record's key: the sort, the reducer, the
// slices and the merges see a key like any other
extern "C" int hsk_result_pairs_oriented(hsk_ctx *c, const hsk_result *res, const hsk_strands *strands, int32_t task_lo, int32_t task_hi, uint32_t min_shared,
                                         int32_t on_device, uint64_t max_records, hsk_pairs *out, hsk_pairs_slices *info)
{
    if (!strands) { if (c && out) memset(out, 0, sizeof *out); return c ? fail(c, HSK_ERR_INVALID_ARG, "hsk_result_pairs_oriented: strands is NULL") : HSK_ERR_INVALID_ARG; }
    return pairs_entry(c, res, strands, task_lo, task_hi, min_shared, on_device, true, max_records, out, info, "hsk_result_pairs_oriented");
}

// The several-list contract on the GPU: host lists go up, device lists are read where they are, and all meet on a PairStack.  Part: the
// ABI struct of the lists (hsk_pairs, hsk_pair_diags); out gets the sums of records and self_records.
template <typename R, typename Part>
static int pairs_stack_parts(hsk_ctx *c, const Part *const *parts, int32_t nparts, PairClock &ck, PairStack<R> &stk, Part *out)
{
    int32_t last = -1;
    for (int32_t i = 0; i < nparts; ++i) { out->records += parts[i]->records; out->self_records += parts[i]->self_records; if (parts[i]->n) last = i; }
    for (int32_t i = 0; i <= last; ++i) {
        const Part *p = parts[i];
        if (!p->n) continue;
        PairList l; l.n = p->n;
        if (p->rows_dev) { l.rows = (u64 *)p->rows_dev; l.owned = false; }
        else {
            DALLOC(c, l.rows, u64 *, p->n * R::WORDS * 8);
            HIPCHK(c, hipMemcpyAsync(l.rows, p->rows, p->n * R::WORDS * 8, hipMemcpyHostToDevice, c->stream));      // (pageable or pinned: the part outlives the call's last wait)
            c->stats.h2d_bytes += p->n * R::WORDS * 8;
        }
        const int rc = stk.push(c, l, i != last, ck); if (rc) return rc;
    }
    return HSK_OK;
}

static int pairs_merge_impl(hsk_ctx *c, const hsk_pairs *const *parts, int32_t nparts, u32 min_shared, bool on_device, hsk_pairs *out, PairsPriv *pp)
{
    PairCall pc(c);
    PairClock &ck = pc.ck;
    int rc = pc.start(c); if (rc) return rc;
    PairStack<PairRow> stk;
    rc = pairs_stack_parts(c, parts, nparts, ck, stk, out); if (rc) return rc;
    PairList fin; PairMergeCounts cnt;
    rc = stk.finish(c, min_shared, ck, &fin, &cnt); if (rc) return rc;
    out->keys = cnt.keys;
    rc = pairs_egress(c, fin, 32, on_device, pc, pp); if (rc) return rc;
    pairs_store(out, fin.n, pp, pc);
    out->ms_reduce = ck.ms[PT_MERGE];                    // (the merges are this call's reduction)
    return HSK_OK;
}

// what a merge call refuses about its parts (`min_name`: what the call names its filter)
template <typename Part>
static int pairs_merge_check(hsk_ctx *c, const char *name, const Part *const *parts, int32_t nparts, uint32_t min_rows, const char *min_name)
{
    if (nparts < 0) return fail(c, HSK_ERR_INVALID_ARG, "%s: %d parts", name, nparts);
    if (nparts > 0 && !parts) return fail(c, HSK_ERR_INVALID_ARG, "%s: %d parts and no array of them", name, nparts);
    if (min_rows == 0) return fail(c, HSK_ERR_INVALID_ARG, "%s must be at least 1", min_name);
    for (int32_t i = 0; i < nparts; ++i) {
        if (!parts[i]) return fail(c, HSK_ERR_INVALID_ARG, "%s: part %d is NULL", name, i);
        if (parts[i]->n && !parts[i]->rows_dev && !parts[i]->rows) return fail(c, HSK_ERR_INVALID_ARG, "%s: part %d has %llu rows and neither rows nor rows_dev", name, i, (unsigned long long)parts[i]->n);
        if (parts[i]->n && ((uintptr_t)parts[i]->rows_dev & 15)) return fail(c, HSK_ERR_INVALID_ARG, "%s: rows_dev of part %d is not 16-byte aligned", name, i);
        if (parts[i]->n >> 58) return fail(c, HSK_ERR_INVALID_ARG, "%s: part %d claims %llu rows", name, i, (unsigned long long)parts[i]->n);
    }
    return HSK_OK;
}

extern "C" int hsk_pairs_merge(hsk_ctx *c, const hsk_pairs *const *parts, int32_t nparts, uint32_t min_shared, int32_t on_device, hsk_pairs *out)
{
    if (!c || !out) return HSK_ERR_INVALID_ARG;
    memset(out, 0, sizeof *out);
    const int chk = pairs_merge_check(c, "hsk_pairs_merge", parts, nparts, min_shared, "min_shared"); if (chk) return chk;
    return pairs_api_call(c, "hsk_pairs_merge", out, [&](PairsPriv *pp) { return pairs_merge_impl(c, parts, nparts, min_shared, on_device != 0, out, pp); });
}

extern "C" void hsk_pairs_free(hsk_ctx *c, hsk_pairs *p)
{
    if (!p) return;
    pairs_priv_free(c, p->priv);
    memset(p, 0, sizeof *p);
}
