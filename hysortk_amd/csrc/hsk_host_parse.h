// hsk_host_parse.h -- host side of the parse stage (kernels: hsk_parse.h; tiling and capacities: hsk_parseplan.h).  The supermer store; what
// both drivers share -- the scan's buffers (ScanBufs), the verdict words (ParseFlags), launch_scan / launch_place, the slab copies; and the
// drivers: parse_count (fast scan, verdict, general count) + parse_place, and parse_ingest_pipelined for hsk_count() from pinned memory.
// Part of the single translation unit hsk_api.hip (included in this order; everything here is file-local).
#pragma once

// ------------------------------------------------------------------------------------------------
// stage: parse (a4, a5, a6)
// ------------------------------------------------------------------------------------------------
// where the bases of a task's supermers live
struct BaseSource {
    const u64 *src8 = nullptr; u64 bit0 = 0; u64 nwords = 0;   // byte stream rounded down to 8 bytes
    const u64 *gpos = nullptr;                                  // reference mode positions (null: prefix-sum byte offsets)
    const u32 *boff = nullptr;                                  // byte-store mode: supermer s starts at byte seg.byte_off + boff[s] of the stream
    const void *bitems = nullptr; u32 n_bitems = 0;             // item mode with scan-placed bins: the bucket order's work list (BucketItem[], one per chunk), built on the device
    const u32 *sub = nullptr; const u64 *item = nullptr;        // item mode (combining extraction): minimizer bits and the two item words of every supermer (SupermerStore::sm_sub / sm_item); nothing else
};
static bool reads_in_place(const BaseSource &b) { return b.gpos != nullptr || b.boff != nullptr; }   // no prefix sums needed to find a supermer's bases
static BaseSource source_from_packed(const u8 *d_packed, u64 packed_bytes, const u64 *gpos)
{
    BaseSource b; const uintptr_t p = (uintptr_t)d_packed;
    b.src8 = (const u64 *)(p & ~(uintptr_t)7); b.bit0 = 8 * (u64)(p & 7); b.nwords = ((p & 7) + packed_bytes + 7) / 8; b.gpos = gpos;
    return b;
}
static BaseSource source_from_bytes(const u8 *bytes, u64 nbytes)
{
    BaseSource b; b.src8 = (const u64 *)bytes; b.bit0 = 0; b.nwords = (nbytes + 7) / 8 + 1; b.gpos = nullptr;   // pool blocks are padded
    return b;
}

struct SupermerStore {
    u32 ntasks = 0, nblocks = 0;
    u8 *sm_len = nullptr; u8 *sm_bytes = nullptr; u64 *sm_gpos = nullptr; u32 *sm_pos = nullptr; int32_t *sm_rid = nullptr;
    u32 *sm_boff = nullptr;       // byte-store mode (place_bytes_kernel): sm_bytes is complete, sm_boff[slot] = offset inside the task's byte run
    void *d_bitems = nullptr; u32 n_bitems = 0; void *bin_aux[4] = {nullptr, nullptr, nullptr, nullptr};      // scan-placed bins: work list + cursor / map / control / chunk owners (released with the store)
    bool bytes_done = false;      // place_bytes_kernel has written sm_bytes (supermers that travel: without sm_boff -- the receiver scans the lengths anyway)
    unsigned short *sm_sub16 = nullptr;   // several ranks, combining extraction on the owner's side: the top 16 minimizer bits of every supermer (they travel with sm_len)
    u32 *sm_sub = nullptr;        // combining extraction (hsk_combine.h): 32 mixed bits of the supermer's minimizer hash ...
    u64 *sm_item = nullptr;       // ... and the supermer itself (place_items_kernel); sm_len / sm_gpos do not exist in this mode
    u64 tot_sup = 0, tot_bytes = 0, tot_kmers = 0;
    std::vector<u64> task_tot;    // [ntasks][3] supermers, bytes, kmers
    std::vector<u64> task_base;   // [ntasks][3] slot, byte, kmer bases (tasks stored in `order`)
    std::vector<u32> order;       // storage order of tasks (grouped by owner rank, ascending id)
    BaseSource base;              // multi-GPU: where pack_kernel reads the bases from (the rank's packed reads)
    std::vector<char> group_packed;  // multi-GPU, grouped exchange: sm_bytes of task group g have been produced
};

static void free_store(hsk_ctx *c, SupermerStore &s)
{
    c->pool.release(s.sm_sub16); s.sm_sub16 = nullptr;
    c->pool.release(s.d_bitems); s.d_bitems = nullptr; s.n_bitems = 0; for (void *&p : s.bin_aux) { c->pool.release(p); p = nullptr; }
    c->pool.release(s.sm_len); c->pool.release(s.sm_bytes); c->pool.release(s.sm_gpos); c->pool.release(s.sm_pos); c->pool.release(s.sm_rid); c->pool.release(s.sm_boff); c->pool.release(s.sm_sub); s.sm_sub = nullptr; c->pool.release(s.sm_item); s.sm_item = nullptr;
    s.sm_len = s.sm_bytes = nullptr; s.sm_gpos = nullptr; s.sm_pos = nullptr; s.sm_rid = nullptr; s.sm_boff = nullptr;
}

// where the extraction finds the bases of the store's supermers: the store's own byte runs, or (position mode) the packed reads
static BaseSource source_from_store(const SupermerStore &st, const u8 *d_packed, u64 packed_bytes)
{
    if (!st.sm_boff) { BaseSource b = source_from_packed(d_packed, packed_bytes, st.sm_gpos); b.sub = st.sm_sub; b.item = st.sm_item; b.bitems = st.d_bitems; b.n_bitems = st.n_bitems; return b; }
    BaseSource b = source_from_bytes(st.sm_bytes, st.tot_bytes);
    b.boff = st.sm_boff;
    return b;
}

// Byte-store placement or position placement?  Measured on 10 Gbp (one GPU): the byte store cuts the extraction's fetch
// traffic from ~6.5x to ~1x its algorithmic read bytes, but the extraction does not get faster (38.3 against 37.6 ms: it is
// bound by its chain of dependent phases, not by bandwidth) while the placement pays for the extra stores (12.8 against
// 8.4 ms).  With several GPUs the bytes must be produced anyway (they are what travels), and writing them here replaces
// pack_kernel's scattered gather (~20 ms per rank and step).  So: byte store when the supermers travel, positions when
// they stay; tuning "place_bytes=0" / "=1" forces either.
static bool place_bytes_enabled(const hsk_ctx *c, bool supermers_travel)
{
    const int forced = (int)c->tune.place_bytes;
    return forced < 0 ? supermers_travel : forced != 0;
}

// this call's tiling (hsk_parseplan.h); nslabs > 1: the slab ingest wants that many slabs
static ParseTiling call_tiling(hsk_ctx *c, u64 packed_bytes, u32 nslabs = 1) { return parse_tiling(packed_bytes, c->call.scan_blocks, nslabs); }
// the tiling and the call's constants as the kernels take them (t.nslabs > 1: scan_kernel and the three placement kernels only, see ParseArgs)
static ParseArgs make_parse_args(hsk_ctx *c, const ParseTiling &t, const u8 *d_packed, u64 packed_bytes, const u64 *d_roff, const u32 *d_rlen,
                                 u64 nreads, int64_t rid_base, u32 ntasks)
{
    ParseArgs a; memset(&a, 0, sizeof a);
    a.packed = d_packed; a.packed_bytes = packed_bytes; a.roff = d_roff; a.rlen = d_rlen; a.nreads = nreads;
    a.k = c->cfg.kmer_size; a.m = c->cfg.minimizer_size; a.ntasks = ntasks; a.fm = make_fastmod(ntasks >> c->call.vt_shift); a.vt_shift = c->call.vt_shift;      // (virtual tasks: `ntasks` counts them)
    a.item_maxk = (u32)std::max(1, std::min(16, 61 - c->cfg.kmer_size));
    a.rid_base = rid_base;
    a.ntiles = t.ntiles; a.tiles_per_block = t.tiles_per_block; a.nslabs = t.nslabs; a.slab = 0; a.slab_tiles = t.slab_tiles;
    return a;
}

// The parse in two steps, so that a caller that needs the task sizes before it can fix the storage order
// (multi-GPU: sizes -> all-reduce -> dispatcher -> owner-grouped order) hashes the reads only once:
//   parse_count: minimizers + supermer boundaries of every tile; per-(workgroup, task) counts; task totals
//   parse_place: exclusive scan of the counts in the storage order `order`, supermers to their slots
// Fast path = scan_kernel + a placement kernel (compact supermer records kept in between); the general path
// (M > 25, or a tile with more supermers than the record capacity) = parse_kernel<COUNT> + emit_kernel.
// scan_kernel places the items of the combining extraction itself (one GPU; ParseArgs::bin_*, hsk_parse.h: bin_place): bins = (XCD, virtual
// task) chunk lists.  The chunk store is sized from the EXPECTED supermer count (a window of W k-mers starts a supermer every (W + 1) / 2
// positions on random sequence, every 16 k-mers at least, once per read) with a quarter to spare; real genomes with long low-complexity
// stretches make FEWER supermers, and an input that does overrun it (error bit 128; a bin beyond its map: 256) sends the call round again
// without the combining extraction.  tuning "scan_place=1" selects it (default: tile records + the item placement, see below).
struct ScanBins {
    u32 *cursor = nullptr, *map = nullptr, *ctl = nullptr, *chunk_bin = nullptr, *subs = nullptr; ulonglong2 *items = nullptr;
    BinTable *d_table = nullptr;                          // the table scan_kernel<.., true> reads (ParseArgs::bins)
    u32 vmax = 0, cap = 0, nchunks = 0, nbins = 0;
};
// Measured (10 Gbp, round 4): scan 47.6 ms with the items placed by it against 33.9 + 13.4 ms (scan + item placement): the same ~13.5 ms wherever the
// placement runs, 101.7 ms per step either way -- and from host memory the separate placement hides behind the ingest's DMA while the longer scan
// does not (140 against 123 ms).  So the default stays the placement kernel; "scan_place=1" takes the fused form (no tile records: 13 GB less device
// memory and 20 GB less traffic per 10 Gbp).
static void bins_release(hsk_ctx *c, ScanBins &b)
{
    c->pool.release(b.cursor); c->pool.release(b.map); c->pool.release(b.ctl); c->pool.release(b.chunk_bin); c->pool.release(b.subs); c->pool.release(b.items); c->pool.release(b.d_table);
    b = ScanBins();
}
static int bins_alloc(hsk_ctx *c, ScanBins &b, u32 nvt, u64 packed_bytes, u64 nreads, int W, hipStream_t stream)
{
    b = ScanBins();
    const double positions = (double)packed_bytes * 4.0;
    const double maxk = (double)std::max(1, std::min(16, 61 - c->cfg.kmer_size));      // k-mers per item at most (ParseArgs::item_maxk)
    const double expect = positions * std::max(2.2 / (double)(W + 1), 1.2 / maxk) + 2.0 * (double)nreads + 65536.0;
    b.nbins = 8u * nvt;
    if (b.nbins > 8192) return fail(c, HSK_ERR_UNSUPPORTED, "more than 8192 bins");      // (a chunk's owner word: 13 bits of bin)
    const long long pct = c->tune.bin_cap_pct;
    const u64 cap = (u64)(expect * (double)pct / 100.0 / BIN_CHUNK) + (pct >= 100 ? 2 * b.nbins + 64 : b.nbins + 1);      // (+ a first chunk and a chunk opened ahead per bin)      // (tests: a store that runs out)
    if (cap >= 0xFFFFFFF0ULL) return fail(c, HSK_ERR_UNSUPPORTED, "item store of %llu chunks", (unsigned long long)cap);
    b.cap = (u32)cap;
    b.vmax = (u32)std::min<u64>(std::max<u64>(cap / b.nbins * 64, 256), 1u << 16);
    if (const long long vmax = c->tune.bin_vmax; vmax > 0) b.vmax = (u32)vmax;                               // (tests: a bin beyond its map)
    DALLOC(c, b.cursor, u32 *, (size_t)b.nbins * 4 * BIN_CUR_STRIDE);
    DALLOC(c, b.map, u32 *, (size_t)b.nbins * b.vmax * 4);
    DALLOC(c, b.ctl, u32 *, 256);
    DALLOC(c, b.chunk_bin, u32 *, (size_t)b.cap * 4 + 64);
    DALLOC(c, b.items, ulonglong2 *, (size_t)b.cap * BIN_CHUNK * 16 + 64);
    DALLOC(c, b.subs, u32 *, (size_t)b.cap * BIN_CHUNK * 4 + 64);
    HIPCHK(c, hipMemsetAsync(b.cursor, 0, (size_t)b.nbins * 4 * BIN_CUR_STRIDE, stream));
    HIPCHK(c, hipMemsetAsync(b.map, 0, (size_t)b.nbins * b.vmax * 4, stream));
    HIPCHK(c, hipMemsetAsync(b.ctl, 0, 256, stream));
    DALLOC(c, b.d_table, BinTable *, 256);
    BinTable *h = (BinTable *)((char *)c->pinned + (384u << 10));      // (pinned staging: the copy is asynchronous)
    h->cursor = b.cursor; h->map = b.map; h->vmax = b.vmax; h->cap_chunks = b.cap; h->ctl = b.ctl; h->chunk_bin = b.chunk_bin; h->items = b.items; h->subs = b.subs; h->err = c->d_err;
    HIPCHK(c, hipMemcpyAsync(b.d_table, h, sizeof(BinTable), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(bins_init_kernel, dim3((b.nbins + 255) / 256), dim3(256), 0, stream, *h, b.nbins);
    return HSK_OK;
}
// the store takes the bins over: items and minimizer bits where they are, the bucket order's work list from the chunk lists
static int bins_to_store(hsk_ctx *c, ScanBins &b, SupermerStore &st, u32 nvt, u32 vt_shift, hipStream_t stream);

// What the fast scan writes besides the COUNT matrix.  Both drivers (parse_count, parse_ingest_pipelined) own one: scan_setup decides
// what the call needs, allocates, clears and names it in the kernels' arguments; scan_release gives it back.
struct ScanBufs {
    u32 *d_overflow = nullptr;                            // set by a tile with more supermers than the record capacity
    u32 *d_tile_rec = nullptr, *d_tile_nrec = nullptr;    // the tiles' supermer records, kept for the placement ...
    ScanBins bins;                                        // ... or no records at all: scan_kernel places the items itself
    u32 *d_tile_r0 = nullptr;                             // EXTENSION: first read of every tile (hint for the (pos, rid) lookup)
    u32 *d_tile_sub = nullptr;                            // combining extraction: minimizer bits of every record
    unsigned long long *d_dropped = nullptr;              // scan_kernel<.., DROP>: positions left out (CallState::drop_mask_now)
};
static void scan_release(hsk_ctx *c, ScanBufs &s)
{
    c->pool.release(s.d_overflow); c->pool.release(s.d_tile_rec); c->pool.release(s.d_tile_nrec); c->pool.release(s.d_tile_r0); c->pool.release(s.d_tile_sub); c->pool.release(s.d_dropped);
    bins_release(c, s.bins);
    s = ScanBufs();
}
static int scan_setup(hsk_ctx *c, ScanBufs &s, ParseArgs &a, hipStream_t stream)
{
    const int W = c->cfg.kmer_size - c->cfg.minimizer_size + 1;
    a.rec_cap = parse_rec_cap(W, c->tune.parse_rec_cap);
    a.place_group = place_group(PLACE_RECORDS, a.rec_cap);               // (launch_place: each kind's own)
    const bool items = c->call.combine_now && a.rec_cap <= PLACE_ITEM_REC;
    const bool bins = items && c->call.item_mode_now && c->tune.scan_place != 0;
    DALLOC(c, s.d_overflow, u32 *, 256);
    HIPCHK(c, hipMemsetAsync(s.d_overflow, 0, 4, stream));
    a.overflow = s.d_overflow;
    if (bins) {
        int brc = bins_alloc(c, s.bins, a.ntasks, a.packed_bytes, a.nreads, W, stream); if (brc) return brc;
        a.bins = s.bins.d_table;
    } else {
        DALLOC(c, s.d_tile_rec, u32 *, (size_t)a.ntiles * a.rec_cap * 4 + 64);
        DALLOC(c, s.d_tile_nrec, u32 *, (size_t)a.ntiles * 4 + 64);
        a.tile_rec = s.d_tile_rec; a.tile_nrec = s.d_tile_nrec;
    }
    if (c->cfg.extension && a.nreads < (1ULL << 32)) { DALLOC(c, s.d_tile_r0, u32 *, (size_t)a.ntiles * 4 + 64); a.tile_r0 = s.d_tile_r0; }
    if (items && !bins) { DALLOC(c, s.d_tile_sub, u32 *, (size_t)a.ntiles * a.rec_cap * 4 + 64); a.tile_sub = s.d_tile_sub; }
    c->call.dropped_now = 0;
    a.drop_mask = bins ? 0u : c->call.drop_mask_now;
    if (a.drop_mask) { DALLOC(c, s.d_dropped, unsigned long long *, 256); HIPCHK(c, hipMemsetAsync(s.d_dropped, 0, 8, stream)); a.dropped = s.d_dropped; }
    return HSK_OK;
}

struct ParseJob {
    ParseArgs a; u32 nblocks = 0, ntasks = 0; bool fast = false, empty = true;
    const u64 *d_roff = nullptr; u64 nreads = 0; int64_t rid_base = 0;
    u64 *d_blk_cnt = nullptr; u16 *d_dest_cache = nullptr;
    ScanBufs scan;                // fast path
    std::vector<u64> task_tot;    // [ntasks][3] supermers, bytes, kmers of this rank
};

static void parse_release(hsk_ctx *c, ParseJob &j)
{
    c->pool.release(j.d_blk_cnt); c->pool.release(j.d_dest_cache); j.d_blk_cnt = nullptr; j.d_dest_cache = nullptr;
    scan_release(c, j.scan);
}

// The verdict words of a parse as the host reads them from the staging area (PinnedTail::parse_flags): a tile held more supermers than the
// record capacity; the device's error word; scan-placed items: chunks handed out; positions the drop mask left out
struct ParseFlags { u32 overflow, err, chunks, unused; unsigned long long dropped; };
static_assert(offsetof(ParseFlags, overflow) == 0 && offsetof(ParseFlags, err) == 4 && offsetof(ParseFlags, chunks) == 8 && offsetof(ParseFlags, dropped) == 16, "verdict words");
static_assert(sizeof(ParseFlags) <= sizeof(PinnedTail::parse_flags), "the verdict words live in PinnedTail::parse_flags");
constexpr u32 PARSE_ERR_INDEX = 32u;                      // error word: index_check_kernel refused the read index
constexpr u32 PARSE_ERR_BINS = 2u | 128u | 256u;          // error word: the scan-placed items' chunk store or a bin's map ran out
static ParseFlags *parse_flags(hsk_ctx *c) { return reinterpret_cast<ParseFlags *>(staging(c)->parse_flags); }
// the words on their way to the host; scan: the fast scan's own (overflow, chunks) among them
static int read_parse_flags(hsk_ctx *c, hipStream_t stream, const ScanBufs &s, bool scan)
{
    ParseFlags *h = parse_flags(c);
    if (scan) HIPCHK(c, hipMemcpyAsync(&h->overflow, s.d_overflow, 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(c, hipMemcpyAsync(&h->err, c->d_err, 4, hipMemcpyDeviceToHost, stream));
    if (scan && s.bins.items) HIPCHK(c, hipMemcpyAsync(&h->chunks, s.bins.ctl, 4, hipMemcpyDeviceToHost, stream));
    if (s.d_dropped) HIPCHK(c, hipMemcpyAsync(&h->dropped, s.d_dropped, 8, hipMemcpyDeviceToHost, stream));
    return HSK_OK;
}

// an event pair of the profile (HSK_FLAG_PROFILE; kind: drain_profile_events, hsk_api.hip) around what follows on `stream`
static EvPair prof_begin(hsk_ctx *c, int kind, hipStream_t stream)
{
    EvPair ep{};
    if (c->cfg.flags & HSK_FLAG_PROFILE) { ep.a = ev_get(c); ep.b = ev_get(c); ep.kind = kind; (void)hipEventRecord(ep.a, stream); }
    return ep;
}
static void prof_end(hsk_ctx *c, const EvPair &ep, hipStream_t stream)
{
    if (c->cfg.flags & HSK_FLAG_PROFILE) { (void)hipEventRecord(ep.b, stream); c->ev_pending.push_back(ep); }
}

// The one place that names the instances of scan_kernel.  (k, m) = (31, 17) and (51, 17) have instances of their own;
// "scan_generic=1" (tests) sends them through the generic one.
static void launch_scan(const hsk_ctx *c, hipStream_t stream, u32 nblocks, u32 ntasks, const ParseArgs &a)
{
    const dim3 grid(nblocks), block(PARSE_THREADS);
    const size_t lds = (size_t)ntasks * 16;
    const bool generic = c->tune.scan_generic != 0;
    const bool k31 = a.k == 31 && a.m == 17 && !generic, k51 = a.k == 51 && a.m == 17 && !generic;
    if (a.drop_mask) hipLaunchKernelGGL((scan_kernel<0, 0, false, true>), grid, block, lds, stream, a);
    else if (a.bins && k31) hipLaunchKernelGGL((scan_kernel<31, 17, true>), grid, block, lds, stream, a);
    else if (a.bins) hipLaunchKernelGGL((scan_kernel<0, 0, true>), grid, block, lds, stream, a);
    else if (k31) hipLaunchKernelGGL((scan_kernel<31, 17>), grid, block, lds, stream, a);
    else if (k51) hipLaunchKernelGGL((scan_kernel<51, 17>), grid, block, lds, stream, a);
    else hipLaunchKernelGGL((scan_kernel<0, 0>), grid, block, lds, stream, a);
}

// The one place that names the placement kernels of the fast path.  place_items_kernel stages 16384 records + 32 tiles of packed
// words (~158 KB of dynamic LDS) and place_bytes_kernel nearly as much, which the runtime wants announced.
static void launch_place(hsk_ctx *, hipStream_t stream, PlaceKind kind, ParseArgs a, u32 nblocks, u32 ntasks)
{
    static bool announced[3] = {false, false, false};
    a.place_group = place_group(kind, a.rec_cap);
    if (kind == PLACE_RECORDS) {
        hipLaunchKernelGGL(place_kernel, dim3(nblocks), dim3(PARSE_THREADS), (size_t)ntasks * 16 + PLACE_MAX_REC * 4, stream, a);
        return;
    }
    const void *fn = kind == PLACE_ITEMS ? reinterpret_cast<const void *>(place_items_kernel) : reinterpret_cast<const void *>(place_bytes_kernel);
    if (!announced[kind]) { (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512); announced[kind] = true; }
    if (kind == PLACE_ITEMS)
        hipLaunchKernelGGL(place_items_kernel, dim3(nblocks), dim3(PLACE_ITEM_THREADS), (size_t)ntasks * 16 + 8 + (size_t)PLACE_ITEM_REC * 8 + (size_t)PLACE_ITEM_WORDS * 4, stream, a);
    else
        hipLaunchKernelGGL(place_bytes_kernel, dim3(nblocks), dim3(PLACE_BYTES_THREADS),
                           (size_t)ntasks * 40 + PLACE_BYTES_REC * 8 + PLACE_BYTES_WORDS * 4 + (a.sm_sub16 ? PLACE_BYTES_REC * 2 : 0), stream, a);
}
// ... and the general path's: emit_kernel reads the task ids COUNT has kept, without them the parse kernel hashes again
static void launch_emit(hsk_ctx *, hipStream_t stream, const ParseArgs &a, u32 nblocks, u32 ntasks)
{
    if (a.dest_cache) hipLaunchKernelGGL(emit_kernel, dim3(nblocks), dim3(PARSE_THREADS), (size_t)ntasks * 16, stream, a);
    else if (a.drop_mask) hipLaunchKernelGGL((parse_kernel<PARSE_EMIT, false, true>), dim3(nblocks), dim3(PARSE_THREADS), (size_t)ntasks * 16, stream, a);
    else hipLaunchKernelGGL((parse_kernel<PARSE_EMIT, false>), dim3(nblocks), dim3(PARSE_THREADS), (size_t)ntasks * 16, stream, a);
}

// The slab ingest.  The packed reads cross PCIe as DMA copies, slab by slab, on the copy stream -- all of them enqueued before the
// first scan -- while the main stream hashes the slabs that have landed, so the link and the VALUs work side by side: the parse takes
// about as long as the transfer (a kernel reading the host buffer in place gets ~40 GB/s out of the link, the DMA engine ~55).
// A slab's scan reaches PARSE_WORDS - 128 words into the NEXT slab (the windows of its last k-mers), not further: every slab's first
// SLAB_HEAD bytes travel as a copy of their own with an event (`head`), and the scan of slab s waits for slab s (`landed`) and for the
// head of slab s + 1 -- not for all of slab s + 1 (the first scan started after two slabs, 5.6 ms into the call; now after one).
struct SlabEvents { std::vector<hipEvent_t> head, landed; };
static int enqueue_slab_copies(hsk_ctx *c, EvList &evs, const ParseTiling &t, const u8 *h2d_src, const u8 *d_packed, u64 packed_bytes, SlabEvents &ev)
{
    hipStream_t s = c->d2h_stream;
    u8 *dst = const_cast<u8 *>(d_packed);
    ev.head.resize(t.nslabs); ev.landed.resize(t.nslabs);
    const EvPair hp = prof_begin(c, 5, s);
    for (u32 sl = 0; sl < t.nslabs; ++sl) {
        const SlabBytes b = slab_bytes(t, sl, packed_bytes);
        if (b.bh > b.b0) HIPCHK(c, hipMemcpyAsync(dst + b.b0, h2d_src + b.b0, b.bh - b.b0, hipMemcpyHostToDevice, s));
        ev.head[sl] = evs.get();
        HIPCHK(c, hipEventRecord(ev.head[sl], s));
        if (b.b1 > b.bh) HIPCHK(c, hipMemcpyAsync(dst + b.bh, h2d_src + b.bh, b.b1 - b.bh, hipMemcpyHostToDevice, s));
        ev.landed[sl] = evs.get();
        HIPCHK(c, hipEventRecord(ev.landed[sl], s));
    }
    prof_end(c, hp, s);
    return HSK_OK;
}
// `stream` may scan slab sl after this
static int wait_for_slab(hsk_ctx *c, hipStream_t stream, const SlabEvents &ev, u32 sl)
{
    HIPCHK(c, hipStreamWaitEvent(stream, ev.landed[sl], 0));
    if (sl + 1 < ev.head.size()) HIPCHK(c, hipStreamWaitEvent(stream, ev.head[sl + 1], 0));
    return HSK_OK;
}

// the scan of the COUNT matrix: parse_scan_kernel (one workgroup) for the usual few dozen tasks, the three-kernel form from 128 columns on
static int launch_parse_scan(hsk_ctx *c, hipStream_t st, const u64 *blk_cnt, u32 nblocks, u32 ntasks, const u32 *d_order, const u8 *d_skip,
                             u64 *d_task_tot, u64 *d_task_base, u64 *d_blk_base, u64 *d_run = nullptr, u64 *d_scratch = nullptr)
{
    if (ntasks < 128) {
        hipLaunchKernelGGL(parse_scan_kernel, dim3(1), dim3(HSK_MAX_TASKS), 0, st, blk_cnt, nblocks, ntasks, d_order, d_skip, d_task_tot, d_task_base, d_blk_base, d_run);
        return HSK_OK;
    }
    u64 *d_part = d_scratch;                              // [PS_SEGS][ntasks][3]
    if (!d_part) DALLOC(c, d_part, u64 *, (size_t)PS_SEGS * ntasks * 3 * 8);
    const dim3 grid((ntasks + PS_THREADS - 1) / PS_THREADS, PS_SEGS);
    hipLaunchKernelGGL(parse_scan_part_kernel, grid, dim3(PS_THREADS), 0, st, blk_cnt, nblocks, ntasks, d_skip, d_part);
    hipLaunchKernelGGL(parse_scan_base_kernel, dim3(1), dim3(HSK_MAX_TASKS), 0, st, (const u64 *)d_part, ntasks, d_order, d_task_tot, d_task_base, d_run);
    hipLaunchKernelGGL(parse_scan_fill_kernel, grid, dim3(PS_THREADS), 0, st, blk_cnt, nblocks, ntasks, d_skip, (const u64 *)d_part, (const u64 *)d_task_base, d_blk_base);
    if (!d_scratch) c->pool.release(d_part);              // (stream-ordered reuse: the caller's later work is enqueued on the same stream)
    return HSK_OK;
}

// parse_count, part 1 -- the fast scan: its buffers, scan_kernel over the whole input or slab by slab behind the DMA copies (h2d_src),
// the task totals and the verdict words; returns when the host has them
static int count_fast_scan(hsk_ctx *c, ParseJob &j, const ParseTiling &t, const u8 *h2d_src, u64 *d_task_tot)
{
    ParseArgs &a = j.a;
    const u8 *d_packed = a.packed;
    int rc = scan_setup(c, j.scan, a, c->stream); if (rc) return rc;
    if (c->call.zc_src) { a.packed = c->call.zc_src; a.packed_copy = (u32 *)const_cast<u8 *>(d_packed); }      // ingest fused into the scan
    EvPair ep = prof_begin(c, 3, c->stream); ep.bytes = a.packed_bytes;
    if (h2d_src) {
        EvList evs(c); SlabEvents ev;
        rc = enqueue_slab_copies(c, evs, t, h2d_src, d_packed, a.packed_bytes, ev); if (rc) return rc;
        for (u32 sl = 0; sl < a.nslabs; ++sl) {
            rc = wait_for_slab(c, c->stream, ev, sl); if (rc) return rc;
            a.slab = sl;
            launch_scan(c, c->stream, j.nblocks, j.ntasks, a);
        }
        a.slab = 0;
    } else launch_scan(c, c->stream, j.nblocks, j.ntasks, a);
    prof_end(c, ep, c->stream);
    a.packed = d_packed; a.packed_copy = nullptr; c->call.zc_src = nullptr;                                  // everything after the scan reads the copy in HBM
    hipLaunchKernelGGL(task_totals_kernel, dim3(1), dim3(HSK_MAX_TASKS), 0, c->stream, j.d_blk_cnt, j.nblocks, j.ntasks, d_task_tot);
    rc = read_parse_flags(c, c->stream, j.scan, true); if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(j.task_tot.data(), d_task_tot, (size_t)j.ntasks * 3 * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hsk_sync(c, c->stream));
    if (j.scan.d_dropped) c->call.dropped_now = parse_flags(c)->dropped;
    if (j.scan.bins.items) j.scan.bins.nchunks = std::min(parse_flags(c)->chunks, j.scan.bins.cap);
    return HSK_OK;
}

// parse_count, part 2 -- the verdict on the fast scan: counted, or one of the two ways on; an error, or the call again (retry_plan)
enum ParseVerdict { PARSE_COUNTED, PARSE_GAPS, PARSE_OVERFLOW };
static int count_verdict(hsk_ctx *c, const ParseJob &j, ParseVerdict &v)
{
    const ParseFlags &f = *parse_flags(c);
    v = PARSE_COUNTED;
    bool gaps = c->call.roff_bad; c->call.roff_bad = false;
    if (c->call.roff_check.valid() && !c->call.roff_check.get()) gaps = true;
    if (gaps) { v = PARSE_GAPS; return HSK_OK; }                   // the host threads found a gap while the GPU scanned
    if (c->call.index_unchecked) {
        c->call.index_unchecked = false;
        if (f.err & PARSE_ERR_INDEX) { (void)hipMemsetAsync(c->d_err, 0, 4, c->stream); return fail(c, HSK_ERR_INVALID_ARG, "the read index is not ascending / overlaps / leaves the packed buffer"); }
    }
    if (j.scan.bins.items && (f.err & PARSE_ERR_BINS)) {           // the call again, without the combining extraction
        (void)hipMemsetAsync(c->d_err, 0, 4, c->stream); c->call.combine_veto = true; return retry_plan("the scan-placed items' chunk store or a bin's map ran out (error word)", f.err);
    }
    if (f.overflow && c->call.vt_shift) { c->call.combine_veto = true; return retry_plan("a tile beyond the record capacity"); }      // (the general kernels know no virtual tasks: the call again, without them)
    if (f.overflow) v = PARSE_OVERFLOW;                            // a tile with more supermers than the record capacity: the general kernels
    return HSK_OK;
}
// PARSE_GAPS: the buffer's reads do not lie back to back.  The caller's offsets (and lengths, where those were a guess from a sample)
// are copied now and validated on the device; the fast part then runs again with them
static int send_given_index(hsk_ctx *c, const u64 *d_roff, const u32 *d_rlen, u64 nreads, u64 packed_bytes)
{
    u64 *given = c->call.roff_given;
    if (c->call.rlen_host) {
        HIPCHK(c, hipMemcpyAsync(const_cast<u32 *>(d_rlen), c->call.rlen_host, nreads * 4, hipMemcpyHostToDevice, c->stream));
        c->stats.h2d_bytes += nreads * 4; c->call.rlen_host = nullptr;
    }
    HIPCHK(c, hipMemcpyAsync(given, c->call.roff_host, nreads * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(given + nreads, d_roff + nreads, 8, hipMemcpyDeviceToDevice, c->stream));
    hipLaunchKernelGGL(index_check_kernel, dim3(1024), dim3(256), 0, c->stream, given, d_rlen, nreads, packed_bytes, c->d_err);
    c->call.index_unchecked = true;
    c->stats.h2d_bytes += nreads * 8;
    return HSK_OK;
}
// PARSE_OVERFLOW: the job leaves the fast path.  The general kernels know one tile range per workgroup and no records
static void leave_fast_path(hsk_ctx *c, ParseJob &j)
{
    ParseArgs &a = j.a;
    j.fast = false; c->stats.parse_fallbacks++;
    c->call.dropped_now = 0;                                       // (the general kernels count again; they honour the same mask: several ranks stay consistent)
    if (a.nslabs > 1) {
        const ParseTiling t = call_tiling(c, a.packed_bytes);
        ParseArgs b = make_parse_args(c, t, a.packed, a.packed_bytes, a.roff, a.rlen, a.nreads, a.rid_base, a.ntasks);
        b.blk_cnt = a.blk_cnt; b.rec_cap = a.rec_cap; b.place_group = a.place_group;
        a = b; j.nblocks = t.nblocks;
    }
    ScanBufs &s = j.scan;
    c->pool.release(s.d_tile_r0); c->pool.release(s.d_tile_rec); c->pool.release(s.d_tile_nrec); c->pool.release(s.d_tile_sub);
    s.d_tile_r0 = s.d_tile_rec = s.d_tile_nrec = s.d_tile_sub = nullptr;
    a.tile_r0 = a.tile_rec = a.tile_nrec = a.tile_sub = nullptr;
}

// parse_count, part 3 -- the general kernels' COUNT (M > SCAN_MAX_M, "parse_fast=0", or after PARSE_OVERFLOW)
static int count_general(hsk_ctx *c, ParseJob &j, u64 *d_task_tot)
{
    ParseArgs &a = j.a;
    // task id per base position, kept from COUNT to EMIT (2 B x 4 x packed_bytes); optional: without it EMIT re-hashes
    j.d_dest_cache = (u16 *)c->pool.alloc((size_t)a.ntiles * PARSE_TILE * 2);
    a.dest_cache = j.d_dest_cache;
    a.drop_mask = c->call.drop_mask_now;                               // (a fresh ParseArgs after a slab fallback has lost it)
    if (a.drop_mask) {
        if (!j.scan.d_dropped) DALLOC(c, j.scan.d_dropped, unsigned long long *, 256);
        HIPCHK(c, hipMemsetAsync(j.scan.d_dropped, 0, 8, c->stream)); a.dropped = j.scan.d_dropped;
    }
    if (a.drop_mask) hipLaunchKernelGGL((parse_kernel<PARSE_COUNT, false, true>), dim3(j.nblocks), dim3(PARSE_THREADS), (size_t)j.ntasks * 16, c->stream, a);
    else hipLaunchKernelGGL((parse_kernel<PARSE_COUNT, false>), dim3(j.nblocks), dim3(PARSE_THREADS), (size_t)j.ntasks * 16, c->stream, a);
    hipLaunchKernelGGL(task_totals_kernel, dim3(1), dim3(HSK_MAX_TASKS), 0, c->stream, j.d_blk_cnt, j.nblocks, j.ntasks, d_task_tot);
    int rc = read_parse_flags(c, c->stream, j.scan, false); if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(j.task_tot.data(), d_task_tot, (size_t)j.ntasks * 3 * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hsk_sync(c, c->stream));
    if (a.drop_mask) c->call.dropped_now = parse_flags(c)->dropped;
    // (hsk_count derives the read index only for the fast parse; should a derived index ever arrive here with its verdict still open, a
    //  wrong guess must not be counted: the call fails instead of trusting lengths and offsets nobody has confirmed)
    if (c->call.roff_check.valid() && !c->call.roff_check.get()) return fail(c, HSK_ERR_INTERNAL, "derived read index reached the general parse unverified and does not match the caller's");
    if (c->call.index_unchecked) {
        c->call.index_unchecked = false;
        if (parse_flags(c)->err & PARSE_ERR_INDEX) { (void)hipMemsetAsync(c->d_err, 0, 4, c->stream); return fail(c, HSK_ERR_INVALID_ARG, "the read index is not ascending / overlaps / leaves the packed buffer"); }
    }
    return HSK_OK;
}

static int parse_count(hsk_ctx *c, const u8 *d_packed, u64 packed_bytes, const u64 *d_roff, const u32 *d_rlen, u64 nreads,
                       int64_t rid_base, u32 ntasks, ParseJob &j)
{
    j = ParseJob();
    j.ntasks = ntasks; j.d_roff = d_roff; j.nreads = nreads; j.rid_base = rid_base;
    j.task_tot.assign((size_t)ntasks * 3, 0);
    if (nreads == 0 || packed_bytes == 0) return HSK_OK;            // nothing to parse on this rank
    j.empty = false;
    j.fast = c->tune.parse_fast != 0 && c->cfg.minimizer_size <= SCAN_MAX_M;
    // slab ingest (hsk_count() from pinned memory): only the fast path hashes slab by slab, and only an input large enough for slabs;
    // everything else wants the reads in HBM first
    const u8 *h2d_src = c->call.h2d_src; c->call.h2d_src = nullptr;
    const ParseTiling t = call_tiling(c, packed_bytes, h2d_src && j.fast ? (u32)c->call.h2d_slabs : 1);
    if (h2d_src && t.nslabs <= 1) { HIPCHK(c, hipMemcpyAsync(const_cast<u8 *>(d_packed), h2d_src, packed_bytes, hipMemcpyHostToDevice, c->stream)); h2d_src = nullptr; }
    j.a = make_parse_args(c, t, d_packed, packed_bytes, d_roff, d_rlen, nreads, rid_base, ntasks);
    j.nblocks = t.nblocks;
    DALLOC(c, j.d_blk_cnt, u64 *, (size_t)PARSE_MAX_BLOCKS * ntasks * 3 * 8);
    j.a.blk_cnt = j.d_blk_cnt;
    u64 *d_task_tot; DALLOC(c, d_task_tot, u64 *, (size_t)ntasks * 3 * 8 + 64);
    parse_flags(c)->overflow = 0;
    int rc = HSK_OK;
    if (j.fast) {
        ParseVerdict v = PARSE_COUNTED;
        rc = count_fast_scan(c, j, t, h2d_src, d_task_tot);
        if (rc == HSK_OK) rc = count_verdict(c, j, v);
        if (rc == HSK_OK && v == PARSE_GAPS) {                      // everything again with the caller's offsets: a second call of the fast part
            c->pool.release(d_task_tot);
            parse_release(c, j);
            rc = send_given_index(c, d_roff, d_rlen, nreads, packed_bytes); if (rc) return rc;
            return parse_count(c, d_packed, packed_bytes, c->call.roff_given, d_rlen, nreads, rid_base, ntasks, j);
        }
        if (rc == HSK_OK && v == PARSE_OVERFLOW) leave_fast_path(c, j);
    }
    if (rc == HSK_OK && c->call.zc_src) {                           // the general kernels read the reads more than once: plain copy first
        HIPCHK(c, hipMemcpyAsync(const_cast<u8 *>(d_packed), c->call.zc_src, packed_bytes, hipMemcpyDefault, c->stream));
        c->call.zc_src = nullptr;
    }
    if (rc == HSK_OK && !j.fast) rc = count_general(c, j, d_task_tot);
    if (rc == HSK_OK) HIPCHK(c, hipGetLastError());
    c->pool.release(d_task_tot);
    return rc;
}

// `order` (storage order of tasks) must be a permutation of 0..ntasks-1.
// skip (optional, [ntasks]): tasks whose supermers are not stored (they take no room and report zero totals)
static int parse_place(hsk_ctx *c, ParseJob &j, const std::vector<u32> &order, SupermerStore &st, const std::vector<u8> *skip = nullptr, bool supermers_travel = false)
{
    const bool ext = c->cfg.extension != 0;
    const u32 ntasks = j.ntasks;
    st = SupermerStore();
    st.ntasks = ntasks; st.nblocks = j.nblocks; st.order = order;
    st.task_tot = j.task_tot;
    if (skip) for (u32 t = 0; t < ntasks; ++t) if ((*skip)[t]) st.task_tot[3 * t] = st.task_tot[3 * t + 1] = st.task_tot[3 * t + 2] = 0;
    st.task_base.assign((size_t)ntasks * 3, 0);
    { u64 s = 0, b = 0, k = 0;
      for (u32 i = 0; i < ntasks; ++i) { const u32 t = order[i]; st.task_base[3 * t] = s; st.task_base[3 * t + 1] = b; st.task_base[3 * t + 2] = k;
                                          s += st.task_tot[3 * t]; b += st.task_tot[3 * t + 1]; k += st.task_tot[3 * t + 2]; }
      st.tot_sup = s; st.tot_bytes = b; st.tot_kmers = k; }
    if (j.empty) return HSK_OK;
    ParseArgs &a = j.a;
    u64 *d_blk_base, *d_task_tot, *d_task_base; u32 *d_order;
    DALLOC(c, d_blk_base, u64 *, (size_t)j.nblocks * ntasks * 2 * 8);
    DALLOC(c, d_task_tot, u64 *, (size_t)ntasks * 3 * 8);
    DALLOC(c, d_task_base, u64 *, (size_t)ntasks * 3 * 8);
    DALLOC(c, d_order, u32 *, (size_t)ntasks * 4);
    HIPCHK(c, hipMemcpyAsync(d_order, order.data(), (size_t)ntasks * 4, hipMemcpyHostToDevice, c->stream));
    u8 *d_skip = nullptr;
    if (skip) {
        DALLOC(c, d_skip, u8 *, ntasks);
        HIPCHK(c, hipMemcpyAsync(d_skip, skip->data(), ntasks, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hsk_sync(c, c->stream));          // the mask is host memory of the caller
    }
    a.task_skip = d_skip;
    { int prc = launch_parse_scan(c, c->stream, j.d_blk_cnt, j.nblocks, ntasks, d_order, d_skip, d_task_tot, d_task_base, d_blk_base); if (prc) return prc; }
    // the small matrices are released once their last reader is enqueued (pool reuse is stream-ordered: every later user of these
    // blocks is enqueued on the same stream)
    auto done = [&](int rc) {
        c->pool.release(d_blk_base); c->pool.release(d_task_tot); c->pool.release(d_task_base); c->pool.release(d_order); c->pool.release(d_skip);
        a.task_skip = nullptr;
        return rc;
    };
    const bool from_bins = j.fast && j.scan.bins.items != nullptr && !skip && !supermers_travel && !ext;      // scan_kernel has placed the items already
    const bool item_mode = from_bins || (j.fast && a.tile_sub && !skip && !supermers_travel && !ext);      // combining extraction: the slots hold the supermers themselves
    if (!item_mode) DALLOC(c, st.sm_len, u8 *, st.tot_sup + 64);
    // byte-store mode (fast parse path): the supermers' bases are copied into per-task byte runs while the reads stream through
    // the byte placement once; positions are kept only where something still needs them (EXTENSION: pos / rid lookup)
    bool bytes_mode = !item_mode && j.fast && place_bytes_enabled(c, supermers_travel) && a.rec_cap <= PLACE_BYTES_REC;
    for (u32 t = 0; t < ntasks && bytes_mode; ++t) if (st.task_tot[3 * t + 1] >= (1ULL << 32)) bytes_mode = false;     // 32-bit offsets inside a task's run
    // several ranks with the combining extraction planned (c->call.combine_now): the supermers' minimizer bits go into the store as well
    const bool with_sub16 = bytes_mode && supermers_travel && c->call.combine_now && a.tile_sub && !ext;      // (heavy-hitter tasks are skipped by the kernel itself: their k-mers travel as lists)
    a.sm_sub16 = nullptr;
    if (with_sub16) { DALLOC(c, st.sm_sub16, unsigned short *, st.tot_sup * 2 + 64); a.sm_sub16 = st.sm_sub16; }
    if (bytes_mode) {
        DALLOC(c, st.sm_bytes, u8 *, st.tot_bytes + 256);
        if (!supermers_travel) DALLOC(c, st.sm_boff, u32 *, st.tot_sup * 4 + 64);
        st.bytes_done = true;
        HIPCHK(c, hipMemsetAsync(st.sm_bytes + st.tot_bytes, 0, 256, c->stream));     // the extraction's windows read a few words past the last supermer
    }
    if ((!bytes_mode && !item_mode) || ext) DALLOC(c, st.sm_gpos, u64 *, st.tot_sup * 8 + 64);      // position mode: bases stay in the packed reads
    if (ext) { DALLOC(c, st.sm_pos, u32 *, st.tot_sup * 4 + 64); DALLOC(c, st.sm_rid, int32_t *, st.tot_sup * 4 + 64); }
    a.sm_sub = nullptr; a.sm_item = nullptr;
    if (from_bins) return done(bins_to_store(c, j.scan.bins, st, ntasks, c->call.vt_shift, c->stream));
    if (item_mode) { DALLOC(c, st.sm_sub, u32 *, st.tot_sup * 4 + 64); DALLOC(c, st.sm_item, u64 *, st.tot_sup * 16 + 64); a.sm_sub = st.sm_sub; a.sm_item = st.sm_item; }
    a.blk_base = d_blk_base; a.sm_len = st.sm_len; a.sm_gpos = st.sm_gpos; a.sm_bytes = st.sm_bytes; a.sm_boff = st.sm_boff; a.task_base3 = d_task_base;
    if (st.tot_sup) {
        if (j.fast) {
            EvPair ep = prof_begin(c, 4, c->stream); ep.keys = st.tot_sup;
            launch_place(c, c->stream, bytes_mode ? PLACE_BYTES : item_mode ? PLACE_ITEMS : PLACE_RECORDS, a, j.nblocks, ntasks);
            prof_end(c, ep, c->stream);
        }
        else launch_emit(c, c->stream, a, j.nblocks, ntasks);
        if (ext) hipLaunchKernelGGL(resolve_pos_rid_kernel, dim3((u32)std::min<u64>((st.tot_sup + 255) / 256, 8192)), dim3(256), 0, c->stream,
                                    st.sm_gpos, st.tot_sup, j.d_roff, j.nreads, j.rid_base, st.sm_pos, st.sm_rid, (const u32 *)j.scan.d_tile_r0, a.ntiles);
    }
    HIPCHK(c, hipGetLastError());
    return done(HSK_OK);
}

// hsk_count() from pinned host memory on one GPU (no payload): ingest, scan and placement as ONE pipeline over slabs.
//   copy stream   DMA copy of slab s + 2          (the link: ~55 GB/s, the floor of the whole parse)
//   main stream   scan_kernel of slab s            (behind the copy of slab s + 1; the VALUs have ~0.8 ms to spare per slab)
//   second stream task totals, slot bases and the placement of slab s - 1   (fills those gaps: the placement, 8.6 ms when it
//                 runs after the last scan, is off the critical path)
// The store is laid out [slab][task] (a slab's slot bases need only the slabs before it: parse_scan_kernel carries the
// running totals on the device), so a task's supermers are one segment per slab (`segs`), which the extraction takes like the
// segments of several source ranks.  Returns HSK_OK, an error, or PARSE_FALLBACK: nothing has been decided, the packed reads
// are in HBM, the caller takes parse_count / parse_place (a tile beyond the record capacity, an index that needs the
// caller's offsets, a device-side index check that failed).
constexpr int PARSE_FALLBACK = -1000;
// its buffers: the scan's, a COUNT matrix per slab, and what the slabs' placements share
struct PipeBufs {
    ScanBufs scan;
    u64 *d_blk_cnt = nullptr, *d_blk_base = nullptr, *d_tot = nullptr, *d_task_base = nullptr, *d_run = nullptr, *d_ps = nullptr; u32 *d_order = nullptr;
};
static void pipe_release(hsk_ctx *c, PipeBufs &p)
{
    scan_release(c, p.scan);
    c->pool.release(p.d_blk_cnt); c->pool.release(p.d_blk_base); c->pool.release(p.d_tot); c->pool.release(p.d_task_base); c->pool.release(p.d_run); c->pool.release(p.d_ps); c->pool.release(p.d_order);
    p = PipeBufs();
}
// buffers, store (at most rec_cap supermers per tile -- a tile beyond that falls back; its real size is known when the last slab is in)
// and the arguments; everything it enqueues is on the main stream
static int pipe_setup(hsk_ctx *c, PipeBufs &p, ParseArgs &a, u32 nblocks, SupermerStore &st)
{
    const u32 ntasks = a.ntasks, nsl = a.nslabs;
    const size_t mat = (size_t)nblocks * ntasks;
    DALLOC(c, p.d_blk_cnt, u64 *, mat * 3 * 8 * nsl);
    DALLOC(c, p.d_blk_base, u64 *, mat * 2 * 8);
    DALLOC(c, p.d_tot, u64 *, (size_t)nsl * ntasks * 3 * 8 + 64);
    DALLOC(c, p.d_task_base, u64 *, (size_t)ntasks * 3 * 8);
    DALLOC(c, p.d_run, u64 *, 256);
    DALLOC(c, p.d_order, u32 *, (size_t)ntasks * 4);
    DALLOC(c, p.d_ps, u64 *, (size_t)PS_SEGS * ntasks * 3 * 8);
    int rc = scan_setup(c, p.scan, a, c->stream); if (rc) return rc;
    const u64 cap_sup = a.ntiles * (u64)a.rec_cap;
    st = SupermerStore();
    st.ntasks = ntasks; st.nblocks = nblocks;
    if (a.bins) {}                                                          // (the items live in the bins' chunk store)
    else if (a.tile_sub) { DALLOC(c, st.sm_sub, u32 *, cap_sup * 4 + 64); DALLOC(c, st.sm_item, u64 *, cap_sup * 16 + 64); }      // item mode (combining extraction)
    else { DALLOC(c, st.sm_len, u8 *, cap_sup + 64); DALLOC(c, st.sm_gpos, u64 *, cap_sup * 8 + 64); }
    st.order.resize(ntasks); for (u32 t = 0; t < ntasks; ++t) st.order[t] = t;
    u32 *h_order = (u32 *)((char *)c->pinned + (128u << 10));              // (pinned staging: the copy is asynchronous)
    memcpy(h_order, st.order.data(), (size_t)ntasks * 4);
    HIPCHK(c, hipMemsetAsync(p.d_run, 0, 24, c->stream));
    HIPCHK(c, hipMemcpyAsync(p.d_order, h_order, (size_t)ntasks * 4, hipMemcpyHostToDevice, c->stream));
    a.place_one = 1;
    a.sm_len = st.sm_len; a.sm_gpos = st.sm_gpos; a.blk_base = p.d_blk_base; a.task_base3 = p.d_task_base;
    a.sm_sub = st.sm_sub; a.sm_item = st.sm_item;
    return HSK_OK;
}
// segments: slab by slab, tasks in storage order inside a slab (what parse_scan_kernel laid out on the device)
static void pipe_segments(const std::vector<u64> &tot, u32 nsl, bool bins, SupermerStore &st, std::vector<TaskSegs> &segs)
{
    const u32 ntasks = st.ntasks;
    st.task_tot.assign((size_t)ntasks * 3, 0); st.task_base.assign((size_t)ntasks * 3, 0);
    segs.assign(ntasks, TaskSegs());
    u64 run_s = 0, run_b = 0;
    for (u32 sl = 0; sl < nsl; ++sl)
        for (u32 i = 0; i < ntasks; ++i) {
            const u32 t = st.order[i];
            const u64 *m = &tot[((size_t)sl * ntasks + t) * 3];
            if (m[0] && bins && !segs[t].segs.empty()) segs[t].segs[0].n_sup += m[0];      // (bins: one pseudo segment per task -- only its supermer total is used)
            else if (m[0]) {
                ExpSeg sg; sg.sup_off = run_s; sg.n_sup = m[0]; sg.byte_off = run_b; sg.kmer_off = segs[t].nkmers; sg.tile_start = 0;
                segs[t].segs.push_back(sg);
            }
            segs[t].nkmers += m[2];
            st.task_tot[3 * t] += m[0]; st.task_tot[3 * t + 1] += m[1]; st.task_tot[3 * t + 2] += m[2];
            run_s += m[0]; run_b += m[1];
        }
    st.tot_sup = run_s; st.tot_bytes = run_b; st.tot_kmers = 0;
    for (u32 t = 0; t < ntasks; ++t) st.tot_kmers += st.task_tot[3 * t + 2];
}
static int parse_ingest_pipelined(hsk_ctx *c, const u8 *h2d_src, const u8 *d_packed, u64 packed_bytes, const u64 *d_roff, const u32 *d_rlen, u64 nreads,
                                  int64_t rid_base, u32 ntasks, SupermerStore &st, std::vector<TaskSegs> &segs)
{
    const ParseTiling t = call_tiling(c, packed_bytes, (u32)c->call.h2d_slabs);
    if (t.nslabs <= 1) return PARSE_FALLBACK;
    const u32 nsl = t.nslabs, nblocks = t.nblocks;
    ParseArgs a = make_parse_args(c, t, d_packed, packed_bytes, d_roff, d_rlen, nreads, rid_base, ntasks);
    hipStream_t sA = c->stream, sB = c->comm_stream;
    PipeBufs p;
    int rc = pipe_setup(c, p, a, nblocks, st); if (rc) return rc;
    const bool bins = a.bins != nullptr;                                    // scan_kernel places the items itself: no records, no placement kernel
    const PlaceKind kind = a.tile_sub ? PLACE_ITEMS : PLACE_RECORDS;
    EvList evs(c);
    hipEvent_t ready = evs.get();                                          // the small buffers are set up; the second stream may start
    HIPCHK(c, hipEventRecord(ready, sA));
    HIPCHK(c, hipStreamWaitEvent(sB, ready, 0));
    SlabEvents ev;
    rc = enqueue_slab_copies(c, evs, t, h2d_src, d_packed, packed_bytes, ev); if (rc) return rc;
    EvPair sp = prof_begin(c, 3, sA), pp = prof_begin(c, 4, sB); sp.bytes = packed_bytes;
    for (u32 sl = 0; sl < nsl; ++sl) {
        rc = wait_for_slab(c, sA, ev, sl); if (rc) return rc;
        a.slab = sl; a.blk_cnt = p.d_blk_cnt + (size_t)sl * nblocks * ntasks * 3;
        launch_scan(c, sA, nblocks, ntasks, a);
        hipEvent_t scanned = evs.get();
        HIPCHK(c, hipEventRecord(scanned, sA));
        // the slab's placement on the second stream: totals, bases (behind everything the slabs before laid out), supermers to their slots
        // -- before the host has seen the overflow word: the placement kernels read it themselves (ParseArgs::place_one)
        HIPCHK(c, hipStreamWaitEvent(sB, scanned, 0));
        rc = launch_parse_scan(c, sB, (const u64 *)a.blk_cnt, nblocks, ntasks, (const u32 *)p.d_order, (const u8 *)nullptr,
                               p.d_tot + (size_t)sl * ntasks * 3, p.d_task_base, p.d_blk_base, p.d_run, p.d_ps); if (rc) return rc;
        if (!bins) launch_place(c, sB, kind, a, nblocks, ntasks);
    }
    prof_end(c, sp, sA); prof_end(c, pp, sB);
    // the verdicts and the totals (sB is behind every scan: scanned events)
    std::vector<u64> tot((size_t)nsl * ntasks * 3);
    u64 *h_tot = (u64 *)((char *)c->pinned + (192u << 10));
    const bool staged = (size_t)nsl * ntasks * 24 <= (64u << 10);
    rc = read_parse_flags(c, sB, p.scan, true); if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(staged ? h_tot : tot.data(), p.d_tot, (size_t)nsl * ntasks * 24, hipMemcpyDeviceToHost, sB));
    hipEvent_t placed = evs.get();
    HIPCHK(c, hipEventRecord(placed, sB));
    HIPCHK(c, hipStreamWaitEvent(sA, placed, 0));                          // the extraction (main stream) reads the store
    HIPCHK(c, hsk_sync(c, sB));
    if (staged) memcpy(tot.data(), h_tot, (size_t)nsl * ntasks * 24);
    const ParseFlags &f = *parse_flags(c);
    bool fallback = f.overflow != 0;                                        // a tile with more supermers than the record capacity
    if (c->call.roff_check.valid() && !c->call.roff_check.get()) { fallback = true; c->call.roff_bad = true; }     // the reads do not lie back to back: the caller's offsets are needed
    if (c->call.index_unchecked && (f.err & PARSE_ERR_INDEX)) fallback = true;          // (parse_count reports it)
    if (bins && (f.err & PARSE_ERR_BINS)) { fallback = true; (void)hipMemsetAsync(c->d_err, 0, 4, sA); }      // (run_pipeline: the call again, without virtual tasks)
    if (fallback) { HIPCHK(c, hsk_sync(c, sA)); pipe_release(c, p); free_store(c, st); return PARSE_FALLBACK; }      // (the main stream's wait first: its scans read the buffers)
    if (p.scan.d_dropped) c->call.dropped_now = f.dropped;
    if (bins) {
        p.scan.bins.nchunks = std::min(f.chunks, p.scan.bins.cap);
        rc = bins_to_store(c, p.scan.bins, st, ntasks, c->call.vt_shift, sA); if (rc) { pipe_release(c, p); return rc; }      // (main stream: behind the `placed` wait above)
    }
    c->call.index_unchecked = false;
    pipe_segments(tot, nsl, bins, st, segs);
    const u64 cap_sup = a.ntiles * (u64)a.rec_cap;
    if (!bins && st.tot_sup > cap_sup) { pipe_release(c, p); free_store(c, st); return fail(c, HSK_ERR_INTERNAL, "supermer store overrun (%llu > %llu)", (unsigned long long)st.tot_sup, (unsigned long long)cap_sup); }
    if ((c->cfg.flags & HSK_FLAG_PROFILE) && !c->ev_pending.empty()) c->ev_pending.back().keys = st.tot_sup;
    pipe_release(c, p);                                                     // (stream-ordered reuse: later users are enqueued behind the kernels above)
    return HSK_OK;
}

// count + place with a known storage order
static int parse_phase(hsk_ctx *c, const u8 *d_packed, u64 packed_bytes, const u64 *d_roff, const u32 *d_rlen, u64 nreads,
                       int64_t rid_base, u32 ntasks, const std::vector<u32> &order, SupermerStore &st)
{
    ParseJob j;
    int rc = parse_count(c, d_packed, packed_bytes, d_roff, d_rlen, nreads, rid_base, ntasks, j);
    if (rc == HSK_OK) rc = parse_place(c, j, order, st);
    parse_release(c, j);
    return rc;
}
