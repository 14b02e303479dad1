// hsk_host_strand.h -- host side of hsk_result_strands, hsk_strands_task and hsk_strands_free: the strand of every k-mer occurrence of a
// resident EXTENSION result, one bit per payload slot (kernel: hsk_strand.h).
// Part of the single translation unit hsk_api.hip (included behind hsk_host_pairs.h, whose task table it shares; everything here is file-local).
#pragma once

// One block of bit words for all tasks, every task from a word boundary; the tasks that have entries through ONE launch over the table of
// task descriptors the pairs stage uses (pairs_range_tasks), a task whose entries were all filtered out -- nothing but gaps -- by a memset.
// Host reads are uploaded for the call.  One wait: the counters and the error word.
static int strands_impl(hsk_ctx *c, const ResultPriv *rp, int nw, int32_t ntasks, const void *packed, u64 packed_bytes, const void *roff, const void *rlen, u64 nreads,
                        int64_t rid_base, bool reads_on_device, hsk_strands *out, StrandsPriv *sp)
{
    PairRange r;
    int rc = pairs_range_tasks(c, rp, 0, ntasks, r); if (rc) return rc;
    std::vector<StrandSpan> span;
    u64 words = 0, tiles = 0;
    sp->word0.assign(ntasks, 0); sp->npay.assign(ntasks, 0);
    for (int32_t t = 0; t < ntasks; ++t) {
        const TaskOut &to = rp->dev_tasks[t];
        sp->word0[t] = words; sp->npay[t] = to.npay;
        if (to.n) { const StrandSpan s = {tiles, words}; span.push_back(s); tiles += (to.npay + ST_TILE - 1) / ST_TILE; }
        words += (to.npay + 63) / 64;
    }
    { const StrandSpan s = {tiles, words}; span.push_back(s); }
    if (tiles > 0x7fffffffULL) return fail(c, HSK_ERR_UNSUPPORTED, "hsk_result_strands: %llu payload tiles are more than one launch covers", (unsigned long long)tiles);
    EvList ev(c);
    hipEvent_t e_start = ev.get(), e_end = ev.get();
    HIPCHK(c, hipEventRecord(e_start, c->stream));
    DALLOC(c, sp->bits, u64 *, words * 8 + 64);
    for (int32_t t = 0; t < ntasks; ++t) {
        const TaskOut &to = rp->dev_tasks[t];
        if (!to.n && to.npay) HIPCHK(c, hipMemsetAsync(sp->bits + sp->word0[t], 0, (to.npay + 63) / 64 * 8, c->stream));
    }
    u64 *st = staging(c)->read_pairs;
    memset(st, 0, STRAND_STAT_WORDS * 8);
    if (!r.tk.empty()) {
        u8 *d_packed = nullptr; u64 *d_roff = nullptr; u32 *d_rlen = nullptr;
        if (!reads_on_device) {
            DALLOC(c, d_packed, u8 *, packed_bytes + 64); DALLOC(c, d_roff, u64 *, nreads * 8 + 64); DALLOC(c, d_rlen, u32 *, nreads * 4 + 64);
            if (packed_bytes) HIPCHK(c, hipMemcpyAsync(d_packed, packed, packed_bytes, hipMemcpyHostToDevice, c->stream));      // (pageable or pinned: the caller's arrays outlive the wait below)
            if (nreads) {
                HIPCHK(c, hipMemcpyAsync(d_roff, roff, nreads * 8, hipMemcpyHostToDevice, c->stream));
                HIPCHK(c, hipMemcpyAsync(d_rlen, rlen, nreads * 4, hipMemcpyHostToDevice, c->stream));
            }
            c->stats.h2d_bytes += packed_bytes + nreads * 12;
        }
        PairTask *d_tasks; StrandSpan *d_span; unsigned long long *d_stat;
        DALLOC(c, d_tasks, PairTask *, r.tk.size() * sizeof(PairTask)); DALLOC(c, d_span, StrandSpan *, span.size() * sizeof(StrandSpan));
        DALLOC(c, d_stat, unsigned long long *, STRAND_STAT_WORDS * 8);
        HIPCHK(c, hipMemcpyAsync(d_tasks, r.tk.data(), r.tk.size() * sizeof(PairTask), hipMemcpyHostToDevice, c->stream));      // (tk and span live until the wait below)
        HIPCHK(c, hipMemcpyAsync(d_span, span.data(), span.size() * sizeof(StrandSpan), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(d_stat, 0, STRAND_STAT_WORDS * 8, c->stream));
        StrandArgs sa; memset(&sa, 0, sizeof sa);
        sa.tasks = d_tasks; sa.span = d_span; sa.ntasks = (u32)r.tk.size(); sa.k = c->cfg.kmer_size;
        sa.packed = reads_on_device ? (const u8 *)packed : d_packed; sa.packed_bytes = packed_bytes;
        sa.roff = reads_on_device ? (const u64 *)roff : d_roff; sa.rlen = reads_on_device ? (const u32 *)rlen : d_rlen; sa.nreads = nreads; sa.rid_base = rid_base;
        sa.bits = sp->bits; sa.stats = d_stat;
        with_nw(nw, [&](auto w) { hipLaunchKernelGGL(strand_kernel<decltype(w)::value>, dim3((u32)tiles), dim3(ST_THREADS), 0, c->stream, sa); return 0; });
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(st, d_stat, STRAND_STAT_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipEventRecord(e_end, c->stream));
        HIPCHK(c, hsk_sync(c, c->stream));
        c->pool.release(d_tasks); c->pool.release(d_span); c->pool.release(d_stat);
        c->pool.release(d_packed); c->pool.release(d_roff); c->pool.release(d_rlen);
    } else {
        HIPCHK(c, hipEventRecord(e_end, c->stream));
        HIPCHK(c, hsk_sync(c, c->stream));
    }
    const u64 err = st[STRAND_STAT_ERR];
    if (err & STRAND_ERR_RID)
        return fail(c, HSK_ERR_INVALID_ARG, "hsk_result_strands: a payload names a read outside [%lld, %lld), the reads that were given (a rank is given the reads its payload names)",
                    (long long)rid_base, (long long)(rid_base + (int64_t)nreads));
    if (err & STRAND_ERR_POS) return fail(c, HSK_ERR_INVALID_ARG, "hsk_result_strands: a payload's position + K lies behind the end of its read: these are not the reads the result was counted from");
    if (err & STRAND_ERR_INDEX) return fail(c, HSK_ERR_INVALID_ARG, "hsk_result_strands: a read of the index lies outside the %llu packed bytes", (unsigned long long)packed_bytes);
    if (err & STRAND_ERR_MISMATCH) return fail(c, HSK_ERR_INVALID_ARG, "hsk_result_strands: the bases at a payload's position spell neither its k-mer nor the reverse complement: these are not the reads the result was counted from");
    out->ntasks = ntasks;
    out->payloads = st[STRAND_STAT_PAYLOADS]; out->reverse = st[STRAND_STAT_REVERSE]; out->palindromes = st[STRAND_STAT_PALINDROMES];
    float f = 0;
    if (hipEventElapsedTime(&f, e_start, e_end) == hipSuccess) out->ms_total = f;
    return HSK_OK;
}

extern "C" int hsk_result_strands(hsk_ctx *c, const hsk_result *res, const void *packed, uint64_t packed_bytes, const void *roff, const void *rlen,
                                  uint64_t nreads, int64_t rid_base, int32_t reads_on_device, hsk_strands *out)
{
    if (!c || !res || !out) return HSK_ERR_INVALID_ARG;
    memset(out, 0, sizeof *out);
    if ((nreads && (!roff || !rlen)) || (packed_bytes && !packed)) return fail(c, HSK_ERR_INVALID_ARG, "hsk_result_strands: %llu reads in %llu packed bytes and a NULL pointer among packed, read_byte_off and read_len",
                                                                               (unsigned long long)nreads, (unsigned long long)packed_bytes);
    const ResultPriv *rp;
    const int chk = pairs_check_resident(c, res, "hsk_result_strands", &rp); if (chk) return chk;
    if (rid_base < 0 || nreads > (1ULL << 31) || (u64)rid_base + nreads > (1ULL << 31))
        return fail(c, HSK_ERR_INVALID_ARG, "hsk_result_strands: read ids [%lld, %lld + %llu) do not lie below 2^31 (bit 63 of an oriented key must be free)", (long long)rid_base, (long long)rid_base, (unsigned long long)nreads);
    if (reads_on_device && ((uintptr_t)packed & 3) != 0) return fail(c, HSK_ERR_INVALID_ARG, "hsk_result_strands: packed must be 4-byte aligned on the device");
    StrandsPriv *sp = new StrandsPriv();
    const int rc = ApiCall(c, "hsk_result_strands").run([&] { return strands_impl(c, rp, res->nw, res->ntasks, packed, packed_bytes, roff, rlen, nreads, rid_base, reads_on_device != 0, out, sp); });
    if (rc != HSK_OK) {                                   // (the device blocks went back with the call's rollback)
        delete sp;
        memset(out, 0, sizeof *out);
        return rc;
    }
    out->priv = sp;
    return HSK_OK;
}

extern "C" int hsk_strands_task(const hsk_strands *s, int32_t task, const void **bits_dev, uint64_t *npay)
{
    if (!s || !s->priv || task < 0 || task >= s->ntasks) return HSK_ERR_INVALID_ARG;
    const StrandsPriv *sp = (const StrandsPriv *)s->priv;
    if (bits_dev) *bits_dev = sp->npay[task] ? sp->bits + sp->word0[task] : nullptr;
    if (npay) *npay = sp->npay[task];
    return HSK_OK;
}

extern "C" void hsk_strands_free(hsk_ctx *c, hsk_strands *s)
{
    if (!s) return;
    StrandsPriv *sp = (StrandsPriv *)s->priv;
    if (sp) {
        if (c) c->pool.release(sp->bits);
        delete sp;
    }
    memset(s, 0, sizeof *s);
}
