// hsk_pairdiag.h -- read pairs by diagonal: the seed bins of every oriented read pair and the best-supported one (device).
//
// hsk_result_pair_diagonals (include/hsk.h) takes the records of hsk_result_pairs_oriented -- key o << 63 | rid_a << 32 | rid_b, value
// pos_a << 32 | pos_b -- and groups them by (key, diagonal bin) (hsk_diagbin.h).  The expansion (pair_expand_kernel<true, true>, hsk_pairs.h)
// writes a two-word key, the pair key in word 1 and the sort word of the bin in word 0; the library's radix sort orders the records by it.
//
//   diag_maxpos_kernel   a bound of every position the range's records can hold: the largest pos among the payload slots of the entries
//                        that have records (the gap slots of filtered k-mers are not read: nothing says what they hold).  One lane per
//                        entry walks its slice; one atomicMax per workgroup.  The sort word is taken relative to this bound.
//   diag_reduce_kernel   level 1: runs of equal (key, word 0) become BIN ROWS of six words { key, support, bin, support, first, last },
//                        the all-bins row of the ABI.  The steps of pair_reduce_kernel (hsk_runmask.h), a count pass, count_scan_kernel,
//                        an emit pass; the compare is on two words, which every lane holds in registers (its record and the one before
//                        it: neighbouring 16-byte loads), so that LDS holds the values only.  The zero-key run is self_records.  Per
//                        tile it also counts the key heads (`keys`) and the runs before min_support (`bins`).
//   diag_select_kernel   level 2: runs of equal key over the bin rows become one row { key, sum of support, bin, support, first, last }
//                        of the bin with the largest support, the smallest such bin on a tie (diag_better).  The same steps; what a
//                        lane keeps of a run is (sum, best support, best bin, row of the best), reduced over the workgroup for the
//                        tile's last key.  No atomics.  first / last are read from the winning bin row.  Rows leave as three 16-byte
//                        stores, in key order by popcount prefix; min_support is applied after the selection.
#pragma once
#include "hsk_device.h"
#include "hsk_count.h"
#include "hsk_runmask.h"
#include "hsk_pairs.h"
#include "hsk_diagbin.h"

namespace hsk {

typedef unsigned long long v2u64d __attribute__((ext_vector_type(2)));
constexpr int DIAG_ROW_WORDS = 6;
enum { DIAG_STAT_MAXPOS = 5, DIAG_STAT_BINS = 6 };       // words of the pair stage's stat block (PAIR_STAT_*) that only this call uses
static_assert(DIAG_STAT_MAXPOS > PAIR_STAT_ERR && DIAG_STAT_BINS < PAIR_STAT_WORDS, "the stat block has PAIR_STAT_WORDS words");

struct DiagMaxArgs {
    const PairTask *tasks;
    const u64 *off, *loc;    // what pair_tsum_kernel left: nent + 1 record offsets, nent payload locations (every slice checked against its task)
    u64 nent; int nw;
    u64 *maxpos;             // zero before the launch
};

__global__ __launch_bounds__(PAIR_THREADS) void diag_maxpos_kernel(DiagMaxArgs a)
{
    __shared__ u32 s_m[PAIR_THREADS / WAVE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u32 m = 0;
    for (u64 g = (u64)blockIdx.x * PAIR_THREADS + tid; g < a.nent; g += (u64)gridDim.x * PAIR_THREADS) {
        if (a.off[g + 1] == a.off[g]) continue;           // no records: cnt < 2
        const u64 L = a.loc[g];
        const PairTask &tk = a.tasks[L >> PAIR_LOC_SHIFT];
        const u64 first = L & ((1ULL << PAIR_LOC_SHIFT) - 1);
        const u64 cnt = tk.entries[(g - tk.ent_base) * (u64)(a.nw + 1) + a.nw];
        for (u64 i = 0; i < cnt; ++i) { const u32 p = tk.pos[first + i]; m = p > m ? p : m; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u32 x = __shfl_xor(m, o, WAVE); m = x > m ? x : m; }
    if (lane == 0) s_m[wave] = m;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < PAIR_THREADS / WAVE; ++w) m = s_m[w] > m ? s_m[w] : m;
        if (m) atomicMax((unsigned long long *)a.maxpos, (unsigned long long)m);
    }
}

// ---- level 1: records -> bin rows ----------------------------------------------------------------------------------------------------
constexpr int DR_PPT = 8, DR_TILE = PAIR_THREADS * DR_PPT, DR_WORDS = DR_TILE / 64;
constexpr int DR_AHEAD = 4;                              // records per lane and step of the read-ahead

struct DiagReduceArgs {
    const u64 *keys;         // sorted: record i = { word 0: sort word of the bin, word 1: pair key } at [2 i]
    const u64 *vals;         // n
    u64 n;
    u64 diag_w; const u64 *maxpos;
    u32 min_support;         // all_bins: the caller's; else 1 (the selection comes first)
    u64 *tile_cnt;           // COUNT out / EMIT in (after the scan: the tile's first row)
    u64 *tile_keys;          // COUNT out: heads of key runs (key != 0) of the tile
    u64 *tile_bins;          // COUNT out: runs of the tile with a key other than 0, before min_support
    u64 *rows;               // EMIT: { key, support, bin, support, first, last }
    u64 *stats;              // COUNT: [PAIR_STAT_SELF] records of the zero-key run
};

template <bool EMIT>
__global__ __launch_bounds__(PAIR_THREADS) void diag_reduce_kernel(DiagReduceArgs a)
{
    __shared__ u64 s_v[EMIT ? DR_TILE : 1];
    __shared__ u64 s_head[DR_WORDS], s_keep[DR_WORDS];
    __shared__ u32 s_pre[DR_WORDS + 1];
    __shared__ u64 s_red[4][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 base = (u64)blockIdx.x * DR_TILE;
    const u32 tn = (u32)(a.n - base < (u64)DR_TILE ? a.n - base : (u64)DR_TILE);
    const u64 obase = EMIT ? a.tile_cnt[blockIdx.x] : 0;
    const v2u64d *kk = (const v2u64d *)a.keys;
    u64 k0[DR_PPT], k1[DR_PPT];
    bool head[DR_PPT], khead[DR_PPT];
#pragma unroll
    for (int j = 0; j < DR_PPT; ++j) {
        const u32 p = j * PAIR_THREADS + tid;
        head[j] = khead[j] = false; k0[j] = k1[j] = 0;
        if (p < tn) {
            const v2u64d cur = kk[base + p];
            k0[j] = cur.x; k1[j] = cur.y;
            if (base + p == 0) head[j] = khead[j] = true;
            else { const v2u64d prev = kk[base + p - 1]; khead[j] = prev.y != cur.y; head[j] = khead[j] || prev.x != cur.x; }
            if (EMIT) s_v[p] = a.vals[base + p];
        }
        rm_publish(s_head, j, __ballot(head[j]));
    }
    __syncthreads();
    const int p_last = rm_last_head<DR_WORDS>(s_head);
    if (p_last < 0) { if (!EMIT && tid == 0) { a.tile_cnt[blockIdx.x] = 0; a.tile_keys[blockIdx.x] = 0; a.tile_bins[blockIdx.x] = 0; } return; }      // the tile lies inside a run that started before it

    // ---- the tile's last run: the workgroup follows it to its end --------------------------------------------------
    const v2u64d key_last = kk[base + p_last];
    // (scalars and the loop in the kernel's own text, not RunAcc and rm_follow: 64 VGPRs and occupancy 8 that way, 66 and 7 the other)
    u64 lc = 0, lmn = ~0ULL, lmx = 0;
    for (u32 i = p_last + tid; i < tn; i += PAIR_THREADS) {
        ++lc;
        if (EMIT) { const u64 v = s_v[i]; lmn = v < lmn ? v : lmn; lmx = v > lmx ? v : lmx; }
    }
    for (u64 g = base + tn;; g += (u64)PAIR_THREADS * DR_AHEAD) {
        int stop = g >= a.n;
        if (!stop) {
#pragma unroll
            for (int s = 0; s < DR_AHEAD; ++s) {
                const u64 gi = g + (u64)s * PAIR_THREADS + tid;
                if (gi >= a.n) { stop = 1; continue; }
                const v2u64d k = kk[gi];
                const u64 v = EMIT ? a.vals[gi] : 0;
                if (k.x != key_last.x || k.y != key_last.y) { stop = 1; continue; }
                ++lc;
                if (EMIT) { lmn = v < lmn ? v : lmn; lmx = v > lmx ? v : lmx; }
            }
        }
        if (__syncthreads_or(stop)) break;
    }
    RunAcc L; L.n = lc; L.mn = lmn; L.mx = lmx;
    rm_reduce_run<EMIT>(L, s_red);

    // ---- run lengths, the min_support filter --------------------------------------------------------------------------
    u64 runlen[DR_PPT];
    u32 nkeys = 0, nbins = 0;
#pragma unroll
    for (int j = 0; j < DR_PPT; ++j) {
        const u32 p = j * PAIR_THREADS + tid;
        u64 c = 0; bool real = false;
        if (head[j]) {
            c = p == (u32)p_last ? L.n : rm_next_head(s_head, p) - p;
            real = k1[j] != 0;
            if (!EMIT && !real) a.stats[PAIR_STAT_SELF] = c;
        }
        const bool keep = real && c >= a.min_support;
        runlen[j] = keep ? c : 0;
        rm_publish(s_keep, j, __ballot(keep));
        if (!EMIT) { nbins += (u32)__popcll(__ballot(real)); nkeys += (u32)__popcll(__ballot(real && khead[j])); }
    }
    __syncthreads();                                      // (s_red has been read by every wave)
    if (!EMIT && lane == 0) { s_red[wave][0] = nkeys; s_red[wave][1] = nbins; }
    __syncthreads();
    rm_prefix<DR_WORDS>(s_keep, s_pre);
    __syncthreads();
    if (!EMIT) {
        if (tid == 0) {
            a.tile_cnt[blockIdx.x] = s_pre[DR_WORDS];
            a.tile_keys[blockIdx.x] = s_red[0][0] + s_red[1][0] + s_red[2][0] + s_red[3][0];
            a.tile_bins[blockIdx.x] = s_red[0][1] + s_red[1][1] + s_red[2][1] + s_red[3][1];
        }
        return;
    }

    // ---- rows: slot = popcount prefix of the kept heads, so the list stays in (key, bin) order -------------------------
    const u64 lo_same = diag_bin_lo(0, (u32)a.maxpos[0], a.diag_w), lo_opp = diag_bin_lo(1, (u32)a.maxpos[0], a.diag_w);      // (the division once, not per row)
#pragma unroll
    for (int j = 0; j < DR_PPT; ++j) {
        const u64 c = runlen[j];
        if (!c) continue;
        const u32 p = j * PAIR_THREADS + tid;
        RunAcc r = L;
        if (p != (u32)p_last) r.span(s_v, p, (u32)c);
        v2u64d *row = (v2u64d *)(a.rows + (obase + rm_slot(s_keep, s_pre, j)) * DIAG_ROW_WORDS);
        const v2u64d r0 = {k1[j], c}, r1 = {k0[j] + ((k1[j] >> 63) ? lo_opp : lo_same), c}, r2 = {r.mn, r.mx};
        row[0] = r0; row[1] = r1; row[2] = r2;
    }
}

// ---- level 2: bin rows -> the best bin of every key ------------------------------------------------------------------------------------
constexpr int DS_PPT = 4, DS_TILE = PAIR_THREADS * DS_PPT, DS_WORDS = DS_TILE / 64;
constexpr int DS_AHEAD = 4;                              // bin rows per lane and step of the read-ahead

struct DiagSelectArgs {
    const u64 *bins;         // n rows of level 1, ascending (key, bin), every (key, bin) once
    u64 n;
    u32 min_support;
    u64 *tile_cnt;           // COUNT out / EMIT in (after the scan: the tile's first row)
    u64 *rows;               // EMIT: { key, shared, bin, support, first, last }
};

// the running choice of a lane: the sum of the supports it has seen, and the best bin among them with the row it stands in
struct DiagBest {
    u64 sum, sup, bin, row;
    __device__ __forceinline__ void clear() { sum = 0; sup = 0; bin = ~0ULL; row = 0; }      // (every bin row has support >= 1: any row beats this)
    __device__ __forceinline__ void take(u64 s, u64 b, u64 r) { sum += s; if (diag_better(s, b, sup, bin)) { sup = s; bin = b; row = r; } }
    __device__ __forceinline__ void join(u64 osum, u64 s, u64 b, u64 r) { sum += osum; if (diag_better(s, b, sup, bin)) { sup = s; bin = b; row = r; } }
};

template <bool EMIT>
__global__ __launch_bounds__(PAIR_THREADS) void diag_select_kernel(DiagSelectArgs a)
{
    __shared__ u64 s_bin[DS_TILE], s_sup[DS_TILE];
    __shared__ u64 s_head[DS_WORDS], s_keep[DS_WORDS];
    __shared__ u32 s_pre[DS_WORDS + 1];
    __shared__ u64 s_red[4][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 base = (u64)blockIdx.x * DS_TILE;
    const u32 tn = (u32)(a.n - base < (u64)DS_TILE ? a.n - base : (u64)DS_TILE);
    const u64 obase = EMIT ? a.tile_cnt[blockIdx.x] : 0;
    u64 key[DS_PPT];
    bool head[DS_PPT];
#pragma unroll
    for (int j = 0; j < DS_PPT; ++j) {
        const u32 p = j * PAIR_THREADS + tid;
        head[j] = false; key[j] = 0;
        if (p < tn) {
            const v2u64d *r = (const v2u64d *)(a.bins + (base + p) * DIAG_ROW_WORDS);
            const v2u64d r0 = r[0], r1 = r[1];
            key[j] = r0.x; s_bin[p] = r1.x; s_sup[p] = r1.y;
            head[j] = base + p == 0 || a.bins[(base + p - 1) * DIAG_ROW_WORDS] != r0.x;
        }
        rm_publish(s_head, j, __ballot(head[j]));
    }
    __syncthreads();
    const int p_last = rm_last_head<DS_WORDS>(s_head);
    if (p_last < 0) { if (!EMIT && tid == 0) a.tile_cnt[blockIdx.x] = 0; return; }      // the tile lies inside a key's bins: the tile of the key's first bin row reads them

    // ---- the tile's last key: the workgroup follows its bin rows to their end, over as many tiles as they take -----------
    const u64 key_last = a.bins[(base + p_last) * DIAG_ROW_WORDS];
    DiagBest L; L.clear();
    for (u32 i = p_last + tid; i < tn; i += PAIR_THREADS) L.take(s_sup[i], s_bin[i], base + i);
    rm_follow<DS_AHEAD>(base + tn, a.n, [&](u64 gi) {
        const v2u64d *r = (const v2u64d *)(a.bins + gi * DIAG_ROW_WORDS);
        const v2u64d r0 = r[0], r1 = r[1];
        if (r0.x != key_last) return false;
        L.take(r1.y, r1.x, gi);
        return true;
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 osum = __shfl_xor(L.sum, o, WAVE), os = __shfl_xor(L.sup, o, WAVE), ob = __shfl_xor(L.bin, o, WAVE), orow = __shfl_xor(L.row, o, WAVE);
        L.join(osum, os, ob, orow);
    }
    if (lane == 0) { s_red[wave][0] = L.sum; s_red[wave][1] = L.sup; s_red[wave][2] = L.bin; s_red[wave][3] = L.row; }
    __syncthreads();
    L.clear();
#pragma unroll
    for (int w = 0; w < 4; ++w) L.join(s_red[w][0], s_red[w][1], s_red[w][2], s_red[w][3]);

    // ---- every key that starts in the tile: its sum and its best bin; min_support after the selection -----------------------
    DiagBest best[DS_PPT];
#pragma unroll
    for (int j = 0; j < DS_PPT; ++j) {
        const u32 p = j * PAIR_THREADS + tid;
        best[j].clear();
        if (head[j]) {
            if (p == (u32)p_last) best[j] = L;
            else for (u32 q = p, e = rm_next_head(s_head, p); q < e; ++q) best[j].take(s_sup[q], s_bin[q], base + q);
        }
        rm_publish(s_keep, j, __ballot(head[j] && best[j].sup >= a.min_support));
    }
    __syncthreads();
    rm_prefix<DS_WORDS>(s_keep, s_pre);
    __syncthreads();
    if (!EMIT) { if (tid == 0) a.tile_cnt[blockIdx.x] = s_pre[DS_WORDS]; return; }

    // ---- rows: slot = popcount prefix of the kept heads, so the list stays in key order ------------------------------------
#pragma unroll
    for (int j = 0; j < DS_PPT; ++j) {
        if (!((s_keep[j * RM_WAVES + wave] >> lane) & 1)) continue;
        const v2u64d fl = ((const v2u64d *)(a.bins + best[j].row * DIAG_ROW_WORDS))[2];
        v2u64d *row = (v2u64d *)(a.rows + (obase + rm_slot(s_keep, s_pre, j)) * DIAG_ROW_WORDS);
        const v2u64d r0 = {key[j], best[j].sum}, r1 = {best[j].bin, best[j].sup};
        row[0] = r0; row[1] = r1; row[2] = fl;
    }
}

} // namespace hsk
