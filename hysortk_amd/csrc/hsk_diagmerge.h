// hsk_diagmerge.h -- two-way merge of all-bins row lists of the read pairs by diagonal, in HBM (device; host: hsk_host_pairdiag.h).
//
// A row is six u64 words { key, support, bin, support, first, last } (include/hsk.h: hsk_pair_diags, all_bins).  A list is ascending by
// (key, bin) -- two unsigned 64-bit words -- and holds a (key, bin) at most once.  The merge of lists A and B is ascending with one row per
// (key, bin); a (key, bin) of both lists gives one JOINED row: support (and shared, the same number) = the sum, first = the unsigned
// minimum, last = the unsigned maximum.  min_support (the final merge only) drops the rows whose joined support is below it; the rows
// before that filter are counted (hsk_pair_diags::bins), and so are the distinct keys among them (hsk_pair_diags::keys).
//
// The kernel is pair_merge_kernel (hsk_pairmerge.h: merge path, the tie rule that puts A's copy in front of B's, ownership by A's copy with
// look-behind and look-ahead, bisection in LDS, a workgroup scan, no atomics) with these differences:
//   - "comes before" is on (key, bin): dm_before.  Every search, in HBM and in LDS, reads two words.
//   - a row comes in as three 16-byte vectors { key, support } { bin, support } { first, last }; LDS keeps five words of it (support once).
//     COUNT loads the first two vectors of a row only.
//   - COUNT also counts the KEY HEADS: the rows (before min_support) whose key differs from the key at the position in front of them.
//     For the tile's first position that is the later of A[a0 - 1] and B[b0 - 1]; both are at or below the row, so the row is a head
//     exactly when neither has its key.  A[a0 - 1] is the look-behind; the key of B[b0 - 1] is one more word.
//
// The parts that need no HIP -- dm_before, the merge-path split dm_split, the join rule dm_join -- are shared with the CPU test
// (tests/diagmerge_test.cpp), as hsk_diagbin.h's are.
#pragma once
#include "hsk_diagbin.h"

namespace hsk {

constexpr int DM_ROW_WORDS = 6;

// does (ka, ba) come before (kb, bb)?  two unsigned words
HSK_DB_FN bool dm_before(uint64_t ka, uint64_t ba, uint64_t kb, uint64_t bb) { return ka < kb || (ka == kb && ba < bb); }

// The number of A rows among the first d positions of the merged sequence (0 <= d <= na + nb): the smallest i for which A[i] does not
// come before or tie with B[d - 1 - i] (a tie puts A's copy in front).  The result lies in [max(d - nb, 0), min(d, na)] whatever the rows hold.
HSK_DB_FN uint64_t dm_split(const uint64_t *a, uint64_t na, const uint64_t *b, uint64_t nb, uint64_t d)
{
    uint64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);      // mid < na, and 0 <= d - 1 - mid < nb
        const uint64_t *ra = a + mid * DM_ROW_WORDS, *rb = b + (d - 1 - mid) * DM_ROW_WORDS;
        if (!dm_before(rb[0], rb[2], ra[0], ra[2])) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the joined row of two rows with one (key, bin): (sup, first, last) takes (sup2, first2, last2) in
HSK_DB_FN void dm_join(uint64_t &sup, uint64_t &first, uint64_t &last, uint64_t sup2, uint64_t first2, uint64_t last2)
{
    sup += sup2;
    first = first2 < first ? first2 : first;
    last = last2 > last ? last2 : last;
}

} // namespace hsk

#if defined(__HIPCC__)
#include "hsk_device.h"
#include "hsk_pairmerge.h"

namespace hsk {

constexpr int DM_THREADS = PM_THREADS;
constexpr int DM_TILE = 512;                             // positions of the merged sequence per workgroup (why not 1024)
constexpr int DM_PPT = DM_TILE / DM_THREADS;
constexpr int DM_ROWS = DM_TILE + 2;                     // + look-behind + look-ahead
static_assert((DM_TILE & (DM_TILE - 1)) == 0 && DM_TILE <= 4096 && DM_TILE % DM_THREADS == 0, "tile of the merge");
static_assert(DM_THREADS == 256, "the workgroup scan is block_excl_scan_256");

struct DiagMergeArgs {
    const u64 *a, *b;        // na / nb rows of six words, 16-byte aligned
    u64 na, nb;
    u32 min_support;
    u64 *tile_cnt;           // COUNT out / EMIT in (after the scan: the tile's first row)
    u64 *tile_keys;          // COUNT out: key heads of the tile before min_support
    u64 *tile_bins;          // COUNT out: rows of the tile before min_support
    u64 *rows;               // EMIT
};

template <bool EMIT>
__global__ __launch_bounds__(DM_THREADS) void diag_merge_kernel(DiagMergeArgs p)
{
    // row i of the A side lies at index i - (a0 - 1): [0] is the look-behind; the B side follows at bbase, the look-ahead last
    // One block of LDS, word w of row i at [w * DM_ROWS + i], and the staging and the stores below pick w by arithmetic.  (Five arrays and a
    // three-way branch on q % 3 were compiled into two merged LDS stores of which the second wrote v.x again for the third vector: `last`
    // came out as `first`.  hipcc of ROCm 7.2, -O3, gfx950; the code object is checked by the tests' exact rows.)
    enum { W_KEY = 0, W_SUP = 1, W_BIN = 2, W_FI = 3, W_LA = 4 };
    __shared__ u64 s_w[(EMIT ? 5 : 3) * DM_ROWS];
    u64 *const s_key = s_w + W_KEY * DM_ROWS, *const s_sup = s_w + W_SUP * DM_ROWS, *const s_bin = s_w + W_BIN * DM_ROWS;
    u64 *const s_fi = s_w + (EMIT ? W_FI : 0) * DM_ROWS, *const s_la = s_w + (EMIT ? W_LA : 0) * DM_ROWS;      // (COUNT never touches them)
    __shared__ u16 s_src[DM_TILE];
    __shared__ u64 s_cut[2];
    __shared__ u32 s_scr[8];
    const int tid = threadIdx.x;
    const u64 total = p.na + p.nb;
    const u64 d0 = (u64)blockIdx.x * DM_TILE, d1 = d0 + DM_TILE < total ? d0 + DM_TILE : total;
    if (tid < 2) s_cut[tid] = dm_split(p.a, p.na, p.b, p.nb, tid ? d1 : d0);
    __syncthreads();
    const u64 a0 = s_cut[0];
    u64 a1 = s_cut[1];
    {   // Ascending lists give a0 <= a1 <= a0 + (d1 - d0).  Lists that break the contract give wrong rows, never a share outside the lists:
        // a1 is held to that range (which meets dm_split's own [d1 - nb, min(d1, na)] whatever the rows are).
        const u64 lo = a0 > (d1 > p.nb ? d1 - p.nb : 0) ? a0 : (d1 > p.nb ? d1 - p.nb : 0);
        u64 hi = a0 + (d1 - d0); if (hi > p.na) hi = p.na; if (hi > d1) hi = d1;
        a1 = a1 < lo ? lo : a1 > hi ? hi : a1;
    }
    const u64 b0 = d0 - a0, b1 = d1 - a1;
    const u32 nap = (u32)(a1 - a0), nbp = (u32)(b1 - b0), nt = nap + nbp;      // nt = d1 - d0 <= DM_TILE
    const bool behind = a0 > 0, ahead = b1 < p.nb;
    const u32 bbase = 1 + nap, la = bbase + nbp;         // la <= DM_TILE + 1 < DM_ROWS
    // COUNT: the key in front of the tile's first B row (the same word for every lane; the tile's first position uses it)
    u64 kb_behind = 0;
    const bool b_behind = !EMIT && b0 > 0;
    if (b_behind) kb_behind = p.b[(b0 - 1) * DM_ROW_WORDS];

    // ---- stage: vector q of a side is word pair (q % 3) of its row q / 3 --------------------------------------------------
    {
        const u32 skip = behind ? 0 : 1;                 // without a look-behind index 0 stays empty
        const pm_v2 *ga = (const pm_v2 *)(p.a + (a0 - (behind ? 1 : 0)) * DM_ROW_WORDS);
        const u32 va = (nap + (behind ? 1 : 0)) * 3;
        for (u32 q = tid; q < va; q += DM_THREADS) {
            const u32 r0 = q / 3, w = q - r0 * 3, r = skip + r0;
            if (!EMIT && w == 2) continue;               // COUNT needs no first / last
            const pm_v2 v = ga[q];
            s_w[(w == 0 ? W_KEY : w == 1 ? W_BIN : W_FI) * DM_ROWS + r] = v.x;
            if (w != 1) s_w[(w == 0 ? W_SUP : W_LA) * DM_ROWS + r] = v.y;
        }
        const pm_v2 *gb = (const pm_v2 *)(p.b + b0 * DM_ROW_WORDS);
        const u32 vb = (nbp + (ahead ? 1 : 0)) * 3;
        for (u32 q = tid; q < vb; q += DM_THREADS) {
            const u32 r0 = q / 3, w = q - r0 * 3, r = bbase + r0;
            if (!EMIT && w == 2) continue;               // COUNT needs no first / last
            const pm_v2 v = gb[q];
            s_w[(w == 0 ? W_KEY : w == 1 ? W_BIN : W_FI) * DM_ROWS + r] = v.x;
            if (w != 1) s_w[(w == 0 ? W_SUP : W_LA) * DM_ROWS + r] = v.y;
        }
    }
    __syncthreads();

    // ---- every row's position inside the tile ----------------------------------------------------------------------------------
    for (u32 e = tid; e < nt; e += DM_THREADS) {
        u32 pos, idx;
        if (e < nap) {                                   // A[a0 + e]: behind the B rows that come before it
            idx = 1 + e;
            const u64 k = s_key[idx], b = s_bin[idx];
            u32 lo = 0, hi = nbp;
            while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (dm_before(s_key[bbase + mid], s_bin[bbase + mid], k, b)) lo = mid + 1; else hi = mid; }
            pos = e + lo;
        } else {                                         // B[b0 + j]: behind the A rows that come before it or tie with it
            const u32 j = e - nap;
            idx = bbase + j;
            const u64 k = s_key[idx], b = s_bin[idx];
            u32 lo = 0, hi = nap;
            while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (!dm_before(k, b, s_key[1 + mid], s_bin[1 + mid])) lo = mid + 1; else hi = mid; }
            pos = j + lo;
        }
        s_src[pos] = (u16)idx;                           // (pos < nt: the positions of the tile's rows are a permutation of 0 .. nt - 1)
    }
    __syncthreads();

    // ---- DM_PPT consecutive positions per lane: dropped, joined, kept -----------------------------------------------------------
    u64 rk[DM_PPT], rb[DM_PPT], rs[DM_PPT], rf[EMIT ? DM_PPT : 1], rl[EMIT ? DM_PPT : 1];
    u32 nbins = 0, nheads = 0, nkept = 0, keptm = 0;
    // (s_src is a permutation for lists that keep the contract; whatever it holds, the index stays inside the staged rows)
    const auto src = [&](u32 q) -> u32 { const u32 v = s_src[q]; return v < la ? v : la; };
#pragma unroll
    for (int i = 0; i < DM_PPT; ++i) {
        const u32 pos = (u32)tid * DM_PPT + i;
        rk[i] = 0; rb[i] = 0; rs[i] = 0;
        if (EMIT) { rf[EMIT ? i : 0] = 0; rl[EMIT ? i : 0] = 0; }
        if (pos >= nt) continue;
        const u32 idx = src(pos);
        const u64 k = s_key[idx], bn = s_bin[idx];
        u64 sup = s_sup[idx], f = 0, l = 0;
        const u32 pv = pos > 0 ? src(pos - 1) : 0;       // the position in front: inside the tile, or A's look-behind
        const bool has_pv = pos > 0 || behind;
        if (idx >= bbase) {                              // a B row: dropped where the position before it holds its (key, bin) (A's copy owns the row)
            if (has_pv && s_key[pv] == k && s_bin[pv] == bn) continue;
            if (EMIT) { f = s_fi[EMIT ? idx : 0]; l = s_la[EMIT ? idx : 0]; }
        } else {                                         // an A row: joins the next position's row where that holds its (key, bin)
            const bool has = pos + 1 < nt || ahead;
            const u32 nx = pos + 1 < nt ? src(pos + 1) : la;
            const bool join = has && s_key[nx] == k && s_bin[nx] == bn;
            if (EMIT) { f = s_fi[EMIT ? idx : 0]; l = s_la[EMIT ? idx : 0]; }
            if (join) dm_join(sup, f, l, s_sup[nx], EMIT ? s_fi[EMIT ? nx : 0] : 0, EMIT ? s_la[EMIT ? nx : 0] : 0);
        }
        ++nbins;
        if (!EMIT) {                                     // a key head: no row in front of it has its key
            bool head = !(has_pv && s_key[pv] == k);
            if (pos == 0 && b_behind && kb_behind == k) head = false;
            nheads += head ? 1u : 0u;
        }
        if (sup >= (u64)p.min_support) {
            rk[i] = k; rb[i] = bn; rs[i] = sup; keptm |= 1u << i; ++nkept;
            if (EMIT) { rf[EMIT ? i : 0] = f; rl[EMIT ? i : 0] = l; }
        }
    }
    u32 tot_kept, tot_bins = 0, tot_heads = 0;
    u32 slot = block_excl_scan_256<u32>(nkept, s_scr, &tot_kept);       // (barriers inside: every lane has read the staged rows it needs)
    if (!EMIT) {
        (void)block_excl_scan_256<u32>(nbins, s_scr, &tot_bins);
        (void)block_excl_scan_256<u32>(nheads, s_scr, &tot_heads);
        if (tid == 0) { p.tile_cnt[blockIdx.x] = tot_kept; p.tile_keys[blockIdx.x] = tot_heads; p.tile_bins[blockIdx.x] = tot_bins; }
        return;
    }

    // ---- the kept rows go back into LDS at their slots, and out 16 bytes per lane ----------------------------------------------
    __syncthreads();
#pragma unroll
    for (int i = 0; i < DM_PPT; ++i) {
        if (!(keptm & (1u << i))) continue;
        s_key[slot] = rk[i]; s_bin[slot] = rb[i]; s_sup[slot] = rs[i]; s_fi[EMIT ? slot : 0] = rf[EMIT ? i : 0]; s_la[EMIT ? slot : 0] = rl[EMIT ? i : 0];
        ++slot;
    }
    __syncthreads();
    pm_v2 *go = (pm_v2 *)(p.rows + p.tile_cnt[blockIdx.x] * DM_ROW_WORDS);
    for (u32 q = tid; q < tot_kept * 3; q += DM_THREADS) {
        const u32 r = q / 3, w = q - r * 3;
        pm_v2 v;
        v.x = s_w[(w == 0 ? W_KEY : w == 1 ? W_BIN : W_FI) * DM_ROWS + r];
        v.y = s_w[(w == 2 ? W_LA : W_SUP) * DM_ROWS + r];
        go[q] = v;
    }
}

} // namespace hsk
#endif
