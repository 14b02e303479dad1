// hsk_pairmerge.h -- two-way merge of read-pair row lists in HBM (device; host: hsk_host_pairs.h).
//
// A row is four u64 words { key, shared, first, last } (include/hsk.h: hsk_pairs).  A list is ascending by key as unsigned 64-bit
// numbers and holds a key at most once.  The merge of lists A and B is ascending with one row per key; a key of both lists gives one
// JOINED row: shared = the sum, first = the unsigned minimum, last = the unsigned maximum.  min_shared (the final merge only) drops the
// rows whose joined shared is below it; the rows before that filter are counted too (hsk_pairs::keys).
//
//   Merge path.  The MERGED SEQUENCE is all na + nb rows in key order, A's copy of a key in front of B's (the tie rule).  Workgroup t
//   takes positions [t * PM_TILE, (t + 1) * PM_TILE) of it.  Position d splits into (ai, d - ai) with ai = the number of A rows among
//   the first d: the smallest i for which A[i] does not come before B[d - 1 - i], found by bisection over the keys in HBM (two lanes: the
//   tile's first and last diagonal).  The tile's share is A[a0, a1) and B[b0, b1), at most PM_TILE rows together.
//
//   Who owns a key of both lists.  By the tie rule B's copy is the position right behind A's copy.  The row belongs to the tile that
//   holds A'S COPY: it joins the next position's row, and where A's copy is the tile's last position that row is B[b1], one row past
//   the tile's share -- the tile stages it as well (the look-ahead).  B's copy is dropped by whoever holds it: it is the B row whose
//   previous position has its key, and for the tile's first position that is A[a0 - 1], staged too (the look-behind).  Both passes run
//   the same code on the same splits, so COUNT and EMIT agree wherever the diagonal falls.
//
//   In LDS.  A[a0 - 1 .. a1) and B[b0 .. b1] come in as 16-byte vectors, consecutive lanes on consecutive addresses, and are laid out
//   word by word (keys apart from the rest: the searches walk keys only).  Every row finds its position by one bisection in the other
//   list's share: A[i] goes to i + (B rows below its key), B[j] to j + (A rows at or below its key).  s_src[position] = where the row
//   lies.  Then every lane takes PM_PPT consecutive positions: dropped / joined by the neighbours' keys, the filter, a workgroup scan of
//   the kept rows.  COUNT leaves rows and keys per tile; count_scan_kernel (hsk_count.h) turns the rows into the tile's first output
//   row; EMIT builds the rows in registers, writes them back into LDS at their slots (the staged rows are dead by then) and stores them
//   16 bytes per lane.  No atomics: the output is ordered by construction.
//
// The kernel moves 32 B per input row in each pass and 32 B per output row; COUNT reads only the first half of every row, which costs the
// same lines of HBM.
#pragma once
#include "hsk_device.h"
#include "hsk_pairplan.h"

namespace hsk {

constexpr int PM_THREADS = 256;
constexpr int PM_TILE = 1024;                            // positions of the merged sequence per workgroup: a power of two, 4096 at most
constexpr int PM_PPT = PM_TILE / PM_THREADS;
constexpr int PM_ROWS = PM_TILE + 2;                     // + look-behind + look-ahead
static_assert((PM_TILE & (PM_TILE - 1)) == 0 && PM_TILE <= 4096 && PM_TILE % PM_THREADS == 0, "tile of the merge");

struct PairMergeArgs {
    const u64 *a, *b;        // na / nb rows of four words, 16-byte aligned
    u64 na, nb;
    u32 min_shared;
    u64 *tile_cnt;           // COUNT out / EMIT in (after the scan: the tile's first row)
    u64 *tile_keys;          // COUNT out: rows of the tile before min_shared
    u64 *rows;               // EMIT
};

typedef unsigned long long pm_v2 __attribute__((ext_vector_type(2)));

// the number of A rows among the first d positions of the merged sequence (0 <= d <= na + nb)
__device__ __forceinline__ u64 pm_split(const u64 *a, u64 na, const u64 *b, u64 nb, u64 d)
{
    u64 lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);           // mid < na, and 0 <= d - 1 - mid < nb
        if (a[mid * 4] <= b[(d - 1 - mid) * 4]) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <bool EMIT>
__global__ __launch_bounds__(PM_THREADS) void pair_merge_kernel(PairMergeArgs p)
{
    // row i of the A side lies at index i - (a0 - 1): [0] is the look-behind; the B side follows at bbase, the look-ahead last
    __shared__ u64 s_key[PM_ROWS], s_sh[PM_ROWS];
    __shared__ u64 s_fi[EMIT ? PM_ROWS : 1], s_la[EMIT ? PM_ROWS : 1];
    __shared__ u16 s_src[PM_TILE];
    __shared__ u64 s_cut[2];
    __shared__ u32 s_scr[8];
    const int tid = threadIdx.x;
    const u64 total = p.na + p.nb;
    const u64 d0 = (u64)blockIdx.x * PM_TILE, d1 = d0 + PM_TILE < total ? d0 + PM_TILE : total;
    if (tid < 2) s_cut[tid] = pm_split(p.a, p.na, p.b, p.nb, tid ? d1 : d0);
    __syncthreads();
    const u64 a0 = s_cut[0];
    u64 a1 = s_cut[1];
    {   // Ascending lists give a0 <= a1 <= a0 + (d1 - d0).  Lists that break the contract give wrong rows, never a share outside the lists:
        // a1 is held to that range (which meets pm_split's own [d1 - nb, min(d1, na)] whatever the keys are).
        const u64 lo = a0 > (d1 > p.nb ? d1 - p.nb : 0) ? a0 : (d1 > p.nb ? d1 - p.nb : 0);
        u64 hi = a0 + (d1 - d0); if (hi > p.na) hi = p.na; if (hi > d1) hi = d1;
        a1 = a1 < lo ? lo : a1 > hi ? hi : a1;
    }
    const u64 b0 = d0 - a0, b1 = d1 - a1;
    const u32 nap = (u32)(a1 - a0), nbp = (u32)(b1 - b0), nt = nap + nbp;      // nt = d1 - d0 <= PM_TILE
    const bool behind = a0 > 0, ahead = b1 < p.nb;
    const u32 bbase = 1 + nap, la = bbase + nbp;         // la <= PM_TILE + 1 < PM_ROWS

    // ---- stage: vector q of a side is word pair (q & 1) of its row q >> 1 -------------------------------------------------
    {
        const u32 skip = behind ? 0 : 1;                 // without a look-behind index 0 stays empty
        const pm_v2 *ga = (const pm_v2 *)(p.a + (a0 - (behind ? 1 : 0)) * 4);
        const u32 va = (nap + (behind ? 1 : 0)) * 2;
        for (u32 q = tid; q < va; q += PM_THREADS) {
            const u32 r = skip + (q >> 1);
            if (!(q & 1)) { const pm_v2 v = ga[q]; s_key[r] = v.x; s_sh[r] = v.y; }
            else if (EMIT) { const pm_v2 v = ga[q]; s_fi[EMIT ? r : 0] = v.x; s_la[EMIT ? r : 0] = v.y; }
        }
        const pm_v2 *gb = (const pm_v2 *)(p.b + b0 * 4);
        const u32 vb = (nbp + (ahead ? 1 : 0)) * 2;
        for (u32 q = tid; q < vb; q += PM_THREADS) {
            const u32 r = bbase + (q >> 1);
            if (!(q & 1)) { const pm_v2 v = gb[q]; s_key[r] = v.x; s_sh[r] = v.y; }
            else if (EMIT) { const pm_v2 v = gb[q]; s_fi[EMIT ? r : 0] = v.x; s_la[EMIT ? r : 0] = v.y; }
        }
    }
    __syncthreads();

    // ---- every row's position inside the tile ----------------------------------------------------------------------------------
    for (u32 e = tid; e < nt; e += PM_THREADS) {
        u32 pos, idx;
        if (e < nap) {                                   // A[a0 + e]: behind the B rows below its key
            idx = 1 + e;
            const u64 k = s_key[idx];
            u32 lo = 0, hi = nbp;
            while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (s_key[bbase + mid] < k) lo = mid + 1; else hi = mid; }
            pos = e + lo;
        } else {                                         // B[b0 + j]: behind the A rows at or below its key
            const u32 j = e - nap;
            idx = bbase + j;
            const u64 k = s_key[idx];
            u32 lo = 0, hi = nap;
            while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (s_key[1 + mid] <= k) lo = mid + 1; else hi = mid; }
            pos = j + lo;
        }
        s_src[pos] = (u16)idx;                           // (pos < nt: the positions of the tile's rows are a permutation of 0 .. nt - 1)
    }
    __syncthreads();

    // ---- PM_PPT consecutive positions per lane: dropped, joined, kept -----------------------------------------------------------
    u64 rk[PM_PPT], rs[PM_PPT], rf[EMIT ? PM_PPT : 1], rl[EMIT ? PM_PPT : 1];
    u32 nkeys = 0, nkept = 0, keptm = 0;
    // (s_src is a permutation for lists that keep the contract; whatever it holds, the index stays inside the staged rows)
    const auto src = [&](u32 q) -> u32 { const u32 v = s_src[q]; return v < la ? v : la; };
#pragma unroll
    for (int i = 0; i < PM_PPT; ++i) {
        const u32 pos = (u32)tid * PM_PPT + i;
        rk[i] = 0; rs[i] = 0;
        if (EMIT) { rf[EMIT ? i : 0] = 0; rl[EMIT ? i : 0] = 0; }
        if (pos >= nt) continue;
        const u32 idx = src(pos);
        const u64 k = s_key[idx];
        u64 sh = s_sh[idx];
        if (idx >= bbase) {                              // a B row: dropped where the position before it holds its key (A's copy owns the row)
            const bool has = pos > 0 || behind;
            const u32 pv = pos > 0 ? src(pos - 1) : 0;
            if (has && s_key[pv] == k) continue;
            if (EMIT) { rf[EMIT ? i : 0] = s_fi[EMIT ? idx : 0]; rl[EMIT ? i : 0] = s_la[EMIT ? idx : 0]; }
        } else {                                         // an A row: joins the next position's row where that holds its key
            const bool has = pos + 1 < nt || ahead;
            const u32 nx = pos + 1 < nt ? src(pos + 1) : la;
            const bool join = has && s_key[nx] == k;
            if (join) sh += s_sh[nx];
            if (EMIT) {
                u64 f = s_fi[EMIT ? idx : 0], l = s_la[EMIT ? idx : 0];
                if (join) { const u64 f2 = s_fi[EMIT ? nx : 0], l2 = s_la[EMIT ? nx : 0]; f = f2 < f ? f2 : f; l = l2 > l ? l2 : l; }
                rf[EMIT ? i : 0] = f; rl[EMIT ? i : 0] = l;
            }
        }
        ++nkeys;
        if (sh >= (u64)p.min_shared) { rk[i] = k; rs[i] = sh; keptm |= 1u << i; ++nkept; }
    }
    u32 tot_kept, tot_keys = 0;
    u32 slot = block_excl_scan_256<u32>(nkept, s_scr, &tot_kept);       // (barriers inside: every lane has read the staged rows it needs)
    if (!EMIT) {
        (void)block_excl_scan_256<u32>(nkeys, s_scr, &tot_keys);
        if (tid == 0) { p.tile_cnt[blockIdx.x] = tot_kept; p.tile_keys[blockIdx.x] = tot_keys; }
        return;
    }

    // ---- the kept rows go back into LDS at their slots, and out 16 bytes per lane ----------------------------------------------
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PM_PPT; ++i) {
        if (!(keptm & (1u << i))) continue;
        s_key[slot] = rk[i]; s_sh[slot] = rs[i]; s_fi[EMIT ? slot : 0] = rf[EMIT ? i : 0]; s_la[EMIT ? slot : 0] = rl[EMIT ? i : 0];
        ++slot;
    }
    __syncthreads();
    pm_v2 *go = (pm_v2 *)(p.rows + p.tile_cnt[blockIdx.x] * 4);
    for (u32 q = tid; q < tot_kept * 2; q += PM_THREADS) {
        const u32 r = q >> 1;
        pm_v2 v;
        if (q & 1) { v.x = s_fi[EMIT ? r : 0]; v.y = s_la[EMIT ? r : 0]; } else { v.x = s_key[r]; v.y = s_sh[r]; }
        go[q] = v;
    }
}

// one lane: every cut of the range's entries under the budget (hsk_pairplan.h), and the record offset at each cut
struct PairPlanArgs {
    const u64 *off; u64 nent, max_records;
    u64 *cut;                // cap pairs { cut, off[cut] }
    u64 cap;
    u64 *ncut;
};

__global__ void pair_plan_kernel(PairPlanArgs p)
{
    if (blockIdx.x || threadIdx.x) return;
    u64 n = 0, from = 0;
    while (from < p.nent && n < p.cap) {
        from = pair_plan_next(p.off, p.nent, from, p.max_records);
        p.cut[2 * n] = from; p.cut[2 * n + 1] = p.off[from];
        ++n;
    }
    p.ncut[0] = from < p.nent ? ~0ULL : n;               // (the bound of the cuts did not hold: never, by hsk_pairplan.h's argument)
}

} // namespace hsk
