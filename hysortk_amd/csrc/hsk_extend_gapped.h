// hsk_extend_gapped.h -- banded, gapped x-drop extension of the seed of every diagonal row, with the reads in HBM (device; include/hsk.h:
// hsk_pair_diags_extend_gapped has the definition; hsk_gapped.h the base accessors, the cell, the best rule and the row that the kernel
// and the CPU test share; the row checks, the error block, the keep flags and the compaction are those of hsk_extend.h).
//
//   extend_gapped_kernel<LANES>   a group of LANES lanes per row (LANES = 8, 16, 32, 64: a wavefront takes 8, 4, 2 or 1 rows), bands up to
//                        LANES - 1.  Lane l holds the two diagonals ke = 2 l - LANES (even) and ke + 1 (odd): on an even antidiagonal d every
//                        lane has exactly one cell, on ke, and on an odd one on ke + 1.  The lane keeps the words of its last even and
//                        its last odd cell.  Cell (i, j) of an even d takes its diagonal predecessor from the lane's even word (d - 2),
//                        (i, j - 1) from its own odd word and (i - 1, j) from lane l - 1's odd word; on an odd d the own even word is
//                        (i - 1, j) and lane l + 1's even word is (i, j - 1): one width-limited shuffle of 64 bits per step.  i grows by one
//                        on every odd d and j on every even d, in all lanes at once: each lane shifts its 32-base windows of x and y by one
//                        base and loads them again every 64 antidiagonals (x where d % 64 == 63, y where d % 64 == 0; d is uniform).
//                        The side's best is needed by every cell of the next antidiagonal, so a lane that holds a cell above it starts
//                        a maximum over its group (taken only on antidiagonals where some lane of the wave has one) and remembers the
//                        cell; the side's (i*, j*, e*) is chosen once at the end: of the cells remembered on the last such antidiagonal
//                        the largest word, in the lowest lane (the smallest i).  A wave stops after two antidiagonals without a live
//                        cell in any of its rows, or behind the largest na + nb of its rows; cells outside a row's own reads do not
//                        exist, and a row whose cells are all dead stays dead, so the rows of a wave do not see each other.
// Every loop is bounded by na + nb; there are no spin-waits and no dependencies between workgroups; the atomics are the error counters
// and the column and cell sums.
#pragma once
#include "hsk_extend.h"
#include "hsk_gapped.h"

namespace hsk {

constexpr int EG_THREADS = 256;
// the words of the call's block (hsk_extend.h) that the gapped call uses differently: it has no long-row list
enum { EXT_STAT_CELLS = EXT_STAT_LONG, EXT_STAT_ERR_SPAN = 7 };
static_assert(EXT_STAT_ERR_SPAN > EXT_STAT_ERR_SEED && EXT_STAT_ERR_SPAN < EXT_STAT_WORDS, "a word of its own");

struct GappedArgs {
    ExtendArgs e;                                        // rows, reads, K, match, the filter, out, keep, stat (mismatch, xdrop, wave_span, the list: unused)
    GpScore sc;
};

template <int LANES>
__device__ __forceinline__ int32_t eg_group_max(int32_t v)
{
#pragma unroll
    for (int o = LANES / 2; o > 0; o >>= 1) { const int32_t n = __shfl_xor(v, o, LANES); v = n > v ? n : v; }
    return v;
}

template <int LANES>
__device__ __forceinline__ int64_t eg_group_max64(int64_t v)
{
#pragma unroll
    for (int o = LANES / 2; o > 0; o >>= 1) { const int64_t n = __shfl_xor(v, o, LANES); v = n > v ? n : v; }
    return v;
}

// one side of the rows of a wave; every lane of a group returns its row's result.  ok: the lane's row is there and valid (else *p is not used)
template <int LANES>
__device__ __forceinline__ GpSide eg_side(const GappedArgs &a, const XdPair &p, bool ok, bool right, int gl)
{
    const GpScore sc = a.sc;
    u32 na = 0, nb = 0;
    if (ok) gp_lengths(p, right, na, nb);
    const int32_t ke = 2 * gl - LANES;
    const bool in_e = ok && ke >= -sc.band && ke <= sc.band, in_o = ok && ke + 1 >= -sc.band && ke + 1 <= sc.band;
    const bool reads = in_e || in_o;
    const u32 dmax = (u32)eg_group_max<WAVE>((int32_t)(na + nb));      // (below 2^22)
    int64_t even = ok && gl == LANES / 2 ? gp_pack(0, 0) : GP_DEAD, odd = GP_DEAD;
    u64 wx = 0, wy = 0;
    if (reads) { wx = gp_x32(a.e.packed, a.e.packed_bytes, p, right, ke / 2); wy = gp_y32(a.e.packed, a.e.packed_bytes, p, right, -(ke / 2)); }
    // the cell of diagonal k is there on the antidiagonals |k| <= d <= min(2 na - k, 2 nb + k): one unsigned comparison per step
    const int32_t hi_e = min(2 * (int32_t)na - ke, 2 * (int32_t)nb + ke), hi_o = min(2 * (int32_t)na - ke - 1, 2 * (int32_t)nb + ke + 1);
    const int32_t ae = ke < 0 ? -ke : ke, ao = ke + 1 < 0 ? -ke - 1 : ke + 1;
    const bool has_e = in_e && hi_e >= ae, has_o = in_o && hi_o >= ao;
    const u32 lo_e = (u32)ae, span_e = has_e ? (u32)(hi_e - ae) : 0u, lo_o = (u32)ao, span_o = has_o ? (u32)(hi_o - ao) : 0u;
    int32_t best = 0;
    int64_t rec = GP_DEAD; u32 rec_d = 0;                // the lane's last cell above the best of its time
    u32 cells = 0;
    int dead = 0;
    // what every antidiagonal ends with: the cell's count, the stop, the raise.  Returns true where the wave stops.
    auto after = [&](int64_t v, u32 d) -> bool {
        const bool live = v > GP_LIVE;
        cells += live ? 1u : 0u;
        if (!__ballot(live)) { if (++dead == 2) return true; } else dead = 0;
        const bool above = live && gp_s(v) > best;
        if (__ballot(above)) {
            if (above) { rec = v; rec_d = d; }
            best = eg_group_max<LANES>(above ? gp_s(v) : best);
        }
        return false;
    };
    for (u32 d = 1; d <= dmax; d += 2) {                 // an odd antidiagonal (diagonal ke + 1), then an even one (ke)
        {
            if ((d & 63) == 63) { if (reads) wx = gp_x32(a.e.packed, a.e.packed_bytes, p, right, ((int32_t)d + ke + 1) >> 1); } else wx <<= 2;
            const int64_t nx = __shfl_down(even, 1, LANES);
            const bool exists = has_o && d - lo_o <= span_o;
            odd = gp_cell(odd, even, gl == LANES - 1 ? GP_DEAD : nx, (u32)((wx ^ wy) >> 32) < (1u << 30), exists, best, sc);
            if (after(odd, d)) break;
        }
        if (d == dmax) break;
        {
            const u32 d2 = d + 1;
            if ((d2 & 63) == 0) { if (reads) wy = gp_y32(a.e.packed, a.e.packed_bytes, p, right, ((int32_t)d2 - ke) >> 1); } else wy <<= 2;
            const int64_t nx = __shfl_up(odd, 1, LANES);
            const bool exists = has_e && d2 - lo_e <= span_e;
            even = gp_cell(even, gl == 0 ? GP_DEAD : nx, odd, (u32)((wx ^ wy) >> 32) < (1u << 30), exists, best, sc);
            if (after(even, d2)) break;
        }
    }
    // the antidiagonal of the last raise, and its best cell: the largest word, the lowest lane
    GpSide st;
    const u32 dl = (u32)eg_group_max<LANES>((int32_t)rec_d);
    const int64_t mine = rec_d == dl && dl != 0 ? rec : GP_DEAD;
    const int64_t top = eg_group_max64<LANES>(mine);
    const u64 b = __ballot(mine == top && top > GP_LIVE);
    const int g0 = lane_id() - gl;                       // the group's first lane
    const u64 gb = (b >> g0) & (LANES == 64 ? ~0ULL : (1ULL << (LANES & 63)) - 1);
    if (gb) {
        const int src = xd_ctz64(gb);
        const int32_t ks = 2 * src - LANES + (int32_t)(dl & 1);
        st.best = gp_s(top); st.e = gp_e(top);
        st.i = (u32)(((int32_t)dl + ks) >> 1); st.j = dl - st.i;
    }
    st.cells = cells;                                    // the lane's own: the caller sums
    return st;
}

template <int LANES>
__global__ __launch_bounds__(EG_THREADS) void extend_gapped_kernel(GappedArgs a)
{
    constexpr int GROUPS = EG_THREADS / LANES;
    const int lane = lane_id();
    const int gl = (int)(threadIdx.x % LANES);
    const u64 i = (u64)blockIdx.x * GROUPS + threadIdx.x / LANES;
    const bool have = i < a.e.n, head = gl == 0;
    u64 key = 0, support = 0, first = 0;
    if (have) {
        const ulonglong2 *r = reinterpret_cast<const ulonglong2 *>(a.e.rows + i * 6);
        const ulonglong2 r0 = r[0], r1 = r[1], r2 = r[2];
        key = r0.x; support = r1.y; first = r2.x;
    }
    XdPair p;
    int err = have ? ext_pair(a.e, key, first, &p) : -1;
    if (err == 0 && (u64)p.la + (u64)p.lb >= GP_MAX_SPAN) err = EXT_STAT_ERR_SPAN;
    if (err == 0 && !xd_seed_matches(a.e.packed, a.e.packed_bytes, p)) err = EXT_STAT_ERR_SEED;
    ext_add_wave(a.e.stat + EXT_STAT_ERR_RID, head && err == EXT_STAT_ERR_RID);
    ext_add_wave(a.e.stat + EXT_STAT_ERR_INDEX, head && err == EXT_STAT_ERR_INDEX);
    ext_add_wave(a.e.stat + EXT_STAT_ERR_FIT, head && err == EXT_STAT_ERR_FIT);
    ext_add_wave(a.e.stat + EXT_STAT_ERR_SPAN, head && err == EXT_STAT_ERR_SPAN);
    ext_add_wave(a.e.stat + EXT_STAT_ERR_SEED, head && err == EXT_STAT_ERR_SEED);
    const bool ok = err == 0;
    const GpSide right = eg_side<LANES>(a, p, ok, true, gl);
    const GpSide left = eg_side<LANES>(a, p, ok, false, gl);
    u64 cols = 0, cells = left.cells + right.cells;
    if (ok && head) {
        u64 row[XD_ROW_WORDS];
        gp_row(p, key, support, a.e.match, left, right, row);
        ulonglong2 *o = reinterpret_cast<ulonglong2 *>(a.e.out + i * XD_ROW_WORDS);
        o[0] = make_ulonglong2(row[0], row[1]); o[1] = make_ulonglong2(row[2], row[3]); o[2] = make_ulonglong2(row[4], row[5]);
        if (a.e.filter) a.e.keep[i] = ext_keeps(a.e, row) ? 1 : 0;
        cols = (u64)left.i + (u64)a.e.k + (u64)right.i;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { cols += __shfl_xor(cols, o, WAVE); cells += __shfl_xor(cells, o, WAVE); }
    if (lane == 0 && cols) atomicAdd(a.e.stat + EXT_STAT_COLUMNS, (unsigned long long)cols);
    if (lane == 0 && cells) atomicAdd(a.e.stat + EXT_STAT_CELLS, (unsigned long long)cells);
}

} // namespace hsk
