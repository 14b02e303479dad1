// hsk_extend.h -- ungapped x-drop extension of the seed of every diagonal row, with the reads in HBM (device; include/hsk.h:
// hsk_pair_diags_extend has the definition; hsk_xdrop.h the windows, the mismatch masks and the step by runs that the kernels, the host
// and the CPU test share).
//
//   extend_lane_kernel   one lane per row.  The lane reads the row (three 16-byte loads), checks it -- read ids, the reads inside the packed
//                        bytes, the seed inside its reads, the seed's K columns -- and knows the row's span before any other base is read.
//                        A bad row is counted in the error block (one atomic per wave and case) and reads nothing more.  A row with
//                        span >= wave_span goes to the long-row list: one atomic per wave, the wave's rows in lane order behind it (the
//                        list's order does not matter).  Any other row is extended right, then left, a window at a time (xd_walk) and
//                        written as three 16-byte stores, with a keep flag if a filter is on.  Rows ascend in rid_a: neighbouring lanes
//                        share A's cache lines, B's loads are the scattered ones.
//   extend_wave_kernel   one wavefront per long row, EW_WAVES rows per workgroup and round.  A side is walked in steps of 64 windows
//                        (2048 columns), lane l at window l: every lane takes its window alone (its sum and the best prefix of it), a
//                        wave scan gives it the (s, best, mismatches) it enters with if nothing stopped the walk before it, and it takes
//                        the window again with these true values.  The earliest lane that stops (ballot) ends the side; the lanes in
//                        front of it saw true values, because nothing stopped in front of them.  `best` rises strictly from one lane
//                        that raises it to the next, so the last such lane up to the stop holds the side's result.  If no lane stops,
//                        lane 63's values enter the next step.  Exactly the definition, column by column.
//   extend_compact_kernel  (with min_score / min_length) the kept rows in the input's order: the keep flags of a tile are a bit mask in
//                        LDS, a row's place is the tile's offset (COUNT, count_scan_kernel, EMIT) plus the popcount of the keep bits in
//                        front of it (hsk_runmask.h).  Without a filter the rows are final where the two kernels wrote them.
// Every loop is bounded by a span or a row count; there are no spin-waits and no dependencies between workgroups; the atomics are the
// list append, the error counters and the column sum.
#pragma once
#include "hsk_device.h"
#include "hsk_runmask.h"
#include "hsk_xdrop.h"

namespace hsk {

constexpr int EL_THREADS = 256;                          // rows per workgroup of the lane path
constexpr int EW_THREADS = 256, EW_WAVES = EW_THREADS / 64;
constexpr int EC_ROUNDS = 4, EC_TILE = RM_THREADS * EC_ROUNDS, EC_WORDS = EC_TILE / 64;
constexpr u32 EXT_DEFAULT_WAVE_SPAN = 512;               // columns: a row at or above it takes the wave path (the sweep of DESIGN.md 6.7f)
// the call's block: the long-row list's length, the columns of all overlaps, the kept rows (the compaction's scan), rows refused by case
enum { EXT_STAT_LONG = 0, EXT_STAT_COLUMNS, EXT_STAT_KEPT, EXT_STAT_ERR_RID, EXT_STAT_ERR_INDEX, EXT_STAT_ERR_FIT, EXT_STAT_ERR_SEED, EXT_STAT_WORDS = 8 };

struct ExtendArgs {
    const u64 *rows; u64 n;                              // six-word diagonal rows, 16-byte aligned
    const u8 *packed; u64 packed_bytes;                  // 4-byte aligned
    const u64 *roff; const u32 *rlen; u64 nreads;
    int64_t rid_base;
    int k;
    int64_t match, mismatch, xdrop;
    u64 wave_span;                                       // span >= wave_span: the wave path (above 2^32: no row)
    u64 min_score; u32 min_length; int filter;
    u64 *out;                                            // n rows of XD_ROW_WORDS words
    u8 *keep;                                            // (filter) one flag per row
    u64 *long_rows; u64 nlong;                           // the long-row list
    unsigned long long *stat;                            // EXT_STAT_*
};

__device__ __forceinline__ void ext_add_wave(unsigned long long *word, bool pred)
{
    const u64 b = __ballot(pred);
    if (b && lane_id() == 0) atomicAdd(word, (unsigned long long)__popcll(b));
}

// the row's seed and reads; 0, or the EXT_STAT_ERR_* word of what is wrong with it (then nothing of *p may be used)
__device__ __forceinline__ int ext_pair(const ExtendArgs &a, u64 key, u64 first, XdPair *p)
{
    const int64_t ra = (int64_t)((key >> 32) & 0x7fffffffULL) - a.rid_base, rb = (int64_t)(key & 0xffffffffULL) - a.rid_base;
    if (ra < 0 || (u64)ra >= a.nreads || rb < 0 || (u64)rb >= a.nreads) return EXT_STAT_ERR_RID;
    const u64 offa = a.roff[ra], offb = a.roff[rb];
    p->la = a.rlen[ra]; p->lb = a.rlen[rb];
    if (offa > a.packed_bytes || ((u64)p->la + 3) / 4 > a.packed_bytes - offa || offb > a.packed_bytes || ((u64)p->lb + 3) / 4 > a.packed_bytes - offb) return EXT_STAT_ERR_INDEX;
    p->pa = (u32)(first >> 32); p->pb = (u32)first; p->k = a.k; p->o = (int32_t)(key >> 63);
    if ((u64)p->pa + (u64)a.k > (u64)p->la || (u64)p->pb + (u64)a.k > (u64)p->lb) return EXT_STAT_ERR_FIT;
    p->bit_a = 8 * offa; p->bit_b = 8 * offb;
    xd_range(*p);
    return 0;
}

__device__ __forceinline__ bool ext_keeps(const ExtendArgs &a, const u64 (&row)[XD_ROW_WORDS])
{
    return row[1] >= a.min_score && (u32)row[2] - (u32)(row[2] >> 32) >= a.min_length;
}

__global__ __launch_bounds__(EL_THREADS) void extend_lane_kernel(ExtendArgs a)
{
    const u64 i = (u64)blockIdx.x * EL_THREADS + threadIdx.x;
    const int lane = lane_id();
    const bool have = i < a.n;
    u64 key = 0, support = 0, first = 0;
    if (have) {
        const ulonglong2 *r = reinterpret_cast<const ulonglong2 *>(a.rows + i * 6);
        const ulonglong2 r0 = r[0], r1 = r[1], r2 = r[2];
        key = r0.x; support = r1.y; first = r2.x;
    }
    XdPair p;
    int err = have ? ext_pair(a, key, first, &p) : -1;
    if (err == 0 && !xd_seed_matches(a.packed, a.packed_bytes, p)) err = EXT_STAT_ERR_SEED;
    ext_add_wave(a.stat + EXT_STAT_ERR_RID, err == EXT_STAT_ERR_RID);
    ext_add_wave(a.stat + EXT_STAT_ERR_INDEX, err == EXT_STAT_ERR_INDEX);
    ext_add_wave(a.stat + EXT_STAT_ERR_FIT, err == EXT_STAT_ERR_FIT);
    ext_add_wave(a.stat + EXT_STAT_ERR_SEED, err == EXT_STAT_ERR_SEED);
    const bool ok = err == 0;
    const bool lng = ok && (u64)(p.t_hi - p.t_lo) >= a.wave_span;
    {                                                    // the long rows of the wave: one atomic, lane order behind it
        const u64 b = __ballot(lng);
        if (b) {
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(a.stat + EXT_STAT_LONG, (unsigned long long)__popcll(b));
            base = __shfl(base, 0, WAVE);
            if (lng) a.long_rows[base + (u64)__popcll(b & ((1ULL << lane) - 1))] = i;
        }
    }
    u64 cols = 0;
    if (ok && !lng) {
        const XdSide right = xd_walk(a.packed, a.packed_bytes, p, true, a.match, a.mismatch, a.xdrop);
        const XdSide left = xd_walk(a.packed, a.packed_bytes, p, false, a.match, a.mismatch, a.xdrop);
        u64 row[XD_ROW_WORDS];
        xd_row(p, key, support, a.match, left, right, row);
        ulonglong2 *o = reinterpret_cast<ulonglong2 *>(a.out + i * XD_ROW_WORDS);
        o[0] = make_ulonglong2(row[0], row[1]); o[1] = make_ulonglong2(row[2], row[3]); o[2] = make_ulonglong2(row[4], row[5]);
        if (a.filter) a.keep[i] = ext_keeps(a, row) ? 1 : 0;
        cols = (u64)left.len + (u64)a.k + (u64)right.len;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cols += __shfl_xor(cols, o, WAVE);
    if (lane == 0 && cols) atomicAdd(a.stat + EXT_STAT_COLUMNS, (unsigned long long)cols);
}

// exclusive maximum of v over the lanes in front of this one (XD_NONE in lane 0)
__device__ __forceinline__ int64_t ext_excl_max(int64_t v, int lane)
{
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int64_t n = __shfl_up(v, o, WAVE);
        if (lane >= o && n > v) v = n;
    }
    const int64_t e = __shfl_up(v, 1, WAVE);
    return lane ? e : XD_NONE;
}

// one side of a long row by the whole wave; every lane returns the side's result
__device__ __forceinline__ XdSide ext_wave_side(const ExtendArgs &a, const XdPair &p, bool right, int lane)
{
    const u64 cols = right ? (u64)(p.t_hi - p.k) : (u64)(-p.t_lo);
    XdSide st;                                           // what enters the step: s, seen; and the side's result so far: best, len, mm
    for (u64 base = 0; base < cols; base += 64 * 32) {
        const u64 c0 = base + 32 * (u64)lane;
        const u32 n = c0 >= cols ? 0u : (cols - c0 < 32 ? (u32)(cols - c0) : 32u);
        const u64 m = n ? xd_walk_mask(a.packed, a.packed_bytes, p, right, c0, n) : 0ULL;
        XdSide own; own.best = XD_NONE;                  // the window alone: its sum, and the best prefix that ends a run of matches
        (void)xd_step(own, m, n, 0, a.match, a.mismatch, XD_NO_DROP);
        const int64_t sum = own.s;
        const int64_t s_in = st.s + wave_incl_scan<int64_t>(sum) - sum;
        const int64_t reach = ext_excl_max(own.best == XD_NONE ? XD_NONE : s_in + own.best, lane);
        const u32 pc = (u32)__popcll(m);
        XdSide q;
        q.s = s_in; q.best = reach > st.best ? reach : st.best; q.seen = st.seen + wave_incl_scan<u32>(pc) - pc;
        const int64_t best_in = q.best;
        const bool drop = xd_step(q, m, n, (u32)c0, a.match, a.mismatch, a.xdrop);
        const u64 dmask = __ballot(drop);
        const int stop = dmask ? xd_ctz64(dmask) : WAVE - 1;
        const u64 umask = __ballot(q.best > best_in) & (stop == WAVE - 1 ? ~0ULL : (1ULL << (stop + 1)) - 1);
        if (umask) {
            const int src = 63 - __builtin_clzll(umask);
            st.best = __shfl(q.best, src, WAVE); st.len = __shfl(q.len, src, WAVE); st.mm = __shfl(q.mm, src, WAVE);
        }
        if (dmask) break;
        st.s = __shfl(q.s, WAVE - 1, WAVE); st.seen = __shfl(q.seen, WAVE - 1, WAVE);
    }
    return st;
}

__global__ __launch_bounds__(EW_THREADS) void extend_wave_kernel(ExtendArgs a)
{
    const int lane = lane_id();
    const u64 wave = (u64)blockIdx.x * EW_WAVES + (threadIdx.x >> 6), nwaves = (u64)gridDim.x * EW_WAVES;
    u64 cols = 0;
    for (u64 j = wave; j < a.nlong; j += nwaves) {
        const u64 i = a.long_rows[j];
        if (i >= a.n) continue;                          // (never: the lane path wrote the list)
        const u64 key = a.rows[i * 6], support = a.rows[i * 6 + 3], first = a.rows[i * 6 + 4];
        XdPair p;
        if (ext_pair(a, key, first, &p) != 0) continue;  // (never: only rows that passed are listed)
        const XdSide right = ext_wave_side(a, p, true, lane);
        const XdSide left = ext_wave_side(a, p, false, lane);
        u64 row[XD_ROW_WORDS];
        xd_row(p, key, support, a.match, left, right, row);
        if (lane < 3) {
            const ulonglong2 v = lane == 0 ? make_ulonglong2(row[0], row[1]) : (lane == 1 ? make_ulonglong2(row[2], row[3]) : make_ulonglong2(row[4], row[5]));
            reinterpret_cast<ulonglong2 *>(a.out + i * XD_ROW_WORDS)[lane] = v;
        }
        if (a.filter && lane == 0) a.keep[i] = ext_keeps(a, row) ? 1 : 0;
        cols += (u64)left.len + (u64)a.k + (u64)right.len;
    }
    if (lane == 0 && cols) atomicAdd(a.stat + EXT_STAT_COLUMNS, (unsigned long long)cols);
}

struct ExtendCompactArgs { const u64 *in; const u8 *keep; u64 n; u64 *tile_cnt; u64 *rows; };

// COUNT (EMIT == false): tile_cnt[tile] = kept rows of the tile.  EMIT: tile_cnt holds the exclusive scan; the kept rows leave in order.
// KEEP_ZERO: the rows whose byte is 0 stay (hsk_overlaps_reduce: the byte is the row's class, and 0 is KEPT).
template <bool EMIT, bool KEEP_ZERO = false>
__global__ __launch_bounds__(RM_THREADS) void extend_compact_kernel(ExtendCompactArgs a)
{
    __shared__ u64 s_keep[EC_WORDS];
    __shared__ u32 s_pre[EC_WORDS + 1];
    const u64 t0 = (u64)blockIdx.x * EC_TILE;
    bool kp[EC_ROUNDS];
#pragma unroll
    for (int j = 0; j < EC_ROUNDS; ++j) {
        const u64 g = t0 + (u64)j * RM_THREADS + threadIdx.x;
        kp[j] = g < a.n && (a.keep[g] != 0) != KEEP_ZERO;
        rm_publish(s_keep, j, __ballot(kp[j]));
    }
    __syncthreads();
    rm_prefix<EC_WORDS>(s_keep, s_pre);
    __syncthreads();
    if (!EMIT) { if (threadIdx.x == 0) a.tile_cnt[blockIdx.x] = s_pre[EC_WORDS]; return; }
    const u64 base = a.tile_cnt[blockIdx.x];
#pragma unroll
    for (int j = 0; j < EC_ROUNDS; ++j) {
        if (!kp[j]) continue;
        const u64 g = t0 + (u64)j * RM_THREADS + threadIdx.x;
        const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(a.in + g * XD_ROW_WORDS);
        ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(a.rows + (base + rm_slot(s_keep, s_pre, j)) * XD_ROW_WORDS);
        const ulonglong2 v0 = src[0], v1 = src[1], v2 = src[2];
        dst[0] = v0; dst[1] = v1; dst[2] = v2;
    }
}

} // namespace hsk
