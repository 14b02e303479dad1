// hsk_runmask.h -- the steps that the run reducers of the pair stage share (device helpers, no kernels).
//
// A workgroup of RM_THREADS lanes looks at a tile of sorted records, lane `tid` at positions p = j * RM_THREADS + tid.  A predicate of
// the positions is a bit mask in LDS: a wave's ballot of round j is word j * RM_WAVES + wave = p >> 6, the lane is bit p & 63.  The HEAD mask
// marks the first record of every run; a run belongs to the tile it starts in, and only the tile's last run can leave the tile: the
// whole workgroup follows that one to its end (rm_follow; diag_reduce_kernel keeps that loop and its three accumulators
// in its own text: through the helper it needs 66 VGPRs, not 64) and reduces what its lanes saw (rm_reduce_run).  The KEEP mask marks the
// heads whose run becomes a row; a row's slot is the popcount of the keep bits in front of it, so the rows leave in the order of the
// records and without atomics.  count_kernel (hsk_count.h) introduced the shape; pair_reduce_kernel (hsk_pairs.h), diag_reduce_kernel
// and diag_select_kernel (hsk_pairdiag.h) are written on top of these helpers.  The barriers between the steps stay with the kernels.
#pragma once
#include "hsk_device.h"

namespace hsk {

constexpr int RM_THREADS = 256, RM_WAVES = RM_THREADS / 64;

// A wave's ballot of round j into its word of the mask.  The caller takes the ballot: with the predicate as a bool argument the compiler
// keeps the kernels' flag arrays in byte registers, which costs diag_reduce_kernel 50 to 80 instructions.
__device__ __forceinline__ void rm_publish(u64 *s_mask, int j, u64 ballot)
{
    if ((threadIdx.x & 63) == 0) s_mask[j * RM_WAVES + (threadIdx.x >> 6)] = ballot;
}

// the position of the last set bit of the mask; -1: none (the tile lies inside a run that started before it)
template <int WORDS>
__device__ __forceinline__ int rm_last_head(const u64 *s_head)
{
    int lw = WORDS - 1;
    while (lw >= 0 && s_head[lw] == 0) --lw;
    return lw < 0 ? -1 : lw * 64 + 63 - __builtin_clzll(s_head[lw]);
}

// the first head behind position p; there is one (p is not the last head of the tile)
__device__ __forceinline__ u32 rm_next_head(const u64 *s_head, u32 p)
{
    u32 w = p >> 6;
    u64 m = s_head[w] & ((p & 63) == 63 ? 0ULL : (~0ULL << ((p & 63) + 1)));
    while (m == 0) m = s_head[++w];
    return (w << 6) + (u32)__builtin_ctzll(m);
}

// The workgroup walks the records from g0 on, RM_THREADS * AHEAD per step, until a lane meets the end of the array or a record for
// which same(gi) is false -- same() takes a record of the run into the lane's partial result.  Every lane leaves at the same step.
template <int AHEAD, typename Same>
__device__ __forceinline__ void rm_follow(u64 g0, u64 n, Same &&same)
{
    for (u64 g = g0;; g += (u64)RM_THREADS * AHEAD) {
        int stop = g >= n;
        if (!stop) {
#pragma unroll
            for (int s = 0; s < AHEAD; ++s) {
                const u64 gi = g + (u64)s * RM_THREADS + threadIdx.x;
                if (gi >= n || !same(gi)) stop = 1;
            }
        }
        if (__syncthreads_or(stop)) break;
    }
}

struct RunAcc {                                           // records of a run, and (MINMAX) the smallest and the largest of their values
    u64 n = 0, mn = ~0ULL, mx = 0;
    template <bool MINMAX> __device__ __forceinline__ void take(u64 v) { ++n; if (MINMAX) { mn = v < mn ? v : mn; mx = v > mx ? v : mx; } }
    // the run [p, p + c) of a tile's values in LDS
    __device__ __forceinline__ void span(const u64 *s_v, u32 p, u32 c) { n = c; mn = ~0ULL; mx = 0; for (u32 q = p; q < p + c; ++q) { const u64 v = s_v[q]; mn = v < mn ? v : mn; mx = v > mx ? v : mx; } }
};

// every lane's partial result of the tile's last run becomes the workgroup's; one barrier, s_red is read by every wave behind it
template <bool MINMAX>
__device__ __forceinline__ void rm_reduce_run(RunAcc &r, u64 (*s_red)[3])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        r.n += __shfl_xor(r.n, o, WAVE);
        if (MINMAX) { const u64 n1 = __shfl_xor(r.mn, o, WAVE), x1 = __shfl_xor(r.mx, o, WAVE); r.mn = n1 < r.mn ? n1 : r.mn; r.mx = x1 > r.mx ? x1 : r.mx; }
    }
    if (lane == 0) { s_red[wave][0] = r.n; s_red[wave][1] = r.mn; s_red[wave][2] = r.mx; }
    __syncthreads();
    r = RunAcc();
#pragma unroll
    for (int w = 0; w < RM_WAVES; ++w) { r.n += s_red[w][0]; r.mn = s_red[w][1] < r.mn ? s_red[w][1] : r.mn; r.mx = s_red[w][2] > r.mx ? s_red[w][2] : r.mx; }
}

// s_pre[w] = the keep bits in front of word w, s_pre[WORDS] = all of them; the first wave's work, between two barriers of the kernel
template <int WORDS>
__device__ __forceinline__ void rm_prefix(const u64 *s_keep, u32 *s_pre)
{
    static_assert(WORDS <= 64, "one wave scans the words");
    const int tid = threadIdx.x;
    if (tid < 64) {
        const u32 v = tid < WORDS ? (u32)__popcll(s_keep[tid]) : 0;
        const u32 inc = wave_incl_scan<u32>(v);
        if (tid < WORDS) s_pre[tid] = inc - v;
        if (tid == WORDS - 1) s_pre[WORDS] = inc;
    }
}

// the kept head of this lane in round j: its place among the tile's rows
__device__ __forceinline__ u32 rm_slot(const u64 *s_keep, const u32 *s_pre, int j)
{
    const u32 w = j * RM_WAVES + (threadIdx.x >> 6);
    return s_pre[w] + (u32)__popcll(s_keep[w] & ((1ULL << (threadIdx.x & 63)) - 1));
}

} // namespace hsk
