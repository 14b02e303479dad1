// hsk_reduce.h -- the string graph of a list of overlap rows in HBM: contained reads out, dovetails turned into arcs between read ends,
// transitive arcs marked (device; include/hsk.h: hsk_overlaps_reduce has the definition; hsk_strgraph.h the row class, the arcs, the
// duplicate rule, the witness test and the search that the kernels, the host and the CPU test share).
//
//   reduce_classify_kernel  one lane per row: three 16-byte loads, the two lengths, the check of the row against them (a bad row is counted
//                        in the call's block, one atomic per wave and case, and gets the byte 0xff), the class a row has by itself, and the
//                        contained bit of read a or b by an atomicOr on the bit words.
//   reduce_arcs_kernel   COUNT / EMIT over tiles of EC_TILE rows (the CountEmit driver), behind the classify launch because the contained
//                        bits must be complete: COUNT turns a dovetail with a contained read into DROPPED_READ and counts the others;
//                        EMIT writes their two arc records (key v << 32 | w, value len << 32 | row) at twice the row's rank among them.
//   reduce_dups_kernel   one lane per sorted record.  A record with an equal key beside it walks its run and gathers (key, ends, score) of
//                        the runs' rows: it is out if a row with the same (key, ends) beats its own (sg_dup_beats).  The values leave for
//                        the sort's other buffer, SG_DEAD for a loser, so no lane reads what another writes; the loser's row gets DUPLICATE
//                        -- from both of its records, the same byte.
//   reduce_offsets_kernel  one lane per vertex: a binary search for the vertex's first record; its degree gives max_degree and the count of
//                        the vertices the wave path takes.
//   reduce_lane_kernel   one lane per record of a vertex below wave_degree: sg_arc_transitive, the walk over out(v) with a search in out(w).
//   reduce_wave_kernel   one workgroup per vertex at or above wave_degree (repeats make vertices of degree in the thousands, where one
//                        lane would walk deg^2 searches while the launch waits for it).  out(v) is staged in LDS RD_CHUNK records at a
//                        time: target, length and a hit word.  Every wave takes every fourth w of out(v); its lanes stream out(w) from
//                        HBM -- coalesced, only the records whose target lies inside the chunk -- and search each target in the chunk in
//                        LDS; a witness sets the hit word.  The same pairs (w, x) meet as on the lane path, so the result is the same.
//   reduce_census_kernel rows per class and contained reads.
// The kept rows leave through extend_compact_kernel (hsk_extend.h) with the class byte as its flag.
// Every loop is bounded by a row, record or vertex count; there are no spin-waits and no dependencies between workgroups; the atomics are
// the contained bits and the call's counters; a class byte is written with one value per launch, whoever writes it.
#pragma once
#include "hsk_device.h"
#include "hsk_runmask.h"
#include "hsk_extend.h"
#include "hsk_strgraph.h"

namespace hsk {

constexpr int RD_THREADS = 256, RD_WAVES = RD_THREADS / 64;
constexpr int RD_CHUNK = 1024;                           // records of out(v) in LDS at a time (12 KB)
constexpr u32 RD_DEFAULT_WAVE_DEGREE = 256;              // out-arcs: a vertex at or above it takes the wave path
constexpr u8 RD_BAD_ROW = 0xff;                          // the byte of a row the call refuses
// the call's block: dovetail rows between live reads (the arcs' scan), rows refused by case, live records, vertices on the wave path, the
// largest degree, the kept rows (the compaction's scan), contained reads; then the rows per class
enum { RD_STAT_ROWS = 0, RD_STAT_ERR_RID, RD_STAT_ERR_LEN, RD_STAT_ARCS, RD_STAT_WAVE, RD_STAT_MAXDEG, RD_STAT_KEPT, RD_STAT_CONTAINED, RD_STAT_CLASS = 8, RD_STAT_WORDS = 16 };

struct ReduceArgs {
    const u64 *rows; u64 n;                              // six-word overlap rows, 16-byte aligned
    const u32 *rlen; u64 nreads; int64_t rid_base;
    u8 *cls;                                             // one byte per row
    u32 *contained; u64 cwords;                          // one bit per read
    u64 *tile_cnt;
    u64 *keys, *vals; u64 narcs;                         // the arc records: EMIT's target, then the sorted side
    u64 *vals_out;                                       // reduce_dups_kernel: the sort's other value buffer
    u64 *off;                                            // 2 nreads + 1 words
    u32 fuzz; u64 wave_degree;                           // (above 2^33: no vertex)
    unsigned long long *stat;                            // RD_STAT_*
};

// the reads of a row, from 0; false: one lies outside the reads that were given
__device__ __forceinline__ bool rd_reads(const ReduceArgs &a, u64 key, u64 *ra, u64 *rb)
{
    const int64_t x = (int64_t)((key >> 32) & 0x7fffffffULL) - a.rid_base, y = (int64_t)(key & 0xffffffffULL) - a.rid_base;
    *ra = (u64)x; *rb = (u64)y;
    return x >= 0 && (u64)x < a.nreads && y >= 0 && (u64)y < a.nreads;
}

__global__ __launch_bounds__(RD_THREADS) void reduce_classify_kernel(ReduceArgs a)
{
    const u64 i = (u64)blockIdx.x * RD_THREADS + threadIdx.x;
    int err = 0;
    if (i < a.n) {
        const ulonglong2 *r = reinterpret_cast<const ulonglong2 *>(a.rows + i * 6);
        const ulonglong2 r0 = r[0], r1 = r[1], r2 = r[2];
        const u64 key = r0.x;
        u64 ra, rb;
        u8 c = RD_BAD_ROW;
        if (!rd_reads(a, key, &ra, &rb)) err = RD_STAT_ERR_RID;
        else {
            const u32 e = (u32)r2.x & 15u;
            if (!sg_consistent(e, a.rlen[ra], a.rlen[rb], sg_span(r1.x, r1.y))) err = RD_STAT_ERR_LEN;
            else {
                c = (u8)sg_row_class((u32)(key >> 63), e, ra, rb);
                if (c == SG_A_CONTAINED) atomicOr(a.contained + (ra >> 5), 1u << (ra & 31));
                if (c == SG_B_CONTAINED) atomicOr(a.contained + (rb >> 5), 1u << (rb & 31));
            }
        }
        a.cls[i] = c;
    }
    ext_add_wave(a.stat + RD_STAT_ERR_RID, err == RD_STAT_ERR_RID);
    ext_add_wave(a.stat + RD_STAT_ERR_LEN, err == RD_STAT_ERR_LEN);
}

// COUNT (EMIT == false): a dovetail with a contained read becomes DROPPED_READ; tile_cnt[tile] = the others.  EMIT: tile_cnt holds the
// exclusive scan; the two records of every dovetail that is left.
template <bool EMIT>
__global__ __launch_bounds__(RM_THREADS) void reduce_arcs_kernel(ReduceArgs a)
{
    __shared__ u64 s_keep[EC_WORDS];
    __shared__ u32 s_pre[EC_WORDS + 1];
    const u64 t0 = (u64)blockIdx.x * EC_TILE;
    bool kp[EC_ROUNDS];
#pragma unroll
    for (int j = 0; j < EC_ROUNDS; ++j) {
        const u64 g = t0 + (u64)j * RM_THREADS + threadIdx.x;
        kp[j] = g < a.n && a.cls[g] == SG_KEPT;
        if (!EMIT && kp[j]) {
            u64 ra, rb;
            (void)rd_reads(a, a.rows[g * 6], &ra, &rb);  // (inside the reads: the row has a class)
            if (((a.contained[ra >> 5] >> (ra & 31)) | (a.contained[rb >> 5] >> (rb & 31))) & 1u) { a.cls[g] = SG_DROPPED_READ; kp[j] = false; }
        }
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
        const ulonglong2 *r = reinterpret_cast<const ulonglong2 *>(a.rows + g * 6);
        const ulonglong2 r0 = r[0], r1 = r[1], r2 = r[2];
        u64 ra, rb;
        (void)rd_reads(a, r0.x, &ra, &rb);
        SgArc x, y;
        sg_arcs((u32)(r0.x >> 63), (u32)r2.x & 15u, (u32)ra, (u32)rb, a.rlen[ra], a.rlen[rb], sg_span(r1.x, r1.y), x, y);
        const u64 slot = base + rm_slot(s_keep, s_pre, j);
        if (2 * slot + 1 >= a.narcs) continue;            // (never: narcs is twice the scan's total)
        reinterpret_cast<ulonglong2 *>(a.keys)[slot] = make_ulonglong2(sg_arc_key(x.v, x.w), sg_arc_key(y.v, y.w));
        reinterpret_cast<ulonglong2 *>(a.vals)[slot] = make_ulonglong2(sg_arc_val(x.len, (u32)g), sg_arc_val(y.len, (u32)g));
    }
}

__global__ __launch_bounds__(RD_THREADS) void reduce_dups_kernel(ReduceArgs a)
{
    const u64 j = (u64)blockIdx.x * RD_THREADS + threadIdx.x;
    bool live = false;
    if (j < a.narcs) {
        const u64 k = a.keys[j], val = a.vals[j];
        const u64 row = val & 0xffffffffULL;
        bool lost = false;
        if (row < a.n && ((j > 0 && a.keys[j - 1] == k) || (j + 1 < a.narcs && a.keys[j + 1] == k))) {
            const u64 rk = a.rows[row * 6], rs = a.rows[row * 6 + 1], re = a.rows[row * 6 + 4] & 15u;
            u64 h = j;
            while (h > 0 && a.keys[h - 1] == k) --h;
            for (u64 i = h; i < a.narcs && a.keys[i] == k && !lost; ++i) {
                const u64 ri = a.vals[i] & 0xffffffffULL;
                if (i == j || ri >= a.n) continue;
                lost = a.rows[ri * 6] == rk && (a.rows[ri * 6 + 4] & 15u) == re && sg_dup_beats(a.rows[ri * 6 + 1], ri, rs, row);
            }
        }
        a.vals_out[j] = lost ? SG_DEAD : val;
        if (lost && row < a.n) a.cls[row] = SG_DUPLICATE;
        live = !lost;
    }
    ext_add_wave(a.stat + RD_STAT_ARCS, live);
}

__global__ __launch_bounds__(RD_THREADS) void reduce_offsets_kernel(ReduceArgs a)
{
    const u64 v = (u64)blockIdx.x * RD_THREADS + threadIdx.x, nv = 2 * a.nreads;
    u64 deg = 0;
    if (v < nv) {
        const u64 lo = sg_lower_bound(a.keys, 0, a.narcs, v << 32);
        const u64 hi = v + 1 == nv ? a.narcs : sg_lower_bound(a.keys, lo, a.narcs, (v + 1) << 32);
        a.off[v] = lo;
        deg = hi - lo;
    } else if (v == nv) a.off[v] = a.narcs;
    ext_add_wave(a.stat + RD_STAT_WAVE, deg != 0 && deg >= a.wave_degree);
    u64 m = deg;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u64 n1 = __shfl_xor(m, o, WAVE); m = n1 > m ? n1 : m; }
    if (lane_id() == 0 && m) atomicMax(a.stat + RD_STAT_MAXDEG, (unsigned long long)m);
}

__global__ __launch_bounds__(RD_THREADS) void reduce_lane_kernel(ReduceArgs a)
{
    const u64 j = (u64)blockIdx.x * RD_THREADS + threadIdx.x;
    if (j >= a.narcs) return;
    const u64 v = a.keys[j] >> 32;
    if (v >= 2 * a.nreads || a.off[v + 1] - a.off[v] >= a.wave_degree) return;
    if (!sg_arc_transitive(a.keys, a.vals, a.off, j, a.fuzz)) return;
    const u64 row = a.vals[j] & 0xffffffffULL;
    if (row < a.n) a.cls[row] = SG_REDUCED;
}

__global__ __launch_bounds__(RD_THREADS) void reduce_wave_kernel(ReduceArgs a)
{
    __shared__ u32 s_x[RD_CHUNK], s_len[RD_CHUNK], s_hit[RD_CHUNK];      // s_hit: 0 open, 1 a witness was found, 2 a dead record
    __shared__ u32 s_lmax;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 nv = 2 * a.nreads;
    for (u64 v = blockIdx.x; v < nv; v += gridDim.x) {
        const u64 s0 = a.off[v], s1 = a.off[v + 1], deg = s1 - s0;
        if (deg == 0 || deg < a.wave_degree || s1 > a.narcs) continue;  // (the same for the whole workgroup)
        for (u64 c0 = s0; c0 < s1; c0 += RD_CHUNK) {
            const u32 nx = s1 - c0 < (u64)RD_CHUNK ? (u32)(s1 - c0) : (u32)RD_CHUNK;
            __syncthreads();                             // (the chunk before has been read)
            if (tid == 0) s_lmax = 0;
            __syncthreads();
            u32 mx = 0;
            for (u32 t = tid; t < nx; t += RD_THREADS) {
                const u64 val = a.vals[c0 + t];
                const bool dead = val == SG_DEAD;
                const u32 len = dead ? 0u : (u32)(val >> 32);
                s_x[t] = (u32)a.keys[c0 + t]; s_len[t] = len; s_hit[t] = dead ? 2u : 0u;
                mx = len > mx ? len : mx;
            }
            if (mx) atomicMax(&s_lmax, mx);
            __syncthreads();
            const u64 reach_max = (u64)s_lmax + (u64)a.fuzz;
            const u32 xmin = s_x[0], xmax = s_x[nx - 1];
            for (u64 i = s0 + wave; i < s1; i += RD_WAVES) {            // this wave's w (the same for its 64 lanes)
                const u64 wval = a.vals[i];
                const u32 w = (u32)a.keys[i];
                const u64 len_vw = wval >> 32;
                if (wval == SG_DEAD || (w >> 1) == (u32)(v >> 1) || len_vw > reach_max || (u64)w >= nv) continue;
                u64 wlo = a.off[w], whi = a.off[(u64)w + 1];
                if (whi > a.narcs) continue;
                if (deg > (u64)RD_CHUNK) {               // only the records of out(w) whose target lies inside the chunk
                    wlo = sg_lower_bound(a.keys, wlo, whi, sg_arc_key(w, xmin));
                    if (xmax != 0xffffffffu) whi = sg_lower_bound(a.keys, wlo, whi, sg_arc_key(w, xmax + 1));
                }
                for (u64 p = wlo + lane; p < whi; p += WAVE) {
                    const u64 v2 = a.vals[p];
                    const u32 x2 = (u32)a.keys[p];
                    if (v2 == SG_DEAD || (x2 >> 1) == (w >> 1)) continue;
                    const u64 sum = len_vw + (v2 >> 32);
                    u32 lo = 0, hi = nx;
                    while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (s_x[mid] < x2) lo = mid + 1; else hi = mid; }
                    for (u32 t = lo; t < nx && s_x[t] == x2; ++t)
                        if (s_hit[t] == 0 && sum <= (u64)s_len[t] + (u64)a.fuzz) s_hit[t] = 1;
                }
            }
            __syncthreads();
            for (u32 t = tid; t < nx; t += RD_THREADS) {
                if (s_hit[t] != 1) continue;
                const u64 row = a.vals[c0 + t] & 0xffffffffULL;
                if (row < a.n) a.cls[row] = SG_REDUCED;
            }
        }
    }
}

// rows per class into stat[RD_STAT_CLASS + class], contained reads into stat[RD_STAT_CONTAINED]
__global__ __launch_bounds__(RD_THREADS) void reduce_census_kernel(ReduceArgs a)
{
    const int lane = lane_id();
    const u64 stride = (u64)gridDim.x * RD_THREADS, first = (u64)blockIdx.x * RD_THREADS + threadIdx.x;
    u64 acc = 0;
    for (u64 b = (u64)blockIdx.x * RD_THREADS; b < a.n; b += stride) {   // (whole waves enter: the ballots see every lane)
        const u64 i = b + threadIdx.x;
        const u32 c = i < a.n ? a.cls[i] : 0xffu;
#pragma unroll
        for (int k = 0; k < SG_CLASSES; ++k) {
            const u64 m = __ballot(c == (u32)k);
            if (lane == k) acc += (u64)__popcll(m);
        }
    }
    if (lane < SG_CLASSES && acc) atomicAdd(a.stat + RD_STAT_CLASS + lane, (unsigned long long)acc);
    u64 bits = 0;
    for (u64 i = first; i < a.cwords; i += stride) bits += (u64)__popc(a.contained[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bits += __shfl_xor(bits, o, WAVE);
    if (lane == 0 && bits) atomicAdd(a.stat + RD_STAT_CONTAINED, (unsigned long long)bits);
}

} // namespace hsk
