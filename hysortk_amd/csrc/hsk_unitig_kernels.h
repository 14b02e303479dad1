// hsk_unitig_kernels.h -- the unitigs of a list of string graph edges in HBM: the maximal non-branching paths, every member read's
// orientation and position (device; include/hsk.h: hsk_overlaps_unitigs has the definition; hsk_unitig.h the out-arcs of a vertex, the
// link test, the state of a vertex and its doubling step, the canonical rule and the row packers that the kernels and the CPU test share).
// The arc records are those of hsk_reduce.h: reduce_arcs_kernel writes them, the sort orders them, reduce_offsets_kernel finds out(v).
//
//   unitig_classify_kernel one lane per row: the check of reduce_classify_kernel, and on top a row that is no dovetail between two different
//                        reads or names a contained read is counted in the call's block; a good row gets the byte KEPT.
//   unitig_out_kernel    one lane per vertex: ut_out over its records -- degree, the only target, the representative.
//   unitig_link_kernel   one lane per vertex: pred(v) from the degrees (ut_pred) and the state ut_init gives it.
//   unitig_round_kernel  one ranking round, one lane per vertex: its state from one buffer (coalesced, two 16-byte loads), the state of
//                        the vertex its pointer names from the same buffer (the gather: 32 bytes, one sector), ut_step, the result into
//                        the other buffer.  No lane follows a chain; no word is read that the launch writes; no atomics.
//   unitig_cut_kernel    one lane per vertex, in place (a lane reads and writes its own state only): ut_cut.
//   unitig_heads_kernel  COUNT / EMIT over tiles of UT_THREADS vertices (the CountEmit driver, two tile arrays): a HEAD is a live vertex
//                        without pointer whose chain is canonical; COUNT sums the heads and their reads per tile, EMIT gives every
//                        head its unitig -- the heads in front of it -- and its first layout row -- their reads --, writes the unitig
//                        row, and leaves UT_NONE for every other vertex.
//   unitig_layout_kernel one lane per vertex: a live vertex whose chain's head has a unitig writes its layout row at first + rank.
//   unitig_census_kernel the counts: over the vertices (links, branch vertices, arcs, live reads) and over the unitig rows (singletons,
//                        circular, longest).
// Block size: every kernel is one vertex per lane in workgroups of 256 -- whole waves, 32 bytes per lane coalesced.  A round is bound
// by the latency of the gather, not by bandwidth or registers (under 32 VGPRs), so what counts is the number of gathers in flight:
// 256-lane workgroups leave every SIMD its full eight waves, and a grid over all vertices keeps them filled to the last tile.
#pragma once
#include "hsk_reduce.h"
#include "hsk_unitig.h"

namespace hsk {

constexpr int UT_THREADS = 256;
// the call's block.  The first eight words are what the first wait brings: the dovetail rows (the arcs' scan) and the refusals by case.
// Then the unitigs and the members (the heads' scans), the census, and BROKEN: how often a guard that can never fire did -- the result
// would have a hole there, so the host turns any such count into HSK_ERR_INTERNAL.
enum { UT_STAT_ROWS = 0, UT_STAT_ERR_RID, UT_STAT_ERR_LEN, UT_STAT_ERR_DOVE, UT_STAT_ERR_CONT, UT_STAT_UNITIGS = 8, UT_STAT_MEMBERS, UT_STAT_SINGLE, UT_STAT_CIRCULAR,
       UT_STAT_LONGEST, UT_STAT_LINKS, UT_STAT_BRANCH, UT_STAT_LIVE, UT_STAT_ARCS, UT_STAT_BROKEN, UT_STAT_WORDS = 24 };

struct UnitigArgs {
    const u64 *rows; u64 n;                              // six-word overlap rows, 16-byte aligned
    const u32 *rlen; u64 nreads; int64_t rid_base;
    u8 *cls;
    const u32 *contained;                                // one bit per read
    const u64 *keys, *vals, *off; u64 narcs;             // the sorted arc records; off: 2 nreads + 1 words
    u32 *deg, *cand, *pred; u64 *rep;                    // per vertex
    const UtState *cur; UtState *nxt;                    // the two state buffers of a round; cur: the final states behind the last one
    u64 *tile_heads, *tile_reads;
    u32 *uid; u64 *ufirst;                               // per vertex: the unitig and the first layout row of a head
    u64 *table, *layout; u64 nunitigs, nmembers;
    unsigned long long *stat;                            // UT_STAT_*
};

// a `(never: ...)` guard fired
__device__ __forceinline__ void ut_broken(const UnitigArgs &a) { atomicAdd(a.stat + UT_STAT_BROKEN, 1ULL); }

__device__ __forceinline__ bool ut_contained(const UnitigArgs &a, u64 r) { return (a.contained[r >> 5] >> (r & 31)) & 1u; }

__device__ __forceinline__ UtState ut_load(const UtState *p)
{
    const ulonglong2 *q = reinterpret_cast<const ulonglong2 *>(p);
    const ulonglong2 x = q[0], y = q[1];
    UtState s; s.sum = x.x; s.ptr = (u32)x.y; s.cnt = (u32)(x.y >> 32); s.minv = (u32)y.x; s.far = (u32)(y.x >> 32); s.cyc = (u32)y.y; s.pad_ = 0;
    return s;
}
__device__ __forceinline__ void ut_store(UtState *p, const UtState &s)
{
    ulonglong2 *q = reinterpret_cast<ulonglong2 *>(p);
    q[0] = make_ulonglong2(s.sum, (u64)s.cnt << 32 | s.ptr);
    q[1] = make_ulonglong2((u64)s.far << 32 | s.minv, (u64)s.cyc);
}

__global__ __launch_bounds__(UT_THREADS) void unitig_classify_kernel(UnitigArgs a)
{
    const u64 i = (u64)blockIdx.x * UT_THREADS + threadIdx.x;
    int err = 0;
    if (i < a.n) {
        const ulonglong2 *r = reinterpret_cast<const ulonglong2 *>(a.rows + i * 6);
        const ulonglong2 r0 = r[0], r1 = r[1], r2 = r[2];
        const u64 key = r0.x;
        const int64_t x = (int64_t)((key >> 32) & 0x7fffffffULL) - a.rid_base, y = (int64_t)(key & 0xffffffffULL) - a.rid_base;
        const u32 e = (u32)r2.x & 15u;
        if (!(x >= 0 && (u64)x < a.nreads && y >= 0 && (u64)y < a.nreads)) err = UT_STAT_ERR_RID;
        else if (!sg_consistent(e, a.rlen[x], a.rlen[y], sg_span(r1.x, r1.y))) err = UT_STAT_ERR_LEN;
        else if (sg_row_class((u32)(key >> 63), e, (u64)x, (u64)y) != SG_KEPT) err = UT_STAT_ERR_DOVE;
        else if (ut_contained(a, (u64)x) || ut_contained(a, (u64)y)) err = UT_STAT_ERR_CONT;
        a.cls[i] = err ? RD_BAD_ROW : (u8)SG_KEPT;
    }
    ext_add_wave(a.stat + UT_STAT_ERR_RID, err == UT_STAT_ERR_RID);
    ext_add_wave(a.stat + UT_STAT_ERR_LEN, err == UT_STAT_ERR_LEN);
    ext_add_wave(a.stat + UT_STAT_ERR_DOVE, err == UT_STAT_ERR_DOVE);
    ext_add_wave(a.stat + UT_STAT_ERR_CONT, err == UT_STAT_ERR_CONT);
}

__global__ __launch_bounds__(UT_THREADS) void unitig_out_kernel(UnitigArgs a)
{
    const u64 v = (u64)blockIdx.x * UT_THREADS + threadIdx.x;
    if (v >= 2 * a.nreads) return;
    u64 lo = a.off[v], hi = a.off[v + 1];
    if (hi > a.narcs) { hi = a.narcs; ut_broken(a); }    // (never: the offsets are searched in these records)
    const UtOut o = ut_out(a.keys, a.vals, lo, hi);
    a.deg[v] = o.deg; a.cand[v] = o.w; a.rep[v] = o.rep;
}

__global__ __launch_bounds__(UT_THREADS) void unitig_link_kernel(UnitigArgs a)
{
    const u64 v = (u64)blockIdx.x * UT_THREADS + threadIdx.x, nv = 2 * a.nreads;
    if (v >= nv) return;
    const u32 p = ut_pred(a.deg, a.cand, nv, (u32)v);
    a.pred[v] = p;
    ut_store(a.nxt + v, ut_init((u32)v, p, p == UT_NONE ? 0u : (u32)(a.rep[p] >> 32)));
}

__global__ __launch_bounds__(UT_THREADS) void unitig_round_kernel(UnitigArgs a)
{
    const u64 v = (u64)blockIdx.x * UT_THREADS + threadIdx.x, nv = 2 * a.nreads;
    if (v >= nv) return;
    const UtState mine = ut_load(a.cur + v);
    UtState theirs = mine;
    if (mine.ptr != UT_NONE && (u64)mine.ptr < nv) theirs = ut_load(a.cur + mine.ptr);
    ut_store(a.nxt + v, ut_step(mine, theirs));
}

__global__ __launch_bounds__(UT_THREADS) void unitig_cut_kernel(UnitigArgs a)
{
    const u64 v = (u64)blockIdx.x * UT_THREADS + threadIdx.x;
    if (v >= 2 * a.nreads) return;
    const UtState s = ut_load(a.cur + v);
    if (s.ptr == UT_NONE) return;
    const u32 p = a.pred[v];
    ut_store(a.nxt + v, ut_cut(s, (u32)v, p, p == UT_NONE ? 0u : (u32)(a.rep[p] >> 32)));       // (nxt == cur: in place)
}

// is v the first vertex of a unitig; *tail: the unitig's last vertex
__device__ __forceinline__ bool ut_head(const UnitigArgs &a, u64 v, u64 nv, UtState *mine, u32 *tail)
{
    if (v >= nv || ut_contained(a, v >> 1)) return false;
    *mine = ut_load(a.cur + v);
    if (mine->ptr != UT_NONE || mine->far != (u32)v) return false;      // a head is where its own window starts
    const UtState comp = ut_load(a.cur + (v ^ 1));
    if (!ut_canonical(*mine, comp)) return false;
    const u32 t = ut_tail(*mine, comp, a.pred[v]);
    *tail = t;
    if ((u64)t >= nv) { *tail = (u32)v; ut_broken(a); }  // (never: the tail of a chain is a vertex)
    return true;
}

template <bool EMIT>
__global__ __launch_bounds__(UT_THREADS) void unitig_heads_kernel(UnitigArgs a)
{
    __shared__ u64 s_scr[8];
    const u64 v = (u64)blockIdx.x * UT_THREADS + threadIdx.x, nv = 2 * a.nreads;
    UtState mine = ut_init(0, UT_NONE, 0); u32 tail = 0;
    const bool head = ut_head(a, v, nv, &mine, &tail);
    UtState ts = mine;
    if (head && tail != (u32)v) ts = ut_load(a.cur + tail);
    const u64 reads = head ? (u64)ts.cnt + 1 : 0;
    u64 tot_h, tot_r;
    const u64 eh = block_excl_scan_256<u64>(head ? 1 : 0, s_scr, &tot_h);
    const u64 er = block_excl_scan_256<u64>(reads, s_scr, &tot_r);
    if (!EMIT) {
        if (threadIdx.x == 0) { a.tile_heads[blockIdx.x] = tot_h; a.tile_reads[blockIdx.x] = tot_r; }
        return;
    }
    if (v >= nv) return;
    const u64 u = a.tile_heads[blockIdx.x] + eh, first = a.tile_reads[blockIdx.x] + er;
    const bool fits = head && u < a.nunitigs && first + reads <= a.nmembers;      // (always: the totals are the scans')
    a.uid[v] = fits ? (u32)u : UT_NONE;
    if (head && !fits) ut_broken(a);
    if (!fits) return;
    a.ufirst[v] = first;
    const bool circular = mine.cyc != UT_NONE;
    const u32 p = a.pred[v];
    u64 row[4];
    ut_unitig_row(row, first, reads, circular, ts.sum, a.rlen[tail >> 1], circular && p != UT_NONE ? (u32)(a.rep[p] >> 32) : 0u);
    reinterpret_cast<ulonglong2 *>(a.table)[2 * u] = make_ulonglong2(row[0], row[1]);
    reinterpret_cast<ulonglong2 *>(a.table)[2 * u + 1] = make_ulonglong2(row[2], row[3]);
}

__global__ __launch_bounds__(UT_THREADS) void unitig_layout_kernel(UnitigArgs a)
{
    const u64 v = (u64)blockIdx.x * UT_THREADS + threadIdx.x, nv = 2 * a.nreads;
    if (v >= nv || ut_contained(a, v >> 1)) return;
    const UtState s = ut_load(a.cur + v);
    if (s.ptr != UT_NONE || (u64)s.far >= nv) { ut_broken(a); return; }      // (never: every window has reached its head)
    const u32 u = a.uid[s.far];
    if (u == UT_NONE) return;                            // the complement chain is the unitig
    const u64 at = a.ufirst[s.far] + s.cnt;
    if (at >= a.nmembers) { ut_broken(a); return; }      // (never: a head's reads are its chain's vertices)
    u64 row[4];
    ut_layout_row(row, u, s.cnt, (u32)v, a.rid_base, s.sum, ut_succ(a.deg, a.cand, nv, (u32)v) == UT_NONE ? UT_NO_LINK : a.rep[v]);
    reinterpret_cast<ulonglong2 *>(a.layout)[2 * at] = make_ulonglong2(row[0], row[1]);
    reinterpret_cast<ulonglong2 *>(a.layout)[2 * at + 1] = make_ulonglong2(row[2], row[3]);
}

__device__ __forceinline__ void ut_add_sum(unsigned long long *word, u64 x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, WAVE);
    if (lane_id() == 0 && x) atomicAdd(word, (unsigned long long)x);
}

__global__ __launch_bounds__(UT_THREADS) void unitig_census_kernel(UnitigArgs a)
{
    const u64 stride = (u64)gridDim.x * UT_THREADS, nv = 2 * a.nreads;
    u64 links = 0, branch = 0, arcs = 0, live = 0, single = 0, circ = 0, longest = 0;
    for (u64 b = (u64)blockIdx.x * UT_THREADS; b < nv; b += stride) {
        const u64 v = b + threadIdx.x;
        if (v >= nv) continue;
        const bool alive = !ut_contained(a, v >> 1);
        const u32 d = a.deg[v];
        arcs += d; branch += alive && d > 1; live += alive && !(v & 1);
        links += ut_succ(a.deg, a.cand, nv, (u32)v) != UT_NONE;
    }
    for (u64 b = (u64)blockIdx.x * UT_THREADS; b < a.nunitigs; b += stride) {
        const u64 u = b + threadIdx.x;
        if (u >= a.nunitigs) continue;
        const u64 reads = a.table[4 * u + 1];
        single += reads == 1; circ += a.table[4 * u + 3] != 0; longest = reads > longest ? reads : longest;
    }
    ut_add_sum(a.stat + UT_STAT_LINKS, links); ut_add_sum(a.stat + UT_STAT_BRANCH, branch); ut_add_sum(a.stat + UT_STAT_ARCS, arcs); ut_add_sum(a.stat + UT_STAT_LIVE, live);
    ut_add_sum(a.stat + UT_STAT_SINGLE, single); ut_add_sum(a.stat + UT_STAT_CIRCULAR, circ);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u64 n1 = __shfl_xor(longest, o, WAVE); longest = n1 > longest ? n1 : longest; }
    if (lane_id() == 0 && longest) atomicMax(a.stat + UT_STAT_LONGEST, (unsigned long long)longest);
}

} // namespace hsk
