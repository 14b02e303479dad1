// hsk_pairfinish.h -- pair_finish_kernel: the first rung of the WEIGHTED finish for one-word keys (the {k-mer, count} pairs of the combining
// extraction, hsk_combine.h), without a hash table.
//
// agg_finish_kernel<cap, true> (hsk_agg.h) was built for k-mer instances: ~4000 records of ~120 distinct keys per bin.  The pairs of the
// combining extraction are nearly all distinct (312 M pairs for 308 M entries on the benchmark's shape), so a bin paid for clearing a table,
// a probe loop per pair, an occupancy scan over all slots and a compaction only to find each key once -- and then ordered the keys with the
// counting sort of the "many keys" branch anyway.  What the result needs is the order inside the bin, the sum of the few partial pairs that
// share a key, and the [L, U] filter.  This kernel does exactly that (the arithmetic: hsk_pairrank.h):
//   - the bin's n <= PF_CAP pairs go straight into registers (at most PF_PER per lane),
//   - a counting sort on the PF_LOG2BKT key bits below the bin prefix puts them bucket-major into LDS,
//   - every pair walks its own bucket once: its rank, whether it is the first arrival of its key (the head), the sum of the equal keys' counts,
//   - heads whose SUM passes [L, U] mark their rank in a bit mask; popcounts below the rank give the output slot,
//   - the entries go through LDS to the bin's slots in 16-byte stores from consecutive lanes, bin_cnt[b] = their number.
// That is what agg_emit_bin leaves behind: agg_scan_kernel, the host's read of flags and totals and agg_compact_kernel do not change.
// A bin of more than PF_CAP pairs is appended to the task's overflow list like a bin whose table ran full (agg_bin_overflow): the ladder's
// next rung (agg_finish_kernel<12, true>) takes it.
//
// Persistent workgroups: a workgroup walks a contiguous range of one task's bins (consecutive bins are consecutive in the records, the
// scratch and bin_cnt).  While bin b is ordered, the records of bin b + 1 and the bound of bin b + 2 are already on their way into a second
// set of registers; the barriers in between wait for LDS traffic only (lds_barrier), so one global round trip is hidden behind every bin's
// five barriers instead of three of them standing in front.  An empty bin costs one store.  Bins stay independent: no workgroup waits for another.
#pragma once
#include "hsk_agg.h"
#include "hsk_pairrank.h"

namespace hsk {

static_assert(PF_LANES == (u32)AG_THREADS, "hsk_pairrank.h counts the lanes of an aggregation workgroup");

__global__ __launch_bounds__(AG_THREADS) void pair_finish_kernel(AggArgs a)
{
    __shared__ u64 s_key[PF_CAP];       // the pairs bucket-major, then the kept entries in key order
    __shared__ u32 s_cnt[PF_CAP];
    __shared__ __attribute__((aligned(16))) u32 s_bkt[PF_NBKT];     // pairs per bucket (zero between two bins)
    __shared__ u32 s_start[PF_NBKT + 1]; // first place of every bucket, n behind the last
    __shared__ u32 s_bits[PF_WORDS];    // bit r: the pair of rank r is a kept head (zero between two bins)
    const AggTask &t = a.t[blockIdx.y];
    if (!t.active) return;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    const u32 b_lo = (u32)((u64)a.nbins * blockIdx.x / gridDim.x), b_hi = (u32)((u64)a.nbins * (blockIdx.x + 1) / gridDim.x);
    if (b_lo >= b_hi) return;
    const u64 *keys = t.keys, *vals = t.vals, *bounds = t.bounds;
    u64 *bin_cnt = t.bin_cnt;
    ulonglong2 *scratch = reinterpret_cast<ulonglong2 *>(t.scratch);
    const u32 slot_shift = t.slot_shift, lower = a.lower, upper = a.upper;
    const int shift = a.shift;

    for (u32 i = tid; i < PF_NBKT; i += AG_THREADS) s_bkt[i] = 0;
    if (tid < (int)PF_WORDS) s_bits[tid] = 0;

    // the bounds come through vector loads from an address the compiler cannot prove uniform: a scalar load would be waited for by the next
    // LDS barrier (one counter), a vector load only where its value is used
    u32 vz = 0;
    asm volatile("" : "+v"(vz));
    auto uniform64 = [](u64 v) -> u64 {
        return ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(v >> 32)) << 32) | (u32)__builtin_amdgcn_readfirstlane((int)(u32)v);
    };
    // the pairs [s, s + n) into a lane's registers: pair u * 256 + tid in slot u (n <= PF_CAP; whole slots are skipped by the wave)
    auto load_bin = [&](u64 s, u32 n, u64 (&k)[PF_PER], u32 (&c)[PF_PER]) {
#pragma unroll
        for (u32 u = 0; u < PF_PER; ++u) {
            k[u] = 0; c[u] = 0;
            if (u * PF_LANES < n) {
                const u32 i = u * PF_LANES + (u32)tid;
                if (i < n) { k[u] = keys[s + i]; c[u] = (u32)vals[s + i]; }
            }
        }
    };
    // n of a bin as the kernel uses it: 0, 1 .. PF_CAP, or PF_CAP + 1 for everything beyond
    auto bin_n = [](u64 s, u64 e) -> u32 { return e - s > (u64)PF_CAP ? PF_CAP + 1u : (u32)(e - s); };

    u64 s = uniform64(bounds[b_lo + vz]), e = uniform64(bounds[b_lo + 1 + vz]);
    u64 e_next = b_lo + 1 < b_hi ? bounds[b_lo + 2 + vz] : 0;       // (in flight)
    u64 k[PF_PER]; u32 c[PF_PER];
    {
        const u32 n0 = bin_n(s, e);
        load_bin(s, n0 <= PF_CAP ? n0 : 0u, k, c);
    }
    lds_barrier();

    for (u32 b = b_lo; b < b_hi; ++b) {
        const u32 n = bin_n(s, e);
        // ---- the next bin's records and the bound behind them are requested before this bin is ordered -----------------------------
        const bool more = b + 1 < b_hi;
        const u64 s2 = e, e2 = more ? uniform64(e_next) : e;
        const u32 n2 = bin_n(s2, e2);
        u64 nk[PF_PER]; u32 nc[PF_PER];
        load_bin(s2, n2 <= PF_CAP ? n2 : 0u, nk, nc);
        u64 e_nn = b + 2 < b_hi ? bounds[b + 3 + vz] : 0;

        if (n == 0) {
            if (tid == 0) bin_cnt[b] = 0;
        } else if (n > PF_CAP) {
            if (tid == 0) { agg_bin_overflow(t, a.nbins, b); atomicMax(t.flags + AG_BATCH, PF_CAP); }
        } else {
            // ---- 1. bucket and arrival index -----------------------------------------------------------------------------------------
            u32 ar[PF_PER];
#pragma unroll
            for (u32 u = 0; u < PF_PER; ++u) {
                ar[u] = 0;
                if (u * PF_LANES < n && u * PF_LANES + (u32)tid < n) ar[u] = atomicAdd(&s_bkt[pf_bucket(k[u], shift)], 1u);
            }
            lds_barrier();
            // every wave scans all buckets (eight per lane, no barrier inside) and writes its quarter of the starts
            {
                const uint4 v0 = reinterpret_cast<const uint4 *>(s_bkt)[lane * 2], v1 = reinterpret_cast<const uint4 *>(s_bkt)[lane * 2 + 1];
                const u32 v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                u32 sum = 0;
#pragma unroll
                for (int x = 0; x < 8; ++x) sum += v[x];
                u32 ex = wave_incl_scan_dpp(sum) - sum;
                if ((lane >> 4) == wave) {
#pragma unroll
                    for (int x = 0; x < 8; ++x) { s_start[lane * 8 + x] = ex; ex += v[x]; }
                    if (tid == AG_THREADS - 1) s_start[PF_NBKT] = ex;
                }
            }
            lds_barrier();
            // ---- the pairs bucket-major; the buckets are zero again for the next bin ---------------------------------------------------
#pragma unroll
            for (u32 u = 0; u < PF_PER; ++u)
                if (u * PF_LANES < n && u * PF_LANES + (u32)tid < n) {
                    const u32 at = s_start[pf_bucket(k[u], shift)] + ar[u];
                    s_key[at] = k[u]; s_cnt[at] = c[u];
                }
            for (u32 i = tid; i < PF_NBKT; i += AG_THREADS) s_bkt[i] = 0;
            lds_barrier();
            // ---- 2. - 4. a pair walks its bucket: rank, head of its run of equal keys, their summed count; kept heads mark their rank ---
            u32 keptm = 0;                              // bit u: the lane's pair u is a kept head; its rank replaces its arrival index in ar[u]
#pragma unroll
            for (u32 u = 0; u < PF_PER; ++u) {
                if (u * PF_LANES < n && u * PF_LANES + (u32)tid < n) {
                    const u32 bk = pf_bucket(k[u], shift), b0 = s_start[bk], b1 = s_start[bk + 1u];
                    PfRank r = {0, 0, 0};
                    for (u32 q = b0; q < b1; ++q) pf_see(r, k[u], ar[u], s_key[q], q - b0, s_cnt[q]);
                    ar[u] = pf_rank(b0, r); c[u] = r.sum;
                    if (pf_keep(r, lower, upper)) { keptm |= 1u << u; atomicOr(&s_bits[pf_word(ar[u])], pf_bit(ar[u])); }
                }
            }
            lds_barrier();
            // ---- 5. every wave scans the mask's words (one per lane); a kept head's slot is the number of marks below its own -----------
            const u32 word = s_bits[lane];
            const u32 pc = (u32)__builtin_popcount(word);
            const u32 incl = wave_incl_scan_dpp(pc);
            const u32 D = (u32)__builtin_amdgcn_readlane((int)incl, WAVE - 1);
#pragma unroll
            for (u32 u = 0; u < PF_PER; ++u) {
                if (u * PF_LANES < n) {                 // (whole waves take the two shuffles)
                    const u32 w = pf_word(ar[u]);
                    const u32 ww = (u32)__shfl((int)word, (int)w, WAVE), before = (u32)__shfl((int)(incl - pc), (int)w, WAVE);
                    if (keptm & (1u << u)) { const u32 o = pf_slot(before, ww, ar[u]); s_key[o] = k[u]; s_cnt[o] = c[u]; }
                }
            }
            lds_barrier();
            // ---- the entries in key order to the bin's slots (16-byte stores from consecutive lanes) -----------------------------------
            ulonglong2 *dst = scratch + (s >> slot_shift);
            for (u32 i = tid; i < D; i += AG_THREADS) dst[i] = make_ulonglong2(s_key[i], (u64)s_cnt[i]);
            if (tid == 0) bin_cnt[b] = D;
            if (tid < (int)PF_WORDS) s_bits[tid] = 0;
        }
        // ---- the next bin's registers become this bin's (here the loads are waited for) -------------------------------------------------
#pragma unroll
        for (u32 u = 0; u < PF_PER; ++u) { k[u] = nk[u]; c[u] = nc[u]; }
        s = s2; e = e2; e_next = e_nn;
    }
}

} // namespace hsk
