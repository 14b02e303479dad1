// hsk_strand.h -- the strand of every k-mer occurrence of a resident EXTENSION result (device; include/hsk.h: hsk_result_strands).
//
// The payload (ReadId, PosInRead) carries no strand, but the entry that owns a payload slot holds the canonical k-mer, and the read's K
// bases at the position spell either it or its reverse complement (hsk_strandbits.h).  One more gather over the payload, with the reads
// still in HBM, gives one bit per payload slot: bit s & 63 of word s >> 6 of the task's array is the strand of slot s, 0 for the gaps
// that filtered k-mers leave.
//
//   strand_kernel  payload slots to lanes, ST_TILE slots of ONE task per workgroup, through one launch over the table of task
//                  descriptors (PairTask, hsk_pairs.h) and the first tile and first bit word of each (StrandSpan).  64 consecutive slots
//                  are one wave: their strands are one __ballot, and one lane stores the word -- no atomics on the bit array and no
//                  memset, tasks start on a word boundary.  The first payload of an entry ascends inside a task and every entry has a
//                  payload (count_kernel: the run's start in the sorted array, hsk_count.h; agg_ext_kernel: the bin's start plus the
//                  prefix of the counts in key order, hsk_agg.h): the workgroup finds the last entry that starts at or before its
//                  tile's first slot by binary search, stages the first payload and the count of the at most ST_TILE + 1 entries its tile
//                  touches in LDS, and every lane searches there.  A slot at or behind first + cnt is a gap and is never read as
//                  (rid, pos).  An owned slot loads rid / pos (adjacent lanes, adjacent addresses), the read's offset and length, and the
//                  read's K bases as aligned 32-bit words -- the random gather of the pass.  Bad input raises bits of one error word and
//                  never an out-of-range access.  payloads / reverse / palindromes: ballots per wave, LDS per workgroup, three atomics.
#pragma once
#include "hsk_device.h"
#include "hsk_pairs.h"
#include "hsk_strandbits.h"

namespace hsk {

constexpr int ST_THREADS = 256, ST_SLOTS = 4, ST_TILE = ST_THREADS * ST_SLOTS;      // payload slots per lane / per workgroup
constexpr int ST_STAGE = ST_TILE + 1;                                                // entries a tile can touch
static_assert(ST_TILE % 64 == 0, "a tile starts on a word of the bit array");
// an owned slot whose read id lies outside the reads given / whose k-mer runs past its read / whose read lies outside the packed buffer /
// whose bases are neither the entry's k-mer nor its reverse complement
constexpr u32 STRAND_ERR_RID = 1, STRAND_ERR_POS = 2, STRAND_ERR_INDEX = 4, STRAND_ERR_MISMATCH = 8;
enum { STRAND_STAT_PAYLOADS = 0, STRAND_STAT_REVERSE, STRAND_STAT_PALINDROMES, STRAND_STAT_ERR, STRAND_STAT_WORDS = 8 };

struct StrandSpan { u64 tile0, word0; };               // of a listed task: its first workgroup, its first word in `bits`; [ntasks]: the totals

struct StrandArgs {
    const PairTask *tasks; const StrandSpan *span; u32 ntasks; int k;
    const u8 *packed; u64 packed_bytes;                  // 4-byte aligned
    const u64 *roff; const u32 *rlen; u64 nreads;
    int64_t rid_base;
    u64 *bits;
    unsigned long long *stats;                           // STRAND_STAT_*
};

template <int NW>
__global__ __launch_bounds__(ST_THREADS) void strand_kernel(StrandArgs a)
{
    __shared__ u64 s_off[ST_STAGE];
    __shared__ u32 s_cnt[ST_STAGE];
    __shared__ u64 s_e0;
    __shared__ u32 s_red[4][4];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u32 slot = 0;                                        // the task of this workgroup: the last one whose first tile is <= blockIdx.x
    { u32 hi = a.ntasks; while (hi - slot > 1) { const u32 mid = (slot + hi) >> 1; if (a.span[mid].tile0 <= blockIdx.x) slot = mid; else hi = mid; } }
    const PairTask &tk = a.tasks[slot];
    const u64 s0 = ((u64)blockIdx.x - a.span[slot].tile0) * ST_TILE;
    u64 *words = a.bits + a.span[slot].word0;
    if (tid == 0) {                                      // the last entry that starts at or before s0; entry 0 if none does
        u64 lo = 0, hi = tk.n;
        while (lo < hi) { const u64 mid = (lo + hi) >> 1; if (tk.payoff[mid] - tk.pay_base <= s0) lo = mid + 1; else hi = mid; }
        s_e0 = lo ? lo - 1 : 0;
    }
    __syncthreads();
    const u64 e0 = s_e0;
    // entries e0 .. e0 + m - 1: the next one starts behind the one before it, so entry e0 + ST_TILE starts at or behind s0 + ST_TILE
    const u32 m = (u32)(tk.n - e0 < (u64)ST_STAGE ? tk.n - e0 : (u64)ST_STAGE);
    for (u32 i = tid; i < m; i += ST_THREADS) {
        s_off[i] = tk.payoff[e0 + i] - tk.pay_base;
        const u64 c = tk.entries[(e0 + i) * (u64)(NW + 1) + NW];
        s_cnt[i] = c > 0xffffffffULL ? 0xffffffffu : (u32)c;
    }
    __syncthreads();
    u32 n_own = 0, n_rev = 0, n_pal = 0, err = 0;
#pragma unroll
    for (int j = 0; j < ST_SLOTS; ++j) {
        const u64 wbase = s0 + (u64)j * ST_THREADS + wave * 64;      // (the same in every lane of the wave)
        const u64 s = wbase + lane;
        bool own = false, rev = false, pal = false;
        u64 ent = 0;
        if (s < tk.npay) {
            u32 lo = 0, hi = m;                          // the staged entries that start at or before s
            while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (s_off[mid] <= s) lo = mid + 1; else hi = mid; }
            if (lo && s - s_off[lo - 1] < (u64)s_cnt[lo - 1]) { own = true; ent = e0 + lo - 1; }
        }
        if (own) {
            const int64_t r = (int64_t)tk.rid[s] - a.rid_base;
            const u32 p = tk.pos[s];
            if (r < 0 || (u64)r >= a.nreads) err |= STRAND_ERR_RID;
            else {
                const u64 off = a.roff[r];
                const u32 len = a.rlen[r];
                if ((u64)p + (u64)a.k > (u64)len) err |= STRAND_ERR_POS;
                else if (off > a.packed_bytes || ((u64)len + 3) / 4 > a.packed_bytes - off) err |= STRAND_ERR_INDEX;
                else {
                    u64 f[NW], e[NW];
                    strand_load<NW>(a.packed, a.packed_bytes, 8 * off + 2 * (u64)p, a.k, f);
#pragma unroll
                    for (int w = 0; w < NW; ++w) e[w] = tk.entries[ent * (u64)(NW + 1) + w];
                    const int d = strand_decide<NW>(f, e, a.k);
                    if (d == STRAND_MISMATCH) err |= STRAND_ERR_MISMATCH;
                    rev = d == STRAND_REVERSE; pal = d == STRAND_PALINDROME;
                }
            }
        }
        const u64 mrev = __ballot(rev);
        n_own += (u32)__popcll(__ballot(own)); n_rev += (u32)__popcll(mrev); n_pal += (u32)__popcll(__ballot(pal));
        if (lane == 0 && wbase < tk.npay) words[wbase >> 6] = mrev;
    }
    u32 werr = 0;
#pragma unroll
    for (u32 b = 1; b <= STRAND_ERR_MISMATCH; b <<= 1) if (__any((int)(err & b))) werr |= b;
    if (lane == 0) { s_red[wave][0] = n_own; s_red[wave][1] = n_rev; s_red[wave][2] = n_pal; s_red[wave][3] = werr; }
    __syncthreads();
    if (tid < 4) {
        u32 v = tid < 3 ? s_red[0][tid] + s_red[1][tid] + s_red[2][tid] + s_red[3][tid] : s_red[0][3] | s_red[1][3] | s_red[2][3] | s_red[3][3];
        if (v) { if (tid < 3) atomicAdd(a.stats + tid, (unsigned long long)v); else atomicOr(a.stats + STRAND_STAT_ERR, (unsigned long long)v); }
    }
}

} // namespace hsk
