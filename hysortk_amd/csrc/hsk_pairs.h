// hsk_pairs.h -- read pairs that share k-mers, from the resident EXTENSION list (device).
//
// The first stage that reads a HSK_FLAG_KEEP_DEVICE result in place (include/hsk.h: hsk_result_pairs).  Every retained k-mer (an entry
// of the per-task CSR: cnt occurrences (rid, pos)) stands for cnt (cnt - 1) / 2 occurrence pairs; every pair of two DIFFERENT reads is
// one record { key = rid_a << 32 | rid_b, value = pos_a << 32 | pos_b }, rid_a < rid_b as unsigned 32-bit numbers.  The records of a
// task range are sorted by key with the library's radix sort (hsk_sort.h, key + payload), and every run of equal keys becomes one row
// { key, records of the run, smallest value, largest value }.
//
//   pair_tsum_kernel    t_e = cnt_e (cnt_e - 1) / 2 per entry, over all tasks of the range through one table of task descriptors:
//                       per tile sums, count_scan_kernel (hsk_count.h), then the exclusive 64-bit offset of every entry and where
//                       its payload slice lies.  Same-read pairs are NOT taken out here: the number of a record stays a closed
//                       form of the counts.
//   pair_expand_kernel  one record per lane slot, PX_TILE records per workgroup.  The workgroup finds the entry of its first record
//                       by binary search in the offsets (the LAST entry whose offset is <= the index: entries with cnt == 1 have
//                       no records and repeat their successor's offset), stages the offsets of the entries its tile touches in LDS,
//                       PX_STAGE at a time, every lane finds its entry there, turns the local index into (i, j) (hsk_pairdecode.h)
//                       and loads rid / pos at slice + i and slice + j: consecutive lanes walk i.  Key and value leave as full
//                       8-byte words per lane.  A pair inside one read is written as key 0 -- no record has it (rid_b >= 1) --
//                       so that it sorts to the front, leaves every digit as trivial as it was, and is counted by the reducer.
//                       The launch covers a WINDOW of the range's records, [rec0, rec0 + records) = entries [ent0, nent): the whole
//                       range for hsk_result_pairs, one slice of it for hsk_result_pairs_sliced (hsk_pairplan.h).
//                       ORIENTED (hsk_result_pairs_oriented): the XOR of the two occurrences' strand bits (hsk_strand.h) is bit 63 of the
//                       key; everything behind the expansion sees a key like any other.
//                       DIAG (hsk_result_pair_diagonals, hsk_pairdiag.h): the key has two words, the oriented key in the more significant
//                       word 1 and the sort word of the record's diagonal bin (hsk_diagbin.h) in word 0; a pair inside one read has both 0.
//   pair_reduce_kernel  the steps of hsk_runmask.h over keys staged in LDS: run heads of a tile as a bit mask, rows per tile,
//                       count_scan_kernel, write pass.  The last run of a tile may go on for any number of tiles (count, min, max
//                       reduced over the workgroup); tiles inside a run have no head and nothing to do.  The zero-key run is
//                       self_records and no row.
#pragma once
#include "hsk_device.h"
#include "hsk_count.h"
#include "hsk_runmask.h"
#include "hsk_pairdecode.h"
#include "hsk_diagbin.h"

namespace hsk {

// one task of the range that has entries (host: hsk_host_pairs.h).  128 bytes, a power of two: the kernels address the table with a shift
struct alignas(128) PairTask {
    const u64 *entries;      // n records of nw + 1 words, the count last
    const u64 *payoff;       // n: first payload of the entry in the rank's numbering
    const u32 *pos;          // npay
    const int32_t *rid;      // npay
    u64 ent_base;            // entries of the range's tasks before this one
    u64 n, npay, pay_base;   // entry i owns pos / rid[payoff[i] - pay_base ...][0 .. cnt_i)
    const u64 *strand;       // hsk_result_pairs_oriented: bit s & 63 of word s >> 6 = the strand of payload slot s (hsk_strand.h); NULL otherwise
};

constexpr int PAIR_THREADS = RM_THREADS;
constexpr int PC_EPT = 8, PC_TILE = PAIR_THREADS * PC_EPT;          // entries per thread / tile of pair_tsum_kernel
constexpr int PAIR_LOC_SHIFT = 40;                                  // loc = task slot << 40 | first payload inside the task (npay < 2^40)
constexpr u32 PAIR_ERR_COUNT = 1, PAIR_ERR_SLICE = 2;               // an entry's count above 65535 / its slice outside the task's payload

struct PairSumArgs {
    const PairTask *tasks; u32 ntasks; int nw;
    u64 nent;
    u64 *tile_sum;           // SUM out / WRITE in (after the scan: the tile's first record)
    u64 *off;                // WRITE: nent + 1
    u64 *loc;                // WRITE: nent
    u32 *err;
};

template <bool WRITE>
__global__ __launch_bounds__(PAIR_THREADS) void pair_tsum_kernel(PairSumArgs a)
{
    __shared__ u64 s_scr[8];
    const int tid = threadIdx.x;
    const u64 g0 = (u64)blockIdx.x * PC_TILE + (u64)tid * PC_EPT;
    u32 t[PC_EPT]; u64 loc[PC_EPT]; u64 sum = 0;
    u32 slot = 0;
    if (g0 < a.nent) {                                   // the task of this thread's first entry: the last one whose base is <= g0
        u32 lo = 0, hi = a.ntasks;
        while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (a.tasks[mid].ent_base <= g0) lo = mid; else hi = mid; }
        slot = lo;
    }
#pragma unroll
    for (int k = 0; k < PC_EPT; ++k) {
        const u64 g = g0 + k;
        t[k] = 0; loc[k] = 0;
        if (g >= a.nent) continue;
        while (g >= a.tasks[slot].ent_base + a.tasks[slot].n) ++slot;      // (every listed task has entries; g < nent ends the walk)
        const PairTask &tk = a.tasks[slot];
        const u64 l = g - tk.ent_base;
        const u64 cnt = tk.entries[l * (u64)(a.nw + 1) + a.nw];
        const u64 first = tk.payoff[l];
        if (cnt > PAIR_MAX_CNT) { if (!WRITE) atomicOr(a.err, PAIR_ERR_COUNT); continue; }
        if (first < tk.pay_base || first - tk.pay_base + cnt > tk.npay) { if (!WRITE) atomicOr(a.err, PAIR_ERR_SLICE); continue; }
        t[k] = pair_count((u32)cnt);
        loc[k] = ((u64)slot << PAIR_LOC_SHIFT) | (first - tk.pay_base);
        sum += t[k];
    }
    u64 total;
    u64 e = block_excl_scan_256<u64>(sum, s_scr, &total);
    if (!WRITE) { if (tid == 0) a.tile_sum[blockIdx.x] = total; return; }
    e += a.tile_sum[blockIdx.x];
#pragma unroll
    for (int k = 0; k < PC_EPT; ++k) {
        const u64 g = g0 + k;
        if (g < a.nent) { a.off[g] = e; a.loc[g] = loc[k]; e += t[k]; if (g + 1 == a.nent) a.off[a.nent] = e; }
    }
}

constexpr int PX_SLOTS = 4, PX_TILE = PAIR_THREADS * PX_SLOTS;      // records per lane / per workgroup
constexpr int PX_STAGE = 1024;                                       // entry offsets staged in LDS at a time

struct PairExpandArgs {
    const PairTask *tasks;
    const u64 *off, *loc;    // nent + 1, nent
    u64 nent, records;       // the window: entries [ent0, nent), records [rec0, rec0 + records) of the range -- off[ent0] == rec0, off[nent] == rec0 + records
    u64 *keys, *vals;        // records each: the window's record rec0 + i at [i]
    u64 rec0, ent0;          // both 0: the whole range (hsk_result_pairs); a slice otherwise (hsk_result_pairs_sliced)
    u64 diag_w;              // DIAG: the bin width, and a word that holds a bound of every position of the range (diag_maxpos_kernel); keys: 2 * records words
    const u64 *maxpos;
};

// ORIENTED (hsk_result_pairs_oriented): bit 63 of the key is the XOR of the two occurrences' strands -- read ids are below 2^31 there
// DIAG (hsk_result_pair_diagonals; with ORIENTED): record i's key is the 16 bytes { sort word of its bin, oriented key } at keys[2 i]
template <bool ORIENTED, bool DIAG = false>
__global__ __launch_bounds__(PAIR_THREADS) void pair_expand_kernel(PairExpandArgs a)
{
    static_assert(ORIENTED || !DIAG, "a diagonal needs the relative strand");
    __shared__ u64 s_off[PX_STAGE + 1];
    __shared__ u64 s_e0;
    const int tid = threadIdx.x;
    const u64 base = a.rec0 + (u64)blockIdx.x * PX_TILE;     // (record numbers are the range's; only the stores are relative to the window)
    const u64 last = a.rec0 + a.records;
    const u64 end = base + PX_TILE < last ? base + PX_TILE : last;
    if (tid == 0) {                                      // the last entry whose offset is <= base (off[ent0] = rec0 <= base < rec0 + records = off[nent])
        u64 lo = a.ent0, hi = a.nent;
        while (hi - lo > 1) { const u64 mid = (lo + hi) >> 1; if (a.off[mid] <= base) lo = mid; else hi = mid; }
        s_e0 = lo;
    }
    __syncthreads();
    u64 e_cur = s_e0;
    u64 ent[PX_SLOTS]; u32 r[PX_SLOTS]; bool found[PX_SLOTS];
#pragma unroll
    for (int s = 0; s < PX_SLOTS; ++s) { ent[s] = 0; r[s] = 0; found[s] = false; }
    const u32 maxpos = DIAG ? (u32)a.maxpos[0] : 0;
    for (;;) {
        // entries e_cur .. e_cur + m - 1 and the offset behind them; a record not found yet lies at or behind s_off[0]
        const u32 m = (u32)(a.nent - e_cur < (u64)PX_STAGE ? a.nent - e_cur : (u64)PX_STAGE);
        for (u32 k = tid; k <= m; k += PAIR_THREADS) s_off[k] = a.off[e_cur + k];
        __syncthreads();
        const u64 hi_off = s_off[m];
#pragma unroll
        for (int s = 0; s < PX_SLOTS; ++s) {
            const u64 idx = base + (u64)s * PAIR_THREADS + tid;
            if (idx < end && !found[s] && idx < hi_off) {
                u32 lo = 0, hi = m;                       // s_off[lo] <= idx < s_off[hi]
                while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (s_off[mid] <= idx) lo = mid; else hi = mid; }
                ent[s] = e_cur + lo; r[s] = (u32)(idx - s_off[lo]); found[s] = true;
            }
        }
        const bool fin = hi_off >= end || e_cur + m >= a.nent;
        __syncthreads();
        if (fin) break;
        // The first record not found yet is number hi_off.  Its entry may lie any number of entries without records further on (cnt == 1:
        // equal offsets): thread 0 searches for it instead of the workgroup walking there, so that every step finds at least one record
        // and a tile takes at most as many steps as it has records.
        if (tid == 0) {                                  // the last entry whose offset is <= hi_off (off[e_cur + m] == hi_off)
            u64 lo = e_cur + m, hi = a.nent;
            while (hi - lo > 1) { const u64 mid = (lo + hi) >> 1; if (a.off[mid] <= hi_off) lo = mid; else hi = mid; }
            s_e0 = lo;
        }
        __syncthreads();
        e_cur = s_e0;
    }
#pragma unroll
    for (int s = 0; s < PX_SLOTS; ++s) {
        const u64 idx = base + (u64)s * PAIR_THREADS + tid;
        if (!found[s]) continue;
        const u64 L = a.loc[ent[s]];
        const PairTask &tk = a.tasks[L >> PAIR_LOC_SHIFT];
        const u64 first = L & ((1ULL << PAIR_LOC_SHIFT) - 1);
        u32 i, j; pair_decode(r[s], &i, &j);
        u32 ra = (u32)tk.rid[first + i], rb = (u32)tk.rid[first + j];
        u32 pa = tk.pos[first + i], pb = tk.pos[first + j];
        if (ra > rb) { const u32 x = ra; ra = rb; rb = x; const u32 y = pa; pa = pb; pb = y; }
        const bool self = ra == rb;
        u64 o = 0;
        if (ORIENTED) { const u64 si = first + i, sj = first + j; o = ((tk.strand[si >> 6] >> (si & 63)) ^ (tk.strand[sj >> 6] >> (sj & 63))) << 63; }
        const u64 key = self ? 0ULL : o | ((u64)ra << 32) | rb;
        if (DIAG) {
            typedef unsigned long long v2u64x __attribute__((ext_vector_type(2)));
            const v2u64x kk = {self ? 0ULL : diag_sort_word(o >> 63, pa, pb, maxpos, a.diag_w), key};
            *(v2u64x *)(a.keys + 2 * (idx - a.rec0)) = kk;
        } else a.keys[idx - a.rec0] = key;
        a.vals[idx - a.rec0] = self ? 0ULL : ((u64)pa << 32) | pb;
    }
}

constexpr int PR_PPT = 8, PR_TILE = PAIR_THREADS * PR_PPT, PR_WORDS = PR_TILE / 64;
constexpr int PR_AHEAD = 4;                              // records per lane and step of the read-ahead
constexpr int PAIR_ROW_WORDS = 4;                        // { key, shared, first, last }
enum { PAIR_STAT_RECORDS = 0, PAIR_STAT_ROWS, PAIR_STAT_SELF, PAIR_STAT_KEYS, PAIR_STAT_ERR, PAIR_STAT_WORDS = 8 };

struct PairReduceArgs {
    const u64 *keys, *vals;  // sorted by key, n each
    u64 n;
    u32 min_shared;
    u64 *tile_cnt;           // COUNT out / EMIT in (after the scan: the tile's first row)
    u64 *tile_keys;          // COUNT out: runs of the tile with a key other than 0 (summed by a scan of their own: no atomics on one word)
    u64 *rows;               // EMIT: { key, shared, first, last }
    u64 *stats;              // COUNT: [PAIR_STAT_SELF] records of the zero-key run
};

template <bool EMIT>
__global__ __launch_bounds__(PAIR_THREADS) void pair_reduce_kernel(PairReduceArgs a)
{
    __shared__ u64 s_k[PR_TILE + 1];                     // [0] = the record before the tile
    __shared__ u64 s_v[EMIT ? PR_TILE : 1];
    __shared__ u64 s_head[PR_WORDS], s_keep[PR_WORDS];
    __shared__ u32 s_pre[PR_WORDS + 1];
    __shared__ u64 s_red[4][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 base = (u64)blockIdx.x * PR_TILE;
    const u32 tn = (u32)(a.n - base < (u64)PR_TILE ? a.n - base : (u64)PR_TILE);
    const u64 obase = EMIT ? a.tile_cnt[blockIdx.x] : 0;
    for (u32 i = tid; i < tn + 1; i += PAIR_THREADS) s_k[i] = (base + i) ? a.keys[base + i - 1] : 0;
    if (EMIT) for (u32 i = tid; i < tn; i += PAIR_THREADS) s_v[i] = a.vals[base + i];
    __syncthreads();
    bool head[PR_PPT];
#pragma unroll
    for (int j = 0; j < PR_PPT; ++j) {
        const u32 p = j * PAIR_THREADS + tid;
        head[j] = p < tn && ((base + p == 0) || s_k[p + 1] != s_k[p]);
        rm_publish(s_head, j, __ballot(head[j]));
    }
    __syncthreads();
    const int p_last = rm_last_head<PR_WORDS>(s_head);
    if (p_last < 0) { if (!EMIT && tid == 0) { a.tile_cnt[blockIdx.x] = 0; a.tile_keys[blockIdx.x] = 0; } return; }      // the tile lies inside a run that started before it

    // ---- the tile's last run: the workgroup follows it to its end --------------------------------------------------
    const u64 key_last = s_k[p_last + 1];
    RunAcc L;
    for (u32 i = p_last + tid; i < tn; i += PAIR_THREADS) L.take<EMIT>(EMIT ? s_v[i] : 0);
    rm_follow<PR_AHEAD>(base + tn, a.n, [&](u64 gi) {
        const u64 k = a.keys[gi];
        const u64 v = EMIT ? a.vals[gi] : 0;
        if (k != key_last) return false;
        L.take<EMIT>(v);
        return true;
    });
    rm_reduce_run<EMIT>(L, s_red);

    // ---- run lengths, the min_shared filter ----------------------------------------------------------------------------
    u64 runlen[PR_PPT];
    u32 nkeys = 0;
#pragma unroll
    for (int j = 0; j < PR_PPT; ++j) {
        const u32 p = j * PAIR_THREADS + tid;
        u64 c = 0; bool real = false;
        if (head[j]) {
            c = p == (u32)p_last ? L.n : rm_next_head(s_head, p) - p;
            real = s_k[p + 1] != 0;
            if (!EMIT && !real) a.stats[PAIR_STAT_SELF] = c;
        }
        const bool keep = real && c >= a.min_shared;
        runlen[j] = keep ? c : 0;
        rm_publish(s_keep, j, __ballot(keep));
        if (!EMIT) nkeys += (u32)__popcll(__ballot(real));
    }
    __syncthreads();                                      // (s_red has been read by every wave)
    if (!EMIT && lane == 0) s_red[wave][0] = nkeys;
    __syncthreads();
    rm_prefix<PR_WORDS>(s_keep, s_pre);
    __syncthreads();
    if (!EMIT) { if (tid == 0) { a.tile_cnt[blockIdx.x] = s_pre[PR_WORDS]; a.tile_keys[blockIdx.x] = s_red[0][0] + s_red[1][0] + s_red[2][0] + s_red[3][0]; } return; }

    // ---- rows: slot = popcount prefix of the kept heads, so the list stays in key order ----------------------------------
#pragma unroll
    for (int j = 0; j < PR_PPT; ++j) {
        const u64 c = runlen[j];
        if (!c) continue;
        const u32 p = j * PAIR_THREADS + tid;
        RunAcc r = L;
        if (p != (u32)p_last) r.span(s_v, p, (u32)c);
        typedef unsigned long long v2u64r __attribute__((ext_vector_type(2)));
        v2u64r *row = (v2u64r *)(a.rows + (obase + rm_slot(s_keep, s_pre, j)) * PAIR_ROW_WORDS);
        const v2u64r r0 = {s_k[p + 1], c}, r1 = {r.mn, r.mx};
        row[0] = r0; row[1] = r1;
    }
}

} // namespace hsk
