// hsk_rowmerge.h -- two-way merge of row lists in HBM: the four-word rows of the read pairs and the six-word all-bins rows of the read
// pairs by diagonal (host: hsk_host_pairs.h, hsk_host_pairdiag.h).  One kernel template over the row's shape.
//
// A row is WORDS u64 words (include/hsk.h):
//   PairRow  { key, shared, first, last }                  hsk_pairs           compared on key
//   DiagRow  { key, support, bin, support, first, last }   hsk_pair_diags, all_bins   compared on (key, bin), two unsigned words
// A list is ascending by its compare words as unsigned 64-bit numbers and holds them at most once.  The merge of lists A and B is ascending
// with one row per compare key; a key of both lists gives one JOINED row: the summed word (both copies of it) = the sum, first = the
// unsigned minimum, last = the unsigned maximum (mp_join).  min_count (the final merge only) drops the rows whose joined sum is below
// it; the rows before that filter are counted too (hsk_pairs::keys, hsk_pair_diags::bins), and for DiagRow so are the distinct keys among
// them (hsk_pair_diags::keys).
//
//   Merge path.  The MERGED SEQUENCE is all na + nb rows in order, A's copy of a key in front of B's (the tie rule).  Workgroup t takes
//   positions [t * TILE, (t + 1) * TILE) of it.  Position d splits into (ai, d - ai) with ai = the number of A rows among the first d:
//   the smallest i for which A[i] comes behind B[d - 1 - i], found by bisection over the rows in HBM (mp_split; two lanes: the tile's
//   first and last diagonal).  The tile's share is A[a0, a1) and B[b0, b1), at most TILE rows together.
//
//   Who owns a key of both lists.  By the tie rule B's copy is the position right behind A's copy.  The row belongs to the tile that
//   holds A'S COPY: it joins the next position's row, and where A's copy is the tile's last position that row is B[b1], one row past
//   the tile's share -- the tile stages it as well (the look-ahead).  B's copy is dropped by whoever holds it: it is the B row whose
//   previous position has its key, and for the tile's first position that is A[a0 - 1], staged too (the look-behind).  Both passes run
//   the same code on the same splits, so COUNT and EMIT agree wherever the diagonal falls.
//
//   In LDS.  A[a0 - 1 .. a1) and B[b0 .. b1] come in as 16-byte vectors, consecutive lanes on consecutive addresses, and are laid out
//   word by word (the searches walk the compare words only); the second copy of the summed word is not kept.  Every row finds its position
//   by one bisection in the other list's share: A[i] goes to i + (B rows before it), B[j] to j + (A rows before it or tied with it).
//   s_src[position] = where the row lies.  Then every lane takes TILE / 256 consecutive positions: dropped / joined by the neighbours'
//   keys, the filter, a workgroup scan of the kept rows.  COUNT leaves its counts per tile; count_scan_kernel (hsk_count.h) turns the kept
//   rows into the tile's first output row; EMIT builds the rows in registers, writes them back into LDS at their slots (the staged rows
//   are dead by then) and stores them 16 bytes per lane.  No atomics: the output is ordered by construction.
//
//   Key heads (DiagRow, COUNT).  The rows before the filter whose key differs from the key at the position in front of them.  For the
//   tile's first position that is the later of A[a0 - 1] and B[b0 - 1]; both are at or below the row, so the row is a head exactly when
//   neither has its key.  A[a0 - 1] is the look-behind; the key of B[b0 - 1] is one more word.  PairRow has no such count: a key is a row.
//
// The kernel moves WORDS * 8 bytes per input row in each pass and per output row; COUNT skips the last vector of every row (first, last).
//
// The parts that need no HIP -- the traits, mp_before, mp_same, the merge-path split mp_split, the join rule mp_join -- are shared with the
// CPU test (tests/rowmerge_test.cpp), as hsk_diagbin.h's are.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define HSK_MP_FN __host__ __device__ inline
#else
#define HSK_MP_FN inline
#endif

namespace hsk {

// A row's shape.  CMP0, CMP1: the compare words (NCMP of them count).  SUM: the summed word, SUM2: its second copy (WORDS: there is none).
// first / last are the row's last vector.  TILE: positions of the merged sequence per workgroup (why these).  NTILE:
// the tile arrays COUNT fills -- kept rows, [key heads,] rows before the filter.  COUNT_ONE: a single list's counts need a merge with
// nothing (DiagRow: its keys are not its rows).
struct PairRow {
    static constexpr int WORDS = 4, NCMP = 1, CMP0 = 0, CMP1 = 0, SUM = 1, SUM2 = WORDS;
    static constexpr int TILE = 1024, NTILE = 2;
    static constexpr bool HEADS = false, COUNT_ONE = false;
};
struct DiagRow {
    static constexpr int WORDS = 6, NCMP = 2, CMP0 = 0, CMP1 = 2, SUM = 1, SUM2 = 3;
    static constexpr int TILE = 512, NTILE = 3;
    static constexpr bool HEADS = true, COUNT_ONE = true;
};

// what a row is compared on; b stays 0 where one word is compared
struct MpKey { uint64_t k, b; };
// of the row whose word w lies at row[w * stride] (in HBM: stride 1)
template <typename Row>
HSK_MP_FN MpKey mp_key(const uint64_t *row, uint32_t stride = 1) { const MpKey x = {row[Row::CMP0 * stride], Row::NCMP == 2 ? row[Row::CMP1 * stride] : 0}; return x; }

// does x come before y?  unsigned words
HSK_MP_FN bool mp_before(MpKey x, MpKey y) { return x.k < y.k || (x.k == y.k && x.b < y.b); }
HSK_MP_FN bool mp_same(MpKey x, MpKey y) { return x.k == y.k && x.b == y.b; }
template <typename Row> HSK_MP_FN bool mp_before(const uint64_t *ra, const uint64_t *rb) { return mp_before(mp_key<Row>(ra), mp_key<Row>(rb)); }
template <typename Row> HSK_MP_FN bool mp_same(const uint64_t *ra, const uint64_t *rb) { return mp_same(mp_key<Row>(ra), mp_key<Row>(rb)); }

// The number of A rows among the first d positions of the merged sequence (0 <= d <= na + nb): the smallest i for which A[i] does not
// come before or tie with B[d - 1 - i] (a tie puts A's copy in front).  The result lies in [max(d - nb, 0), min(d, na)] whatever the rows hold.
template <typename Row>
HSK_MP_FN uint64_t mp_split(const uint64_t *a, uint64_t na, const uint64_t *b, uint64_t nb, uint64_t d)
{
    uint64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);      // mid < na, and 0 <= d - 1 - mid < nb
        if (!mp_before<Row>(b + (d - 1 - mid) * Row::WORDS, a + mid * Row::WORDS)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the joined row of two rows with one key: (sum, first, last) takes (sum2, first2, last2) in
HSK_MP_FN void mp_join(uint64_t &sum, uint64_t &first, uint64_t &last, uint64_t sum2, uint64_t first2, uint64_t last2)
{
    sum += sum2;
    first = first2 < first ? first2 : first;
    last = last2 > last ? last2 : last;
}

} // namespace hsk

#if defined(__HIPCC__)
#include "hsk_device.h"

namespace hsk {

constexpr int MP_THREADS = 256;                          // (the workgroup scan is block_excl_scan_256)

template <typename Row>
struct RowMergeArgs {
    const u64 *a, *b;        // na / nb rows, 16-byte aligned
    u64 na, nb;
    u32 min_count;
    u64 *tile[Row::NTILE];   // COUNT out: [0] the kept rows (EMIT in, after the scan: the tile's first row), [NTILE - 1] the rows before
                             // min_count, and between them (DiagRow) the key heads before min_count
    u64 *rows;               // EMIT
};

typedef unsigned long long mp_v2 __attribute__((ext_vector_type(2)));

// The LDS word of row word w: the words in front of the summed word's second copy keep their number, the ones behind it move down.  A
// vector's two words go through this by arithmetic, in the staging and in the stores alike: one block of LDS, word w of staged row i at
// [w * ROWS + i].  (Separate arrays and a branch per vector were compiled, for six-word rows, into two merged LDS stores of which the second
// wrote v.x again for the third vector: `last` came out as `first`.  hipcc of ROCm 7.2, -O3, gfx950; the tests' exact rows check the code object.)
template <typename Row>
__device__ constexpr u32 mp_lds_word(u32 w) { return w == (u32)Row::SUM2 ? (u32)Row::SUM : w - (w > (u32)Row::SUM2 ? 1u : 0u); }

// stage nvec vectors from g: vector q is word pair q % VECS of the row at index r0 + q / VECS
template <typename Row, bool EMIT>
__device__ __forceinline__ void mp_stage(u64 *s_w, const mp_v2 *g, u32 nvec, u32 r0, int tid)
{
    constexpr u32 VECS = Row::WORDS / 2, ROWS = Row::TILE + 2;
    for (u32 q = tid; q < nvec; q += MP_THREADS) {
        const u32 rq = q / VECS, w = (q - rq * VECS) * 2, r = r0 + rq;
        if (!EMIT && w == (u32)Row::WORDS - 2) continue;     // COUNT needs no first / last
        const mp_v2 v = g[q];
        s_w[mp_lds_word<Row>(w) * ROWS + r] = v.x;
        if (w + 1 != (u32)Row::SUM2) s_w[mp_lds_word<Row>(w + 1) * ROWS + r] = v.y;
    }
}

template <typename Row, bool EMIT>
__global__ __launch_bounds__(MP_THREADS) void row_merge_kernel(RowMergeArgs<Row> p)
{
    constexpr int WORDS = Row::WORDS, VECS = WORDS / 2, TILE = Row::TILE, PPT = TILE / MP_THREADS, ROWS = TILE + 2;      // + look-behind + look-ahead
    constexpr int KEPT = Row::SUM2 < WORDS ? WORDS - 1 : WORDS;                // words of a row in LDS: all of them (EMIT), all but first / last (COUNT)
    constexpr int W_SUM = Row::SUM, W_FI = EMIT ? KEPT - 2 : 0, W_LA = EMIT ? KEPT - 1 : 0;      // (COUNT never touches first / last)
    static_assert((TILE & (TILE - 1)) == 0 && TILE <= 4096 && TILE % MP_THREADS == 0, "tile of the merge");
    static_assert(WORDS % 2 == 0 && Row::NTILE == (Row::HEADS ? 3 : 2), "the row's shape");
    static_assert(Row::SUM2 == WORDS || (Row::SUM2 % 2 == 1 && Row::SUM2 < WORDS - 2), "the sum's second copy is the second word of a vector in front of first / last");
    static_assert(Row::CMP0 < Row::SUM2 && Row::CMP1 < Row::SUM2 && Row::SUM < Row::SUM2, "the compare words and the sum keep their number in LDS");
    // row i of the A side lies at index i - (a0 - 1): [0] is the look-behind; the B side follows at bbase, the look-ahead last
    __shared__ u64 s_w[(EMIT ? KEPT : KEPT - 2) * ROWS];
    __shared__ u16 s_src[TILE];
    __shared__ u64 s_cut[2];
    __shared__ u32 s_scr[8];
    const int tid = threadIdx.x;
    const u64 total = p.na + p.nb;
    const u64 d0 = (u64)blockIdx.x * TILE, d1 = d0 + TILE < total ? d0 + TILE : total;
    if (tid < 2) s_cut[tid] = mp_split<Row>(p.a, p.na, p.b, p.nb, tid ? d1 : d0);
    __syncthreads();
    const u64 a0 = s_cut[0];
    u64 a1 = s_cut[1];
    {   // Ascending lists give a0 <= a1 <= a0 + (d1 - d0).  Lists that break the contract give wrong rows, never a share outside the lists:
        // a1 is held to that range (which meets mp_split's own [d1 - nb, min(d1, na)] whatever the rows are).
        const u64 lo = a0 > (d1 > p.nb ? d1 - p.nb : 0) ? a0 : (d1 > p.nb ? d1 - p.nb : 0);
        u64 hi = a0 + (d1 - d0); if (hi > p.na) hi = p.na; if (hi > d1) hi = d1;
        a1 = a1 < lo ? lo : a1 > hi ? hi : a1;
    }
    const u64 b0 = d0 - a0, b1 = d1 - a1;
    const u32 nap = (u32)(a1 - a0), nbp = (u32)(b1 - b0), nt = nap + nbp;      // nt = d1 - d0 <= TILE
    const bool behind = a0 > 0, ahead = b1 < p.nb;
    const u32 bbase = 1 + nap, la = bbase + nbp;         // la <= TILE + 1 < ROWS
    // key heads: the key in front of the tile's first B row (the same word for every lane; the tile's first position uses it)
    u64 kb_behind = 0;
    bool b_behind = false;
    if constexpr (!EMIT && Row::HEADS) { b_behind = b0 > 0; if (b_behind) kb_behind = p.b[(b0 - 1) * WORDS + Row::CMP0]; }

    // ---- stage (without a look-behind index 0 stays empty) -----------------------------------------------------------------------
    mp_stage<Row, EMIT>(s_w, (const mp_v2 *)(p.a + (a0 - (behind ? 1 : 0)) * WORDS), (nap + (behind ? 1 : 0)) * VECS, behind ? 0 : 1, tid);
    mp_stage<Row, EMIT>(s_w, (const mp_v2 *)(p.b + b0 * WORDS), (nbp + (ahead ? 1 : 0)) * VECS, bbase, tid);
    __syncthreads();

    // ---- every row's position inside the tile ----------------------------------------------------------------------------------
    for (u32 e = tid; e < nt; e += MP_THREADS) {
        u32 pos, idx;
        if (e < nap) {                                   // A[a0 + e]: behind the B rows that come before it
            idx = 1 + e;
            const MpKey k = mp_key<Row>(s_w + idx, ROWS);
            u32 lo = 0, hi = nbp;
            while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (mp_before(mp_key<Row>(s_w + bbase + mid, ROWS), k)) lo = mid + 1; else hi = mid; }
            pos = e + lo;
        } else {                                         // B[b0 + j]: behind the A rows that come before it or tie with it
            const u32 j = e - nap;
            idx = bbase + j;
            const MpKey k = mp_key<Row>(s_w + idx, ROWS);
            u32 lo = 0, hi = nap;
            while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (!mp_before(k, mp_key<Row>(s_w + 1 + mid, ROWS))) lo = mid + 1; else hi = mid; }
            pos = j + lo;
        }
        s_src[pos] = (u16)idx;                           // (pos < nt: the positions of the tile's rows are a permutation of 0 .. nt - 1)
    }
    __syncthreads();

    // ---- PPT consecutive positions per lane: dropped, joined, kept ---------------------------------------------------------------
    u64 rw[PPT][KEPT];                                   // the kept rows, by LDS word (COUNT: never read)
    u32 nrows = 0, nheads = 0, nkept = 0, keptm = 0;
    // (s_src is a permutation for lists that keep the contract; whatever it holds, the index stays inside the staged rows)
    const auto src = [&](u32 q) -> u32 { const u32 v = s_src[q]; return v < la ? v : la; };
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        const u32 pos = (u32)tid * PPT + i;
        if (pos >= nt) continue;
        const u32 idx = src(pos);
        const MpKey k = mp_key<Row>(s_w + idx, ROWS);
        u64 sum = s_w[W_SUM * ROWS + idx], f = 0, l = 0;
        // the position in front (inside the tile, or A's look-behind): B rows look at it, and every row where key heads are counted
        constexpr bool FRONT_ALL = !EMIT && Row::HEADS;
        u32 pv = 0;
        bool has_pv = false;
        const auto look_front = [&] { pv = pos > 0 ? src(pos - 1) : 0; has_pv = pos > 0 || behind; };
        if constexpr (FRONT_ALL) look_front();
        if (idx >= bbase) {                              // a B row: dropped where the position before it holds its key (A's copy owns the row)
            if constexpr (!FRONT_ALL) look_front();
            if (has_pv && mp_same(mp_key<Row>(s_w + pv, ROWS), k)) continue;
            if (EMIT) { f = s_w[W_FI * ROWS + idx]; l = s_w[W_LA * ROWS + idx]; }
        } else {                                         // an A row: joins the next position's row where that holds its key
            const bool has = pos + 1 < nt || ahead;
            const u32 nx = pos + 1 < nt ? src(pos + 1) : la;
            const bool join = has && mp_same(mp_key<Row>(s_w + nx, ROWS), k);
            if (EMIT) { f = s_w[W_FI * ROWS + idx]; l = s_w[W_LA * ROWS + idx]; }
            if (join) mp_join(sum, f, l, s_w[W_SUM * ROWS + nx], EMIT ? s_w[W_FI * ROWS + nx] : 0, EMIT ? s_w[W_LA * ROWS + nx] : 0);
        }
        ++nrows;
        if constexpr (!EMIT && Row::HEADS) {             // a key head: no row in front of it has its key
            bool head = !(has_pv && s_w[Row::CMP0 * ROWS + pv] == k.k);
            if (pos == 0 && b_behind && kb_behind == k.k) head = false;
            nheads += head ? 1u : 0u;
        }
        if (sum >= (u64)p.min_count) {
            keptm |= 1u << i; ++nkept;
            if (EMIT) { rw[i][Row::CMP0] = k.k; if (Row::NCMP == 2) rw[i][Row::CMP1] = k.b; rw[i][W_SUM] = sum; rw[i][W_FI] = f; rw[i][W_LA] = l; }
        }
    }
    u32 tot_kept, tot_rows = 0, tot_heads = 0;
    u32 slot = block_excl_scan_256<u32>(nkept, s_scr, &tot_kept);       // (barriers inside: every lane has read the staged rows it needs)
    if (!EMIT) {
        (void)block_excl_scan_256<u32>(nrows, s_scr, &tot_rows);
        if (Row::HEADS) (void)block_excl_scan_256<u32>(nheads, s_scr, &tot_heads);
        if (tid == 0) { p.tile[0][blockIdx.x] = tot_kept; if (Row::HEADS) p.tile[1][blockIdx.x] = tot_heads; p.tile[Row::NTILE - 1][blockIdx.x] = tot_rows; }
        return;
    }

    // ---- the kept rows go back into LDS at their slots, and out 16 bytes per lane ----------------------------------------------
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        if (!(keptm & (1u << i))) continue;
#pragma unroll
        for (int w = 0; w < KEPT; ++w) s_w[(EMIT ? w : 0) * ROWS + slot] = rw[i][w];
        ++slot;
    }
    __syncthreads();
    mp_v2 *go = (mp_v2 *)(p.rows + p.tile[0][blockIdx.x] * WORDS);
    for (u32 q = tid; q < tot_kept * VECS; q += MP_THREADS) {
        const u32 r = q / (u32)VECS, w = (q - r * VECS) * 2;
        mp_v2 v;
        v.x = s_w[mp_lds_word<Row>(w) * ROWS + r];
        v.y = s_w[mp_lds_word<Row>(w + 1) * ROWS + r];
        go[q] = v;
    }
}

} // namespace hsk
#endif
