// hsk_lanes.h -- how combine_kernel<KT, true> (hsk_combine.h, 3a) hands the k-mers of a round's distinct items to its lanes.
//
// The round's distinct items lie as a dense list of nd <= LN_MAX_ITEMS entries; entry e carries cnt_e k-mers (1 .. 16).  Back to back they are one
// STREAM of T = sum cnt_e k-mers, and entry e knows the stream offset of its first one, P_e (exclusive sum), beside its multiplicity:
//     im_e = multiplicity | P_e << LN_MULT_BITS            (lanes_im; a unit has at most 8192 items, a round at most 16384 k-mers)
// The compaction's block scan carries items and k-mers in one value (lanes_scan_value).  Lane `tid` of LN_LANES takes the k-mers
//     [tid * n, (tid + 1) * n) cut at T,   n = ceil(T / LN_LANES)                                   (lanes_per, lanes_begin)
// finds the entry of its first one by a binary search over P_e (lanes_find: ten reads) and walks forward: inside an item to the next
// position, behind an item's last k-mer to position 0 of the next entry (lanes_step).
//
// No HIP in here: everything runs on the CPU under the sanitizers (tests/combine_lanes_test.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HSK_LANES_FN __host__ __device__ __forceinline__
#else
#define HSK_LANES_FN inline
#endif

namespace hsk {

typedef uint64_t u64;
typedef uint32_t u32;

constexpr u32 LN_LANES = 256;                         // lanes of the workgroup (CB_THREADS)
constexpr u32 LN_MAX_ITEMS = 1024;                    // entries of a round at most (the item table's slots)
constexpr u32 LN_MAX_CNT = 16;                        // k-mers of an item at most
constexpr u32 LN_ITEM_BITS = 11;                      // the scan value: items below, k-mers above
constexpr u32 LN_MULT_BITS = 14;                      // im: the multiplicity below, P_e above
static_assert(LN_MAX_ITEMS < (1u << LN_ITEM_BITS) && (u64)LN_MAX_ITEMS * LN_MAX_CNT < (1ull << (32 - LN_ITEM_BITS)), "items and k-mers of a round in one 32-bit scan value");
static_assert((u64)LN_MAX_ITEMS * LN_MAX_CNT <= (1ull << (32 - LN_MULT_BITS)), "P_e beside the multiplicity");

HSK_LANES_FN u32 lanes_scan_value(u32 items, u32 kmers) { return items | (kmers << LN_ITEM_BITS); }
HSK_LANES_FN u32 lanes_scan_items(u32 v) { return v & ((1u << LN_ITEM_BITS) - 1u); }
HSK_LANES_FN u32 lanes_scan_kmers(u32 v) { return v >> LN_ITEM_BITS; }

HSK_LANES_FN u32 lanes_im(u32 mult, u32 p) { return mult | (p << LN_MULT_BITS); }      // mult < 2^LN_MULT_BITS
HSK_LANES_FN u32 lanes_mult(u32 im) { return im & ((1u << LN_MULT_BITS) - 1u); }
HSK_LANES_FN u32 lanes_off(u32 im) { return im >> LN_MULT_BITS; }

HSK_LANES_FN u32 lanes_per(u32 T) { return (T + LN_LANES - 1u) / LN_LANES; }
// the piece of lane tid: [begin, end); begin >= end: the lane takes nothing
HSK_LANES_FN u32 lanes_begin(u32 tid, u32 n) { return tid * n; }
HSK_LANES_FN u32 lanes_end(u32 tid, u32 n, u32 T) { const u32 e = tid * n + n; return e < T ? e : T; }

// the entry that holds k-mer s of the stream (s < T, nd >= 1): the last e with P_e <= s.  im: the list's im words (P_0 = 0, P ascending strictly)
HSK_LANES_FN u32 lanes_find(const u32 *im, u32 nd, u32 s)
{
    u32 lo = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (u32 step = LN_MAX_ITEMS / 2; step; step >>= 1) {
        const u32 mid = lo + step;
        if (mid < nd && lanes_off(im[mid]) <= s) lo = mid;
    }
    return lo;
}

// one k-mer on: from position r of entry e (cnt k-mers) to the next k-mer of the stream.  True: entry e is done, the next k-mer is position 0 of e + 1.
HSK_LANES_FN bool lanes_step(u32 &e, u32 &r, u32 cnt)
{
    if (++r < cnt) return false;
    ++e; r = 0;
    return true;
}

} // namespace hsk
