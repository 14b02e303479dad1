// hsk_diagbin.h -- the diagonal of a read-pair record and its bin (kernels: hsk_pairs.h, hsk_pairdiag.h; host: hsk_host_pairdiag.h).
//
// A record of hsk_result_pair_diagonals (include/hsk.h) has the key o << 63 | rid_a << 32 | rid_b and the value pos_a << 32 | pos_b.  Its
// diagonal number is
//     D = pos_a - pos_b + 2^32   (o = 0: seeds of a same-strand overlap keep the difference)
//     D = pos_a + pos_b          (o = 1: seeds of a reverse-complement overlap keep the sum)
// in 64-bit arithmetic, never negative and below 2^33; the bin is D / W (W = diag_bin, 1 .. 2^31, unsigned division).
//
// The sort word.  The records are sorted by (key, bin) as a two-word key, and the radix sort skips a digit only when one digit value holds
// all records.  The bin itself is a poor word for that: D = 2^32 +- small has four or five bytes that differ between records (0x00000001 00..
// above the bias, 0x00000000 FF.. below it).  The word that is sorted is therefore bin - bin_lo, with
//     bin_lo = (2^32 - maxpos) / W  (o = 0),    0  (o = 1),
// maxpos >= every position of the range: D >= 2^32 - maxpos, so the word is never negative, it keeps the order of the bins inside a key
// (bin_lo depends on o, which is part of the key), and it is below 2 maxpos / W + 2.  The reducer adds bin_lo back.
//
// The selection: of a key's bins the one with the larger support wins, and among equal supports the smaller bin (diag_better).
//
// No HIP in here: kernel, host and tests share one definition, and it runs on the CPU under the sanitizers (tests/diagbin_test.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define HSK_DB_FN __host__ __device__ inline
#else
#define HSK_DB_FN inline
#endif

namespace hsk {

constexpr uint64_t DIAG_BIAS = 1ULL << 32;               // added to pos_a - pos_b
constexpr uint64_t DIAG_MAX_WIDTH = 1ULL << 31;          // the largest diag_bin the call accepts

HSK_DB_FN uint64_t diag_number(uint64_t o, uint32_t pos_a, uint32_t pos_b)
{
    return o ? (uint64_t)pos_a + pos_b : DIAG_BIAS + pos_a - pos_b;
}
HSK_DB_FN uint64_t diag_bin_of(uint64_t o, uint32_t pos_a, uint32_t pos_b, uint64_t w) { return diag_number(o, pos_a, pos_b) / w; }

// the smallest bin a record of orientation o can have when no position of the range is above maxpos
HSK_DB_FN uint64_t diag_bin_lo(uint64_t o, uint32_t maxpos, uint64_t w) { return o ? 0 : (DIAG_BIAS - maxpos) / w; }
// what the sort sees in word 0 (pos_a, pos_b <= maxpos) and the way back
HSK_DB_FN uint64_t diag_sort_word(uint64_t o, uint32_t pos_a, uint32_t pos_b, uint32_t maxpos, uint64_t w)
{
    return diag_bin_of(o, pos_a, pos_b, w) - diag_bin_lo(o, maxpos, w);
}
HSK_DB_FN uint64_t diag_bin_of_sort_word(uint64_t o, uint64_t word, uint32_t maxpos, uint64_t w) { return word + diag_bin_lo(o, maxpos, w); }

// does bin a (support sa) beat bin b (support sb)?  larger support, then smaller bin
HSK_DB_FN bool diag_better(uint64_t sa, uint64_t bin_a, uint64_t sb, uint64_t bin_b) { return sa > sb || (sa == sb && bin_a < bin_b); }

} // namespace hsk
