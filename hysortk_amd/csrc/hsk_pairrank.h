// hsk_pairrank.h -- the arithmetic of pair_finish_kernel (hsk_pairfinish.h): how the {k-mer, count} pairs of one prefix bin become the bin's
// sorted, merged, filtered entries without a hash table.
//
// A bin holds n <= PF_CAP pairs; nearly all keys are distinct, a few occur twice or more (partial pairs of one k-mer).
//   1. bucket     a pair's bucket is the PF_LOG2BKT key bits right below the bin prefix (pf_bucket); the pair takes the bucket's next ARRIVAL
//                 index (an atomic in the kernel), an exclusive scan of the bucket sizes gives every bucket's start, and the pair lies at
//                 start + arrival of a bucket-major array.
//   2. rank       a pair walks its bucket [b0, b1) once (pf_see per element, itself included): keys smaller than its own, equal keys that
//                 arrived before it, and the sum of the counts of all equal keys (32 bits, wrapping like the table's counter).  Its rank is
//                 b0 + smaller + equal-before (pf_rank): equal keys are ordered by arrival, so the ranks of a bin are a permutation of 0 .. n-1.
//   3. merge      the element of a run of equal keys that arrived first is the run's HEAD (pf_head) and carries the sum; the others are dropped.
//   4. filter     a head is kept when the SUM lies in [lower, upper] (pf_keep) -- never a partial count.
//   5. slot       kept heads set bit `rank` of a mask of PF_WORDS 32-bit words (pf_word, pf_bit); the entry's place in the bin's output is the
//                 number of set bits below its own: the exclusive sum of the words' popcounts plus the bits below inside its word (pf_slot).
//                 The number of entries is the sum of all popcounts.
//
// No HIP in here: everything runs on the CPU under the sanitizers (tests/pairfinish_test.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HSK_PAIRRANK_FN __host__ __device__ __forceinline__
#else
#define HSK_PAIRRANK_FN inline
#endif

namespace hsk {

typedef uint64_t u64;
typedef uint32_t u32;

constexpr u32 PF_LANES = 256;                         // lanes of the workgroup (AG_THREADS)
constexpr u32 PF_PER = 8;                             // pairs a lane holds at most
constexpr u32 PF_CAP = PF_LANES * PF_PER;             // pairs of a bin at most (beyond: the bin is listed for the table ladder)
constexpr int PF_LOG2BKT = 9;
constexpr u32 PF_NBKT = 1u << PF_LOG2BKT;             // buckets of the counting sort (a typical bin: ~480 pairs, one per bucket)
constexpr u32 PF_WORDS = PF_CAP / 32;                 // words of the kept-heads mask: one per lane of a wave
static_assert(PF_WORDS == 64, "a wave scans the mask's words, one per lane");
static_assert(PF_NBKT == 64 * 8, "a wave scans the buckets, eight per lane");

// shift: the bin is key >> shift (AggArgs::shift, 48 .. 55); the prefix bits are equal inside a bin and masked off
HSK_PAIRRANK_FN u32 pf_bucket(u64 key, int shift) { return (u32)(key >> (shift - PF_LOG2BKT)) & (PF_NBKT - 1u); }

struct PfRank { u32 less, eq_before, sum; };          // what a pair has seen of its bucket so far (start: all zero)
// one element of the pair's own bucket (the pair itself is one of them: it adds its own count to the sum)
HSK_PAIRRANK_FN void pf_see(PfRank &r, u64 mine, u32 my_arrival, u64 other, u32 other_arrival, u32 other_cnt)
{
    const bool eq = other == mine;
    r.less += other < mine ? 1u : 0u;
    r.eq_before += (eq && other_arrival < my_arrival) ? 1u : 0u;
    r.sum += eq ? other_cnt : 0u;
}
HSK_PAIRRANK_FN u32 pf_rank(u32 b0, const PfRank &r) { return b0 + r.less + r.eq_before; }
HSK_PAIRRANK_FN bool pf_head(const PfRank &r) { return r.eq_before == 0; }
HSK_PAIRRANK_FN bool pf_keep(const PfRank &r, u32 lower, u32 upper) { return pf_head(r) && r.sum >= lower && r.sum <= upper; }

HSK_PAIRRANK_FN u32 pf_word(u32 rank) { return rank >> 5; }
HSK_PAIRRANK_FN u32 pf_bit(u32 rank) { return 1u << (rank & 31u); }
// words_before: kept heads in the mask words below pf_word(rank); word: the mask word of the rank
HSK_PAIRRANK_FN u32 pf_slot(u32 words_before, u32 word, u32 rank) { return words_before + (u32)__builtin_popcount(word & (pf_bit(rank) - 1u)); }

} // namespace hsk
