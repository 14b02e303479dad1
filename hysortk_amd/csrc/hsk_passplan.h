// hsk_passplan.h -- the digit plans of the radix sort (kernels: hsk_sort.h, hsk_expand.h; host: hsk_host_sort.h).
//
// A plan is the list of digits that the LSD passes take, least significant first: which word of the key, from which bit, how many bits.
// The key is the little-endian integer formed by words 0..NW-1; word w carries min(32, K-32w) bases in its top bits.
//
// Everything sized by a plan -- the PassDesc arrays in the kernel arguments, the [MAX_PASSES][256] histogram, base and ticket blocks, the
// pinned read-back, hist_kernel's and expand_kernel's dynamic LDS of 1 KB per pass -- holds MAX_PASSES digits, and every builder takes the
// capacity of the array it fills: a plan that does not fit is reported (-1) and not written.  MAX_PASSES is the longest plan a configuration
// that hsk_init() accepts can ask for: radix_bits = 4 over three full words (hsk_stage_sort with nw = 3), 3 * 16 = 48 digits.
//
// No HIP in here: the builders run on the CPU under the sanitizers (tests/passplan_test.cpp).
#pragma once
#include <algorithm>

namespace hsk {

constexpr int MAX_PASSES = 48;
constexpr int MIN_RADIX_BITS = 4, MAX_RADIX_BITS = 8;    // hsk_config::radix_bits (a digit has at most 256 values: the [256] rows above)
struct PassDesc { int word; int shift; int bits; };

// digits of the full-width plan: every used bit of every word, in digits of at most rb bits that do not cross a word
inline int pass_plan_length(int K, int nw, int rb)
{
    int np = 0;
    for (int w = 0; w < nw; ++w) np += (2 * std::min(32, K - 32 * w) + rb - 1) / rb;
    return np;
}

// Full-width plan: digits are taken from the least significant used bit of word 0 up; the last digit of a word is the narrower one.
// Returns the number of digits written, -1 (nothing written) for parameters outside the ABI's ranges or a plan longer than cap.
inline int make_pass_plan(int K, int nw, int rb, PassDesc *out, int cap)
{
    if (rb < MIN_RADIX_BITS || rb > MAX_RADIX_BITS || nw < 1 || K <= 32 * (nw - 1) || K > 32 * nw) return -1;
    if (pass_plan_length(K, nw, rb) > cap) return -1;
    int np = 0;
    for (int w = 0; w < nw; ++w) {
        const int nbases = std::min(32, K - 32 * w);
        int lo = 64 - 2 * nbases;
        while (lo < 64) { const int bits = std::min(rb, 64 - lo); out[np++] = PassDesc{w, lo, bits}; lo += bits; }
    }
    return np;
}

// Hybrid plan (one-word keys without payload): only the top 32 bits (16 bases) are ordered by global passes
// (digits at bit 32, 40, 48, 56, least significant first); binsort_kernel finishes the low bits inside each
// bin.  With 32 prefix bits two different k-mers of one task rarely share a bin, so nearly every bin is the
// copies of ONE k-mer and passes through untouched; 24 bits left 40 % of the records in multi-key bins whose
// in-LDS ordering (serial, LDS-latency bound) cost more than the fourth pass.
constexpr int HYBRID_SHIFT = 32;
inline int make_hybrid_plan(PassDesc *out, int cap, int prefix_bits = 64 - HYBRID_SHIFT, int word = 0)
{
    const int np = prefix_bits / 8;                     // LSD passes over the top prefix_bits bits (of the most significant word)
    if (prefix_bits < 8 || prefix_bits > 64 || prefix_bits % 8 || np > cap) return -1;
    for (int i = 0; i < np; ++i) out[i] = PassDesc{word, 64 - prefix_bits + 8 * i, 8};
    return np;
}

// bits of the 16-bit prefix that the most significant word holds (16: all of them)
inline int prefix_top_bits(int K, int nw) { return std::min(16, 2 * (K - 32 * (nw - 1))); }
// The 16-bit prefix of a key whose most significant word has only `top` < 16 significant bits: those, then the top 16 - top
// bits of the word below.  LSD passes, least significant digit first, no digit across a word boundary or wider than 8 bits.
inline int make_split_prefix_plan(PassDesc *out, int cap, int top, int nw)
{
    if (nw < 2 || top < 1 || top > 15) return -1;
    const int low = 16 - top;                            // bits taken from word nw - 2
    if ((low + 7) / 8 + (top + 7) / 8 > cap) return -1;
    int np = 0;
    for (int lo = 64 - low; lo < 64; ) { const int bits = std::min(8, 64 - lo); out[np++] = PassDesc{nw - 2, lo, bits}; lo += bits; }
    for (int lo = 64 - top; lo < 64; ) { const int bits = std::min(8, 64 - lo); out[np++] = PassDesc{nw - 1, lo, bits}; lo += bits; }
    return np;
}

} // namespace hsk
