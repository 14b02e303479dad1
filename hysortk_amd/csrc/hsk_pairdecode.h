// hsk_pairdecode.h -- the r-th unordered pair of an entry's occurrences (kernel: hsk_pairs.h).
//
// An entry with cnt occurrences has T(cnt) = cnt * (cnt - 1) / 2 pairs (i, j), i < j < cnt.  They are numbered column by column:
//     r = T(j) + i,   T(j) = j * (j - 1) / 2          (0,1) (0,2) (1,2) (0,3) (1,3) (2,3) ...
// so that consecutive r walk i (adjacent payload addresses) and the number of a pair does not depend on cnt.  The inverse is
//     j = floor((1 + sqrt(1 + 8 r)) / 2),   i = r - T(j).
// cnt <= 65535 (hsk_config::upper_freq): r < T(65535) = 2 147 385 345 < 2^31 and j <= 65534.  The root is taken in single precision --
// 1 + 8 r has up to 34 bits, a float 24: the estimate of j is off by less than one -- and put right by integer steps, which make the result
// exact whatever the estimate was.
//
// No HIP in here: the decode runs on the CPU under the sanitizers (tests/pairdecode_test.cpp).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define HSK_PD_FN __host__ __device__ inline
#else
#define HSK_PD_FN inline
#endif

namespace hsk {

constexpr uint32_t PAIR_MAX_CNT = 65535;                                  // hsk_config::upper_freq's bound
// pairs of an entry with cnt occurrences (cnt <= PAIR_MAX_CNT: fits 32 bits)
HSK_PD_FN uint32_t pair_count(uint32_t cnt) { return cnt < 2 ? 0u : (uint32_t)(((uint64_t)cnt * (cnt - 1)) >> 1); }

// r < pair_count(PAIR_MAX_CNT)  ->  *i < *j, r == T(*j) + *i
HSK_PD_FN void pair_decode(uint32_t r, uint32_t *i, uint32_t *j)
{
    const float x = (float)(8ull * (uint64_t)r + 1ull);
    uint32_t jj = (uint32_t)((1.0f + sqrtf(x)) * 0.5f);
    if (jj < 1) jj = 1;
    if (jj > PAIR_MAX_CNT) jj = PAIR_MAX_CNT;
    while ((jj * (jj - 1)) / 2 > r) --jj;                                   // (jj <= 65535: the products fit 32 bits)
    while ((jj * (jj + 1)) / 2 <= r) ++jj;
    *j = jj; *i = r - (jj * (jj - 1)) / 2;
}

} // namespace hsk
