// hsk_fmin.h -- the minimum of 64-bit hashes as ONE double-precision instruction (scan_kernel's window minima, hsk_parse.h).
//
// An IEEE double whose sign bit is clear and which is no NaN orders exactly as its bit pattern does as an unsigned integer, denormal
// patterns (top word below 0x00100000) included as long as nothing flushes them: v_min_f64 is then a 64-bit unsigned minimum at a third of
// the issue cycles of v_cmp_lt_u64 + 2 v_cndmask_b32.  Half of all hashes are outside that range (sign bit, infinity, NaN), so:
//   * fmin_clamp() caps a value's TOP WORD at FMIN_SENTINEL, the top word of the largest finite doubles (one v_min_u32); the low word stays.
//     A value below the sentinel class is unchanged; a value inside it keeps only "I am at least 0x7FEFFFFF'00000000";
//   * fmin_u64() of clamped values is exact whenever the result's top word is below the sentinel: then some operand was below the class, every
//     operand of the class is larger than it under both orders, and the operands below the class are compared as they are;
//   * a result whose top word IS the sentinel says that every operand was in the class: which of them is the least is lost (their top
//     words are gone), fmin_exact() is false and the caller repeats the minimum with integer compares on the unclamped values.
// No HIP in here beyond the one instruction: the rest runs on the CPU under the sanitizers (tests/fmin_test.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define HSK_FMIN_HD __host__ __device__ __forceinline__
#else
#define HSK_FMIN_HD inline
#endif

namespace hsk {

constexpr uint32_t FMIN_SENTINEL = 0x7FEFFFFFu;       // top word of the largest finite doubles: 0x7FF00000 and up are infinity, NaN and the negative half

HSK_FMIN_HD uint64_t fmin_clamp(uint64_t v)
{
    const uint32_t hi = (uint32_t)(v >> 32);
    return ((uint64_t)(hi < FMIN_SENTINEL ? hi : FMIN_SENTINEL) << 32) | (uint32_t)v;
}

// minimum of two clamped values (top words <= FMIN_SENTINEL)
HSK_FMIN_HD uint64_t fmin_u64(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    // the instruction itself, not fmin(): the compiler would quiet possible signalling NaNs first (a v_max_f64 per operand).  FP64 denormals
    // are never flushed by a HIP kernel's mode register (FP_DENORM of doubles: in and out allowed) -- tests/test_gpu_scan_minima.py holds it to that
    double d;
    asm("v_min_f64 %0, %1, %2" : "=v"(d) : "v"(__longlong_as_double((long long)a)), "v"(__longlong_as_double((long long)b)));
    return (uint64_t)__double_as_longlong(d);
#else
    double x, y;
    memcpy(&x, &a, 8); memcpy(&y, &b, 8);
    const double m = y < x ? y : x;
    uint64_t r;
    memcpy(&r, &m, 8);
    return r;
#endif
}

HSK_FMIN_HD bool fmin_exact(uint64_t m) { return (uint32_t)(m >> 32) < FMIN_SENTINEL; }

}  // namespace hsk
