// hsk_xdrop.h -- ungapped x-drop extension of a seed of two reads, 32 columns at a time (kernels: hsk_extend.h; host: hsk_host_extend.h;
// include/hsk.h: hsk_pair_diags_extend has the definition this file is held to, word for word).
//
// A COLUMN t pairs base pa + t of read A with a base of read B: B[pb + t] on the same strand (o = 0), the complement of B[pb + K - 1 - t]
// on opposite strands (o = 1); t = 0 is the seed's first base in A's forward direction.  The valid columns are [t_lo, t_hi) (xd_range).
// A WINDOW is 32 consecutive columns of one read as a 64-bit word, column t + c in bits 63 - 2c .. 62 - 2c (xd_window_a, xd_window_b): it is
// built from aligned 32-bit words of the packed stream (strand_word, hsk_strandbits.h: the buffer's last word byte by byte, no byte at or
// beyond `nbytes` is read), shifted to the base, and for B on the opposite strand reversed and complemented.  Columns of a window that
// are not valid hold whatever lies there (bytes of a neighbouring read, zeros outside the buffer): the caller says how many count.
// A WALK leaves the seed to the right (columns K, K + 1, ...) or to the left (-1, -2, ...); xd_walk_mask gives the mismatches of the 32
// walk positions from position c0 on, position c0 + i in bit 2i.  xd_step carries (s, best, the columns taken at best, the mismatches
// among them) across such a mask BY RUNS: since match > 0, s only rises inside a run of matching columns, so `best` needs looking at
// where a run ends, and since the drop best - s only grows at a mismatch, the drop test is needed there alone.
//
// No HIP in here: everything runs on the CPU under the sanitizers (tests/xdrop_test.cpp).
#pragma once
#include <cstdint>
#include "hsk_strandbits.h"

namespace hsk {

constexpr int XD_ROW_WORDS = 6;                          // { key, score, a_lo << 32 | a_hi, b_lo << 32 | b_hi, mismatches << 32 | ends, support }
constexpr int64_t XD_NONE = -(1LL << 62);                 // a `best` that nothing has reached yet (xd_step of a window on its own)
constexpr int64_t XD_NO_DROP = 1LL << 62;                 // an xdrop that never stops

HSK_SB_FN int xd_ctz64(uint64_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (int)__ffsll((unsigned long long)x) - 1;
#else
    return __builtin_ctzll(x);
#endif
}

// 64 bits of the stream from bit `bit` on (even), the first in the MSB; bits at or beyond 8 * nbytes read as zero
HSK_SB_FN uint64_t xd_stream64(const uint8_t *packed, uint64_t nbytes, uint64_t bit)
{
    const uint64_t w0 = bit >> 5;
    const uint32_t r = (uint32_t)(bit & 31);
    const uint32_t b0 = 4 * w0 < nbytes ? strand_word(packed, nbytes, w0) : 0u;
    const uint32_t b1 = 4 * (w0 + 1) < nbytes ? strand_word(packed, nbytes, w0 + 1) : 0u;
    const uint64_t hi = ((uint64_t)b0 << 32) | b1;
    if (!r) return hi;
    const uint32_t b2 = 4 * (w0 + 2) < nbytes ? strand_word(packed, nbytes, w0 + 2) : 0u;
    return (hi << r) | ((uint64_t)b2 >> (32 - r));
}

// bases i .. i + 31 of the read whose first base is bit `bit0` of the stream; i may be negative (the bases in front of the read: zeros)
HSK_SB_FN uint64_t xd_bases(const uint8_t *packed, uint64_t nbytes, uint64_t bit0, int64_t i)
{
    if (i >= 0) return xd_stream64(packed, nbytes, bit0 + 2 * (uint64_t)i);
    return i > -32 ? xd_stream64(packed, nbytes, bit0) >> (2 * (uint32_t)(-i)) : 0ULL;
}

// a seed of two reads and what the walks need to know about them
struct XdPair {
    uint64_t bit_a, bit_b;                               // first bit of read A / read B in the stream
    uint32_t pa, pb, la, lb;
    int32_t  k, o;
    int64_t  t_lo, t_hi;                                 // the valid columns
};

// the valid columns of a seed that fits its reads (pa + k <= la, pb + k <= lb): [t_lo, t_hi) holds 0 .. k - 1
HSK_SB_FN void xd_range(XdPair &p)
{
    const int64_t pa = p.pa, pb = p.pb, la = p.la, lb = p.lb, k = p.k;
    if (!p.o) {
        p.t_lo = -(pa < pb ? pa : pb);
        p.t_hi = la - pa < lb - pb ? la - pa : lb - pb;
    } else {
        p.t_lo = -pa > pb + k - lb ? -pa : pb + k - lb;
        p.t_hi = la - pa < pb + k ? la - pa : pb + k;
    }
}

// columns t .. t + 31 of read A, and of read B in A's direction
HSK_SB_FN uint64_t xd_window_a(const uint8_t *packed, uint64_t nbytes, const XdPair &p, int64_t t)
{
    return xd_bases(packed, nbytes, p.bit_a, (int64_t)p.pa + t);
}
HSK_SB_FN uint64_t xd_window_b(const uint8_t *packed, uint64_t nbytes, const XdPair &p, int64_t t)
{
    if (!p.o) return xd_bases(packed, nbytes, p.bit_b, (int64_t)p.pb + t);
    // column t + c is the complement of B[pb + k - 1 - t - c]: the forward bases from pb + k - 32 - t on, in reverse order
    return ~strand_rev2(xd_bases(packed, nbytes, p.bit_b, (int64_t)p.pb + p.k - 32 - t));
}

// the columns of two windows that differ: column c in bit 62 - 2c
HSK_SB_FN uint64_t xd_mismatch(uint64_t wa, uint64_t wb)
{
    const uint64_t x = wa ^ wb;
    return (x | (x >> 1)) & 0x5555555555555555ULL;
}

// the low n of 32 walk positions (n <= 32)
HSK_SB_FN uint64_t xd_low(uint64_t m, uint32_t n) { return n >= 32 ? m : m & ((1ULL << (2 * n)) - 1); }

// The mismatches of walk positions c0 .. c0 + n - 1 (n <= 32, all valid) of the right walk (position c is column k + c) or the left walk
// (position c is column -1 - c): position c0 + i in bit 2i, the bits from 2n on zero.
HSK_SB_FN uint64_t xd_walk_mask(const uint8_t *packed, uint64_t nbytes, const XdPair &p, bool right, uint64_t c0, uint32_t n)
{
    const int64_t t = right ? (int64_t)p.k + (int64_t)c0 : -(int64_t)c0 - 32;      // the window's first column
    const uint64_t m = xd_mismatch(xd_window_a(packed, nbytes, p, t), xd_window_b(packed, nbytes, p, t));
    // right: column t + i sits in bit 62 - 2i, and reversing the bases brings it to bit 2i; left: position c0 + i is column t + 31 - i, bit 2i as it is
    return xd_low(right ? strand_rev2(m) : m, n);
}

// the seed's own columns 0 .. k - 1: true if they all match
HSK_SB_FN bool xd_seed_matches(const uint8_t *packed, uint64_t nbytes, const XdPair &p)
{
    uint64_t bad = 0;
    for (int32_t t = 0; t < p.k; t += 32) {
        const uint32_t n = p.k - t < 32 ? (uint32_t)(p.k - t) : 32u;
        const uint64_t m = xd_mismatch(xd_window_a(packed, nbytes, p, t), xd_window_b(packed, nbytes, p, t));
        bad |= xd_low(strand_rev2(m), n);
    }
    return bad == 0;
}

// one side of the extension
struct XdSide {
    int64_t  s = 0, best = 0;
    uint32_t len = 0;                                    // walk positions taken when `best` was reached
    uint32_t mm = 0;                                     // mismatches among them
    uint32_t seen = 0;                                   // mismatches among all positions walked
};

// Walk positions pos0 .. pos0 + n - 1, whose mismatches are m (xd_walk_mask).  Returns true if the walk stops inside them (best - s > xdrop
// behind a mismatch); the positions behind the stop are not looked at.  match > 0, mismatch >= 0.
HSK_SB_FN bool xd_step(XdSide &st, uint64_t m, uint32_t n, uint32_t pos0, int64_t match, int64_t mismatch, int64_t xdrop)
{
    uint32_t c = 0;
    while (c < n) {
        const uint32_t z = m ? (uint32_t)xd_ctz64(m) >> 1 : n;      // the next mismatch; (m has no bit at or behind 2n)
        if (z > c) {
            st.s += (int64_t)(z - c) * match;
            c = z;
            if (st.s > st.best) { st.best = st.s; st.len = pos0 + c; st.mm = st.seen; }
        }
        if (c < n) {
            st.s -= mismatch; ++st.seen; ++c;
            m &= m - 1;
            if (st.best - st.s > xdrop) return true;
        }
    }
    return false;
}

// The overlap's row from the two sides (left.len columns in front of the seed, right.len behind it)
HSK_SB_FN void xd_row(const XdPair &p, uint64_t key, uint64_t support, int64_t match, const XdSide &left, const XdSide &right, uint64_t (&row)[XD_ROW_WORDS])
{
    const int64_t begin = -(int64_t)left.len, end = (int64_t)p.k + right.len;
    const uint64_t a_lo = (uint64_t)((int64_t)p.pa + begin), a_hi = (uint64_t)((int64_t)p.pa + end);
    const uint64_t b_lo = (uint64_t)(p.o ? (int64_t)p.pb + p.k - end : (int64_t)p.pb + begin);
    const uint64_t b_hi = (uint64_t)(p.o ? (int64_t)p.pb + p.k - begin : (int64_t)p.pb + end);
    const uint64_t ends = (a_lo == 0 ? 1u : 0u) | (a_hi == p.la ? 2u : 0u) | (b_lo == 0 ? 4u : 0u) | (b_hi == p.lb ? 8u : 0u);
    row[0] = key;
    row[1] = (uint64_t)((int64_t)p.k * match + right.best + left.best);
    row[2] = a_lo << 32 | a_hi;
    row[3] = b_lo << 32 | b_hi;
    row[4] = (uint64_t)(left.mm + right.mm) << 32 | ends;
    row[5] = support;
}

// One side, a window at a time (what a lane of the lane path does, and the CPU): `cols` walk positions are valid.
HSK_SB_FN XdSide xd_walk(const uint8_t *packed, uint64_t nbytes, const XdPair &p, bool right, int64_t match, int64_t mismatch, int64_t xdrop)
{
    const uint64_t cols = right ? (uint64_t)(p.t_hi - p.k) : (uint64_t)(-p.t_lo);
    XdSide st;
    for (uint64_t c0 = 0; c0 < cols; c0 += 32) {
        const uint32_t n = cols - c0 < 32 ? (uint32_t)(cols - c0) : 32u;
        if (xd_step(st, xd_walk_mask(packed, nbytes, p, right, c0, n), n, (uint32_t)c0, match, mismatch, xdrop)) break;
    }
    return st;
}

} // namespace hsk
