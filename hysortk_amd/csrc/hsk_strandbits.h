// hsk_strandbits.h -- the strand of one k-mer occurrence: the K bases of a read at a position, against the canonical k-mer of the entry
// that owns the occurrence (kernel: hsk_strand.h; include/hsk.h: hsk_result_strands).
//
// The packed reads are a big-endian stream of 2-bit bases: base i of the buffer's bit stream sits in byte i / 4 at shift 6 - 2 (i % 4),
// and every read starts on a byte boundary.  strand_load puts the K bases that start at bit `bitpos` of the stream into the Mer<NW>
// layout (base i in word i / 32 at shift 2 (31 - i % 32), the bits behind base K - 1 zero).  It reads the stream as aligned 32-bit
// words -- 2 NW + 1 of them hold K bases at every byte phase -- and takes the buffer's last, partial word byte by byte: no byte at or
// beyond `nbytes` is read, and no word that holds none of the K bases.  strand_decide compares the word with the entry's k-mer first and
// with its reverse complement second: a k-mer that is its own reverse complement (even K only) is forward.
//
// No HIP in here: both run on the CPU under the sanitizers (tests/strandbits_test.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define HSK_SB_FN __host__ __device__ inline
#else
#define HSK_SB_FN inline
#endif

namespace hsk {

enum { STRAND_FORWARD = 0, STRAND_REVERSE = 1, STRAND_PALINDROME = 2, STRAND_MISMATCH = 3 };      // (a palindrome is forward: bit 0)

// the 32 bases of a word in reverse order (base i <-> base 31 - i)
HSK_SB_FN uint64_t strand_rev2(uint64_t x)
{
    x = ((x >> 2) & 0x3333333333333333ULL) | ((x & 0x3333333333333333ULL) << 2);
    x = ((x >> 4) & 0x0f0f0f0f0f0f0f0fULL) | ((x & 0x0f0f0f0f0f0f0f0fULL) << 4);
    x = ((x >> 8) & 0x00ff00ff00ff00ffULL) | ((x & 0x00ff00ff00ff00ffULL) << 8);
    x = ((x >> 16) & 0x0000ffff0000ffffULL) | ((x & 0x0000ffff0000ffffULL) << 16);
    return (x >> 32) | (x << 32);
}

// reverse complement of a K-mer of NW words (the layout and the result of twin<NW>, hsk_device.h)
template <int NW>
HSK_SB_FN void strand_twin(const uint64_t (&f)[NW], int k, uint64_t (&t)[NW])
{
    for (int l = 0; l < NW; ++l) t[NW - 1 - l] = ~strand_rev2(f[l]);
    const int sh = NW * 64 - 2 * k;                      // unused low bits of the last word; 0 < sh < 64 (K % 32 != 0)
    if (sh) {
        for (int i = 0; i < NW; ++i) {
            const uint64_t nxt = i + 1 < NW ? t[i + 1] : 0;
            t[i] = (t[i] << sh) | (nxt >> (64 - sh));
        }
    }
}

// aligned 32-bit word w of the stream, first byte in the top bits; `packed` is 4-byte aligned, 4 w < nbytes
HSK_SB_FN uint32_t strand_word(const uint8_t *packed, uint64_t nbytes, uint64_t w)
{
    const uint64_t b = 4 * w;
    if (b + 4 <= nbytes) {
        const uint32_t v = *reinterpret_cast<const uint32_t *>(packed + b);
        return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24);
    }
    uint32_t v = 0;                                      // the buffer's last word: the bytes it has
    for (int j = 0; j < 4; ++j) if (b + j < nbytes) v |= (uint32_t)packed[b + j] << (24 - 8 * j);
    return v;
}

// The k bases from bit `bitpos` of the stream on (bitpos even; NW = (k + 31) / 32, k % 32 != 0).  The caller has made sure that the last of
// them lies inside the buffer: (bitpos + 2 k - 1) / 8 < nbytes.
template <int NW>
HSK_SB_FN void strand_load(const uint8_t *packed, uint64_t nbytes, uint64_t bitpos, int k, uint64_t (&f)[NW])
{
    constexpr int NWORD = 2 * NW + 1;
    const uint64_t w0 = bitpos >> 5, wl = (bitpos + 2 * (uint64_t)k - 1) >> 5;      // first and last word that hold a base
    const uint32_t r = (uint32_t)(bitpos & 31);
    uint32_t be[NWORD];
    for (int i = 0; i < NWORD; ++i) be[i] = w0 + i <= wl ? strand_word(packed, nbytes, w0 + i) : 0u;
    for (int j = 0; j < NW; ++j) {
        const uint64_t hi = ((uint64_t)be[2 * j] << 32) | be[2 * j + 1];
        f[j] = r ? (hi << r) | ((uint64_t)be[2 * j + 2] >> (32 - r)) : hi;
    }
    f[NW - 1] &= ~0ULL << (NW * 64 - 2 * k);
}

// f: the read's bases (strand_load); e: the entry's k-mer words
template <int NW>
HSK_SB_FN int strand_decide(const uint64_t (&f)[NW], const uint64_t *e, int k)
{
    uint64_t t[NW];
    strand_twin<NW>(f, k, t);
    bool fwd = true, rev = true;
    for (int i = 0; i < NW; ++i) { fwd = fwd && f[i] == e[i]; rev = rev && t[i] == e[i]; }
    return fwd ? (rev ? STRAND_PALINDROME : STRAND_FORWARD) : (rev ? STRAND_REVERSE : STRAND_MISMATCH);
}

} // namespace hsk
