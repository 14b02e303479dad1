// CPU exerciser of the address arithmetic of hysortk_amd/csrc/hsk_chunks.h (chunk_deltas, chunk_slot), built with -fsanitize=address,undefined
// by tests/test_chunks.py.  A reservation of c records that starts off0 slots into a chunk touches up to XS_SPAN physical chunks ph[]; its
// records are slots [st, st + c) of the flush's sorted order.  The definition every writer of the chunk store relies on:
//     slot i  ->  record (ph[v] - 1) * CHUNK + (off0 + i - st) % CHUNK,   v = (off0 + i - st) / CHUNK            (mod 2^32)
// held exhaustively for a small chunk and on seeded draws for the chunk sizes of the kernels.
#include <cstdint>
#include <cstdio>

#include "../hysortk_amd/csrc/hsk_chunks.h"

using hsk::u32;
using hsk::u64;
using hsk::XS_SPAN;

static int g_fail = 0;
static long long g_checked = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static u64 g_rng = 0x243f6a8885a308d3ULL;
static u64 rnd()
{
    g_rng += 0x9e3779b97f4a7c15ULL;
    u64 x = g_rng;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL; x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
    return x ^ (x >> 31);
}

// one reservation: the chunks it does not touch have no physical chunk (0), as chunk_resolve leaves them
template <int CHUNK>
static void check_reservation(u32 st, u32 off0, u32 c, const u32 (&all)[XS_SPAN])
{
    const u32 nv = (off0 + c - 1) / CHUNK + 1;
    CHECK(nv <= (u32)XS_SPAN, "CHUNK=%d off0=%u c=%u: %u chunks", CHUNK, off0, c, nv);
    if (nv > (u32)XS_SPAN) return;
    u32 ph[XS_SPAN];
    for (int q = 0; q < XS_SPAN; ++q) ph[q] = (u32)q < nv ? all[q] : 0u;
    const hsk::uint4 dl = hsk::chunk_deltas<CHUNK>(st, off0, ph);
    for (u32 i = st; i < st + c; ++i) {
        const u32 r = off0 + i - st, v = r / CHUNK;
        const u32 want = (ph[v] - 1u) * (u32)CHUNK + r % CHUNK;
        const u32 got = hsk::chunk_slot<CHUNK>(dl, i);
        ++g_checked;
        CHECK(got == want, "CHUNK=%d st=%u off0=%u c=%u ph={%u,%u,%u} slot %u: record %u, want %u", CHUNK, st, off0, c, ph[0], ph[1], ph[2], i, got, want);
    }
}

template <int CHUNK>
static void sampled(int draws)
{
    const u32 sts[4] = {0, 1, 4095, 8191};
    for (int n = 0; n < draws; ++n) {
        const u32 off0 = (u32)(rnd() % CHUNK), c = 1u + (u32)(rnd() % ((XS_SPAN - 1) * CHUNK));
        u32 ph[XS_SPAN];
        for (int q = 0; q < XS_SPAN; ++q) ph[q] = 1u + (u32)(rnd() % (1u << 20));
        if (n % 4 == 0) ph[(n / 4) % XS_SPAN] = 1u << 20;                  // (ph - 1) * 4096 is just below 2^32, ph * 4096 wraps
        check_reservation<CHUNK>(sts[n % 4], n % 7 == 0 ? 0u : (n % 7 == 1 ? (u32)CHUNK - 1u : off0), n % 5 == 0 ? (u32)(XS_SPAN - 1) * CHUNK : c, ph);
    }
}

int main()
{
    // physical chunks in no order, equal to one another, the first and the last a store can have, and numbers whose products with the chunk
    // size wrap 32 bits (2^20 chunks of 4096 records; with 16 records per chunk: 2^28 and beyond)
    const u32 phs[][XS_SPAN] = {
        {1, 2, 3}, {3, 2, 1}, {7, 1, 4}, {1u << 20, 5, (1u << 20) - 1}, {9, 1u << 20, 2}, {(1u << 20) - 2, 1, 1u << 20},
        {1u << 28, 3, (1u << 28) + 1}, {0xFFFFFFFFu, 1u << 31, 6}, {12, 0xFFFFFFF0u, (1u << 28) - 1},
    };
    constexpr int CH = 16;
    const u32 sts[4] = {0, 1, 4095, 8191};
    for (const auto &ph : phs)
        for (u32 st : sts)
            for (u32 off0 = 0; off0 < (u32)CH; ++off0)
                for (u32 c = 1; c <= (u32)(XS_SPAN - 1) * CH; ++c) check_reservation<CH>(st, off0, c, ph);
    sampled<4096>(300);
    sampled<2048>(300);

    if (g_fail) { std::printf("FAILED: %d checks\n", g_fail); return 1; }
    std::printf("OK %lld slots: every reservation of a 16-record chunk, 300 draws each for chunks of 4096 and 2048 records\n", g_checked);
    return 0;
}
