// CPU exerciser of hysortk_amd/csrc/hsk_lanes.h (how combine_kernel<KT, true> hands the k-mers of a round's distinct items to its lanes), built
// with -fsanitize=address,undefined by tests/test_combine_lanes_plan.py.  The arithmetic is held to a brute-force enumeration: the list is
// built the way items_compact builds it (every one of 256 lanes owns four slots of the table, the block scan carries items and k-mers in one
// packed value), then every lane finds its piece's first entry, walks its piece as the kernel does, and every k-mer of the stream -- every
// (entry, position) -- must have been taken exactly once, in stream order, with the multiplicity of its entry.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../hysortk_amd/csrc/hsk_lanes.h"

using namespace hsk;

static int g_fail = 0;
static long g_lists = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// cnt[slot]: k-mers of the item in table slot `slot` (0: the slot is empty), mult[slot]: its multiplicity; slot = j * 256 + lane, as the kernel reads them
static void check_table(const std::vector<u32> &cnt, const std::vector<u32> &mult, const char *what)
{
    ++g_lists;
    const u32 slots = (u32)cnt.size(), per = (slots + LN_LANES - 1) / LN_LANES;
    // the compaction: a lane's scan value, the exclusive scan over the lanes, the entries written at the lane's offsets
    std::vector<u32> v(LN_LANES, 0);
    for (u32 lane = 0; lane < LN_LANES; ++lane)
        for (u32 j = 0; j < per; ++j) { const u32 s = j * LN_LANES + lane; if (s < slots && cnt[s]) v[lane] += lanes_scan_value(1u, cnt[s]); }
    std::vector<u32> ecnt, emult, im;
    u32 run = 0;
    std::vector<u32> ex(LN_LANES);
    for (u32 lane = 0; lane < LN_LANES; ++lane) { ex[lane] = run; run += v[lane]; }
    const u32 nd = lanes_scan_items(run), T = lanes_scan_kmers(run);
    ecnt.assign(nd, 0); emult.assign(nd, 0); im.assign(nd, 0);
    u64 want_T = 0; u32 want_nd = 0;
    for (u32 s = 0; s < slots; ++s) if (cnt[s]) { want_T += cnt[s]; ++want_nd; }
    CHECK(nd == want_nd && T == want_T, "%s: scan gives %u items %u k-mers, the table holds %u and %llu", what, nd, T, want_nd, (unsigned long long)want_T);
    if (nd != want_nd || T != want_T) return;
    for (u32 lane = 0; lane < LN_LANES; ++lane) {
        u32 o = lanes_scan_items(ex[lane]), p = lanes_scan_kmers(ex[lane]);
        for (u32 j = 0; j < per; ++j) {
            const u32 s = j * LN_LANES + lane;
            if (s >= slots || !cnt[s]) continue;
            CHECK(o < nd, "%s: entry %u of %u", what, o, nd);
            if (o >= nd) return;
            ecnt[o] = cnt[s]; emult[o] = mult[s]; im[o] = lanes_im(mult[s], p);
            CHECK(lanes_mult(im[o]) == mult[s] && lanes_off(im[o]) == p, "%s: im of entry %u", what, o);
            ++o; p += cnt[s];
        }
    }
    // the offsets are the exclusive sums of the entries' counts
    { u32 p = 0; for (u32 e = 0; e < nd; ++e) { CHECK(lanes_off(im[e]) == p, "%s: P_%u = %u, want %u", what, e, lanes_off(im[e]), p); p += ecnt[e]; } }
    // the pieces: every (entry, position) exactly once, in order
    const u32 n = lanes_per(T);
    CHECK((u64)n * LN_LANES >= T && (n == 0 || (u64)(n - 1) * LN_LANES < T), "%s: n %u for T %u", what, n, T);
    std::vector<std::vector<unsigned char>> seen(nd);
    for (u32 e = 0; e < nd; ++e) seen[e].assign(ecnt[e], 0);
    u64 taken = 0; u32 next = 0;
    for (u32 tid = 0; tid < LN_LANES; ++tid) {
        u32 pos = lanes_begin(tid, n);
        const u32 end = lanes_end(tid, n, T);
        if (pos >= end) continue;
        CHECK(pos == next, "%s: lane %u starts at %u, the lane before ended at %u", what, tid, pos, next);
        u32 e = lanes_find(im.data(), nd, pos);
        CHECK(e < nd && lanes_off(im[e]) <= pos && pos < lanes_off(im[e]) + ecnt[e], "%s: lane %u k-mer %u found in entry %u", what, tid, pos, e);
        if (e >= nd) return;
        u32 r = pos - lanes_off(im[e]), cnt_e = ecnt[e], m = lanes_mult(im[e]);
        while (pos < end) {
            CHECK(e < nd && r < ecnt[e] && m == emult[e], "%s: lane %u at k-mer %u: entry %u position %u", what, tid, pos, e, r);
            if (e >= nd || r >= ecnt[e]) return;
            CHECK(lanes_off(im[e]) + r == pos, "%s: lane %u: entry %u position %u is not k-mer %u", what, tid, e, r, pos);
            ++seen[e][r]; ++taken; ++pos;
            if (lanes_step(e, r, cnt_e) && pos < end) { CHECK(e < nd, "%s: lane %u walks past the list", what, tid); if (e >= nd) return; cnt_e = ecnt[e]; m = lanes_mult(im[e]); }
        }
        next = end;
    }
    CHECK(next == T && taken == T, "%s: %llu of %u k-mers taken, pieces end at %u", what, (unsigned long long)taken, T, next);
    for (u32 e = 0; e < nd; ++e) for (u32 r = 0; r < ecnt[e]; ++r) CHECK(seen[e][r] == 1, "%s: entry %u position %u taken %d times", what, e, r, (int)seen[e][r]);
}

int main()
{
    // every count vector of a few short lengths over a few counts (dense tables of that many slots; multiplicity 1 .. )
    const u32 vals[] = {1, 2, 15, 16};
    for (u32 len = 0; len <= 6; ++len) {
        u64 combos = 1; for (u32 i = 0; i < len; ++i) combos *= 4;
        for (u64 c = 0; c < combos; ++c) {
            std::vector<u32> cnt(len), mult(len);
            u64 x = c; for (u32 i = 0; i < len; ++i) { cnt[i] = vals[x & 3]; x >>= 2; mult[i] = 1 + i; }
            check_table(cnt, mult, "short");
        }
    }
    // every count 1 .. 16 alone and in pairs
    for (u32 a = 1; a <= 16; ++a) { check_table({a}, {8192}, "one"); for (u32 b = 1; b <= 16; ++b) check_table({a, b}, {1, 8192}, "two"); }
    // the edges of the packed values: a full table of full items with the largest multiplicity, of single k-mers, and totals around the lanes' number
    check_table(std::vector<u32>(1024, 16), std::vector<u32>(1024, 8192), "full 16");
    check_table(std::vector<u32>(1024, 1), std::vector<u32>(1024, 8192), "full 1");
    for (u32 nslot : {255u, 256u, 257u, 511u, 512u, 513u, 1023u, 1024u}) for (u32 c : {1u, 2u, 3u, 16u}) check_table(std::vector<u32>(nslot, c), std::vector<u32>(nslot, 3), "edge");
    // random tables: a share of the 1024 slots occupied, counts uniform, skewed to 16 (the benchmark: 23 % of the items) or all 1
    std::mt19937_64 rng(20240229);
    for (int it = 0; it < 3000; ++it) {
        const u32 slots = 1 + (u32)(rng() % 1024), fill = 1 + (u32)(rng() % 100), shape = (u32)(rng() % 3);
        std::vector<u32> cnt(slots, 0), mult(slots, 0);
        for (u32 s = 0; s < slots; ++s) {
            if (rng() % 100 >= fill) continue;
            cnt[s] = shape == 0 ? 1 + (u32)(rng() % 16) : shape == 1 ? (rng() % 4 == 0 ? 16u : 1 + (u32)(rng() % 16)) : 1u;
            mult[s] = 1 + (u32)(rng() % 8192);
        }
        check_table(cnt, mult, "random");
    }
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK %ld lists\n", g_lists);
    return 0;
}
