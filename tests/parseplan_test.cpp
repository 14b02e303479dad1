// CPU exerciser of hysortk_amd/csrc/hsk_parseplan.h (the parse stage's tiling, slab byte ranges, record capacity and placement groups),
// built with -fsanitize=address,undefined by tests/test_parseplan.py.  The plan is held to the definition the kernels use (hsk_parse.h:
// scan_kernel's tile0 / tile_end, the placement kernels' walk over the slabs): the workgroups' tile ranges, slab by slab, cover every tile
// exactly once, and the slabs' byte ranges tile the packed buffer.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "../hysortk_amd/csrc/hsk_parseplan.h"

using namespace hsk;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// the tiles of slab sl end here (scan_kernel: tile_end)
static u64 tile_end(const ParseTiling &t, u32 sl)
{
    return (t.nslabs > 1 && ((u64)sl + 1) * t.slab_tiles < t.ntiles) ? ((u64)sl + 1) * t.slab_tiles : t.ntiles;
}

static void check_tiling(u64 bytes, u32 max_blocks, u32 want)
{
    const ParseTiling t = parse_tiling(bytes, max_blocks, want);
    const char *fmt = "bytes %llu max_blocks %u nslabs wanted %u";
#define ARGS (unsigned long long)bytes, max_blocks, want
    CHECK(t.ntiles == (bytes + 511) / 512, fmt, ARGS);
    CHECK(t.nblocks >= 1 && t.nblocks <= PARSE_MAX_BLOCKS && t.nblocks <= (max_blocks ? max_blocks : PARSE_MAX_BLOCKS) && t.nblocks <= t.ntiles, fmt, ARGS);
    CHECK(t.nslabs >= 1 && t.nslabs <= (want ? want : 1) && t.tiles_per_block >= 1, fmt, ARGS);
    if (t.nslabs > 1) CHECK(t.slab_tiles == (u64)t.tiles_per_block * t.nblocks, fmt, ARGS);
    // the ranges in launch order (slab, workgroup) ascend: every tile exactly once means each range starts where the last one ended
    u64 next = 0;
    for (u32 sl = 0; sl < t.nslabs; ++sl)
        for (u32 b = 0; b < t.nblocks; ++b) {
            const u64 lo = (u64)sl * t.slab_tiles + (u64)b * t.tiles_per_block, end = tile_end(t, sl);
            if (lo >= end) continue;                                   // (this workgroup has nothing in this slab)
            const u64 hi = lo + t.tiles_per_block < end ? lo + t.tiles_per_block : end;
            CHECK(lo == next, "%llu != %llu (slab %u workgroup %u); bytes %llu max_blocks %u nslabs wanted %u", (unsigned long long)lo, (unsigned long long)next, sl, b, ARGS);
            next = hi;
        }
    CHECK(next == t.ntiles, "%llu of %llu tiles covered; bytes %llu max_blocks %u nslabs wanted %u", (unsigned long long)next, (unsigned long long)t.ntiles, ARGS);
    // the slabs' bytes: [0, bytes) in order, heads inside their slabs, slab starts on tile boundaries
    u64 at = 0;
    for (u32 sl = 0; sl < t.nslabs; ++sl) {
        const SlabBytes s = slab_bytes(t, sl, bytes);
        CHECK(s.b0 == at && s.b0 <= s.bh && s.bh <= s.b1 && s.bh - s.b0 <= SLAB_HEAD && s.b0 % 512 == 0, "slab %u [%llu %llu %llu); bytes %llu max_blocks %u nslabs wanted %u",
              sl, (unsigned long long)s.b0, (unsigned long long)s.bh, (unsigned long long)s.b1, ARGS);
        if (t.nslabs > 1) CHECK(s.b0 == std::min<u64>((u64)sl * t.slab_tiles * 512, bytes) && s.b1 > s.b0, fmt, ARGS);      // (the tiles of the slab, and no empty slab)
        at = s.b1;
    }
    CHECK(at == bytes, fmt, ARGS);
#undef ARGS
}

int main()
{
    const u32 slabs[] = {1, 2, 3, 8, 16, 17};
    std::vector<u64> sizes = {1, 4, 511, 512, 513, 512 * 1023, 512 * 1024, 512 * 1024 + 1, (32u << 20) + 77, 2500000000ULL, 5ULL << 29, 20000000000ULL, 20ULL << 30};
    for (u32 s : slabs) for (int d = -1; d <= 1; ++d) sizes.push_back(512ULL * 1024 * s + d);
    for (u64 bytes : sizes) for (u32 mb : {1u, 7u, 1024u, 5000u, 0u}) for (u32 want : slabs) check_tiling(bytes, mb, want);
    const ParseTiling none = parse_tiling(0, 0, 16);
    CHECK(none.ntiles == 0 && none.nblocks == 0 && none.nslabs == 1, "empty input");

    static_assert(SLAB_HEAD >= (u64)(PARSE_WORDS - 128) * 4, "the scan of a slab reads PARSE_WORDS - 128 words of the next one");
    static_assert(PARSE_TILE == 2048 && PARSE_TILE / 4 == 512, "a tile is 512 bytes");

    std::vector<u32> caps;
    for (int W = 1; W <= 79; ++W) {
        const u32 cap = parse_rec_cap(W);
        const double need = 1.4 * (2.0 * 2048 / (W + 1) + 40);
        CHECK(cap >= SCAN_REC_CAP && cap <= 2048 && (cap & (cap - 1)) == 0, "W %d: %u", W, cap);
        if (need <= 2048) CHECK((double)cap >= need, "W %d: %u < %f", W, cap, need);
        caps.push_back(cap);
    }
    for (long long forced : {-5LL, 1LL, 100LL, 512LL, 513LL, 4096LL, 8192LL, 8193LL, 1LL << 40}) {
        const u32 cap = parse_rec_cap(17, forced);
        CHECK(cap >= 1 && cap <= PLACE_MAX_REC && (forced < 1 || forced > (long long)PLACE_MAX_REC || cap == (u32)forced), "forced %lld: %u", forced, cap);
        caps.push_back(cap);
    }
    for (PlaceKind kind : {PLACE_RECORDS, PLACE_ITEMS, PLACE_BYTES})
        for (u32 cap : caps) {
            const u32 g = place_group(kind, cap);
            CHECK(g >= 1 && g <= place_tiles(kind), "kind %d rec_cap %u: group %u", (int)kind, cap, g);
            if (cap <= place_rec(kind)) CHECK((u64)cap * g <= place_rec(kind), "kind %d rec_cap %u: group %u", (int)kind, cap, g);      // (a larger rec_cap never gets this kind: parse_place, scan_setup)
        }
    CHECK(place_rec(PLACE_RECORDS) == PLACE_MAX_REC && place_rec(PLACE_ITEMS) == PLACE_ITEM_REC && place_rec(PLACE_BYTES) == PLACE_BYTES_REC, "capacities");

    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK %zu sizes\n", sizes.size());
    return 0;
}
