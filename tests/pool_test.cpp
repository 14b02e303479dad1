// CPU exerciser of hysortk_amd/csrc/hsk_pool.h (the device pool's segment logic against malloc): random allocate / write / check / release
// sequences; every live block keeps its pattern, live blocks never overlap, bytes_live + bytes_cached == bytes mapped, trim returns all.
// The same with red zones on (pool_redzone: quarantine, periodic check + flush), the red zones' own cases (redzone_cases) and a failed
// call's rollback to its mark (rollback_cases).
#include "../hysortk_amd/csrc/hsk_pool.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
static size_t g_mapped = 0, g_limit = (size_t)1 << 30;
static std::map<void *, size_t> g_regions;
static int be_malloc(void **p, size_t n) { if (g_mapped + n > g_limit) { *p = nullptr; return 1; } *p = std::aligned_alloc(256, n); if (!*p) return 1; g_regions[*p] = n; g_mapped += n; return 0; }
static int be_free(void *p) { g_mapped -= g_regions[p]; g_regions.erase(p); std::free(p); return 0; }
// the red zones' backend on the host: memset and a scan (the device's is a memset on the stream and one kernel)
static int g_fills = 0;
static void be_fill(void *, void *p, size_t n) { std::memset(p, DevPool::RZ_BYTE, n); ++g_fills; }
static int be_check(void *, const DevPool::Zone *z, size_t n, size_t *bz, size_t *bo)
{
    for (size_t i = 0; i < n; ++i)
        for (size_t q = 0; q < z[i].bytes; ++q) if ((unsigned char)z[i].p[q] != DevPool::RZ_BYTE) { *bz = i; *bo = q; return 1; }
    return 0;
}
static void with_redzone(DevPool &pool, size_t rz) { pool.redzone = rz; pool.be_fill = be_fill; pool.be_check = be_check; }
static size_t live_blocks(const DevPool &pool) { size_t n = 0; for (auto &kv : pool.segs) n += !kv.second.free && !kv.second.quar; return n; }
#define EXPECT(cond, ...) do { if (!(cond)) { std::printf("FAIL " __VA_ARGS__); std::printf(" (line %d)\n", __LINE__); return 1; } } while (0)

static int redzone_cases()
{
    char msg[320];
    {   // a write one byte past a block of 16-byte multiple size: reported with the block's allocation site and offset; a write inside is not
        DevPool pool; pool.be_malloc = be_malloc; pool.be_free = be_free; with_redzone(pool, 64);
        g_fills = 0;
        unsigned char *other = (unsigned char *)pool.alloc(8192);
        const int line_a = __LINE__; unsigned char *a = (unsigned char *)pool.alloc(4096);
        EXPECT(a && other && g_fills == 2, "alloc");
        std::memset(a, 0, 4096); std::memset(other, 0xff, 8192);
        EXPECT(pool.check(msg, sizeof msg) == 0 && msg[0] == 0, "a write inside the requested size was reported: %s", msg);
        a[4096] = 0;
        EXPECT(pool.check(msg, sizeof msg) == 1, "a write one byte past the block was not reported");
        char want[64]; std::snprintf(want, sizeof want, "pool_test.cpp:%d ", line_a);
        EXPECT(std::strstr(msg, want) && std::strstr(msg, "byte 4096 ") && std::strstr(msg, "(4096 bytes requested)"), "report: %s (want %s)", msg, want);
        EXPECT(pool.check(msg, sizeof msg) == 0, "the zone was not filled again after the hit: %s", msg);
        // a quarantined block's zone is still checked
        pool.release(a);
        a[4096 + 63] = 1;
        EXPECT(pool.check(msg, sizeof msg) == 1 && std::strstr(msg, "byte 4159 "), "a quarantined block's zone: %s", msg);
        pool.flush(); pool.release(other); pool.flush();
        EXPECT(pool.bytes_live == 0 && pool.check(msg, sizeof msg) == 0, "flush");
        pool.trim(); EXPECT(g_mapped == 0, "trim");
    }
    {   // a size that is no multiple of 16: the zone starts at the next 16-byte boundary (bytes 100..111 are the block's own padding)
        DevPool pool; pool.be_malloc = be_malloc; pool.be_free = be_free; with_redzone(pool, 32);
        unsigned char *a = (unsigned char *)pool.alloc(100);
        std::memset(a, 7, 112);
        EXPECT(pool.check(msg, sizeof msg) == 0, "the padding up to the 16-byte boundary was reported: %s", msg);
        a[112 + 31] = 0;
        EXPECT(pool.check(msg, sizeof msg) == 1 && std::strstr(msg, "byte 143 ") && std::strstr(msg, "(100 bytes requested)"), "last zone byte: %s", msg);
        a[112 + 32] = 0;                                         // beyond the zone: not the pool's to see (the segment's slack)
        EXPECT(pool.check(msg, sizeof msg) == 0, "beyond the zone: %s", msg);
        // a zero-byte request has a zone from its first byte on
        unsigned char *z = (unsigned char *)pool.alloc(0);
        z[0] = 0;
        EXPECT(pool.check(msg, sizeof msg) == 1 && std::strstr(msg, "byte 0 ") && std::strstr(msg, "(0 bytes requested)"), "zero-byte block: %s", msg);
        pool.release(a); pool.release(z); pool.flush(); pool.trim(); EXPECT(g_mapped == 0, "trim");
    }
    {   // quarantine: a released block is handed out to nobody before the flush; live / cached bytes return to their old values after it
        DevPool pool; pool.be_malloc = be_malloc; pool.be_free = be_free; with_redzone(pool, 256);
        void *warm = pool.alloc(32u << 20); pool.release(warm); pool.flush();                    // one region, entirely free
        const size_t live0 = pool.bytes_live, cached0 = pool.bytes_cached, mapped0 = pool.bytes_mapped();
        std::vector<void *> first;
        for (int i = 0; i < 8; ++i) first.push_back(pool.alloc(((size_t)1 + i) << 20));
        for (void *p : first) pool.release(p);
        EXPECT(live_blocks(pool) == 0 && pool.rollback(0) == 0, "quarantined blocks are not live for rollback");
        EXPECT(pool.bytes_live > live0, "quarantined blocks still occupy their memory");
        std::vector<void *> second;
        for (int i = 0; i < 16; ++i) {
            void *p = pool.alloc(((size_t)1 + i % 8) << 20);
            EXPECT(p, "alloc");
            for (void *q : first) EXPECT(p != q, "a quarantined block was handed out before the flush");
            second.push_back(p);
        }
        pool.release(first[0]);                                  // a second release of a quarantined block changes nothing
        for (void *p : second) pool.release(p);
        const size_t mapped1 = pool.bytes_mapped();
        EXPECT(pool.check(msg, sizeof msg) == 0, "clean blocks reported: %s", msg);
        pool.flush();
        EXPECT(pool.bytes_live == live0, "bytes_live %zu after the flush, %zu before", pool.bytes_live, live0);
        EXPECT(pool.bytes_cached == cached0 + (mapped1 - mapped0), "bytes_cached %zu after the flush, %zu before (+%zu mapped)", pool.bytes_cached, cached0, mapped1 - mapped0);
        EXPECT(pool.bytes_live + pool.bytes_cached == pool.bytes_mapped(), "accounting");
        // ... and the flushed blocks coalesced: the first region is one free segment again, handed out whole
        void *again = pool.alloc(32u << 20);
        EXPECT(again == warm, "the first region did not coalesce after the flush");
        pool.release(again); pool.flush(); pool.trim(); EXPECT(g_mapped == 0 && pool.bytes_cached == 0, "trim");
    }
    return 0;
}

// a failed call hands back what it allocated after its mark (DevPool::rollback), with and without red zones
static int rollback_cases(size_t rz)
{
    DevPool pool; pool.be_malloc = be_malloc; pool.be_free = be_free;
    if (rz) with_redzone(pool, rz);
    auto settle = [&]() { if (rz) pool.flush(); };              // (red zones: released blocks are quarantined until the call's end)
    auto accounting = [&]() { return pool.bytes_live + pool.bytes_cached == pool.bytes_mapped() && pool.bytes_mapped() == g_mapped; };
    {   // blocks older than the mark survive, newer ones are released; live bytes return to their value at the mark
        void *old1 = pool.alloc(3u << 20), *old2 = pool.alloc(1000);
        const size_t live0 = pool.bytes_live;
        const unsigned long long m = pool.mark();
        void *n1 = pool.alloc(5u << 20), *n2 = pool.alloc(77), *n3 = pool.alloc(2u << 20);
        EXPECT(n1 && n2 && n3 && pool.bytes_live > live0, "alloc");
        pool.release(n2);                                        // released inside the call: not the rollback's to release again
        EXPECT(pool.rollback(m) == 2, "rollback released the wrong number of blocks");
        settle();
        EXPECT(live_blocks(pool) == 2 && pool.bytes_live == live0, "live %zu blocks / %zu bytes after the rollback, %zu bytes at the mark", live_blocks(pool), pool.bytes_live, live0);
        EXPECT(!pool.segs.at((char *)old1).free && !pool.segs.at((char *)old2).free, "a block older than the mark was released");
        EXPECT(pool.rollback(m) == 0, "a second rollback released something");
        EXPECT(accounting(), "accounting after the rollback");
        pool.release(old1); pool.release(old2); settle();
    }
    {   // a block released after the mark and handed out again at the same address is newer than the mark (a list of the live
        // addresses at the mark would keep it)
        char *a = (char *)pool.alloc(1u << 20);
        const unsigned long long m = pool.mark();
        pool.release(a); settle();
        char *b = (char *)pool.alloc(1u << 20);
        EXPECT(b == a, "the released block was not handed out again at its address (test premise)");
        EXPECT(pool.rollback(m) == 1, "the block re-allocated at an old address survived the rollback");
        settle();
        EXPECT(live_blocks(pool) == 0 && pool.bytes_live == 0 && accounting(), "after the rollback");
    }
    if (rz) {   // quarantined blocks are left alone: released once, not twice; the flush hands them back
        const unsigned long long m = pool.mark();
        void *q = pool.alloc(4096), *l = pool.alloc(8192);
        pool.release(q);
        const size_t live1 = pool.bytes_live;
        EXPECT(pool.rollback(m) == 1 && pool.segs.at((char *)q).quar && pool.segs.at((char *)l).quar, "rollback and the quarantine");
        EXPECT(pool.bytes_live == live1, "a quarantined block's bytes changed at the rollback");
        char msg[320];
        EXPECT(pool.check(msg, sizeof msg) == 0, "clean zones reported: %s", msg);
        pool.flush();
        EXPECT(live_blocks(pool) == 0 && pool.bytes_live == 0 && accounting(), "after the flush");
    }
    pool.trim();
    EXPECT(g_mapped == 0 && pool.bytes_cached == 0, "trim");
    return 0;
}

static int random_sequence(unsigned seed, size_t redzone)
{
    std::mt19937_64 rng(seed);
    DevPool pool; pool.be_malloc = be_malloc; pool.be_free = be_free;
    if (redzone) with_redzone(pool, redzone);
    struct Blk { unsigned char *p; size_t n; unsigned char tag; };
    std::vector<Blk> live;
    size_t fails = 0;
    for (int step = 0; step < 200000; ++step) {
        const bool do_alloc = live.empty() || (rng() % 100 < 52 && live.size() < 400);
        if (do_alloc) {
            size_t n;
            switch (rng() % 4) { case 0: n = 1 + rng() % 4096; break; case 1: n = 1 + rng() % (1u << 20); break; case 2: n = (1u << 20) + rng() % (8u << 20); break; default: n = (8u << 20) + rng() % (64u << 20); }
            unsigned char *p = (unsigned char *)pool.alloc(n);
            if (!p) { ++fails; continue; }
            if (((size_t)p & 255) != 0) { std::printf("FAIL misaligned\n"); return 1; }
            const unsigned char tag = (unsigned char)(rng() & 255);
            std::memset(p, tag, std::min<size_t>(n, 4096)); p[n - 1] = tag;
            live.push_back(Blk{p, n, tag});
        } else {
            const size_t i = rng() % live.size();
            Blk b = live[i]; live[i] = live.back(); live.pop_back();
            for (size_t q = 0; q < std::min<size_t>(b.n, 4096); ++q) if (b.p[q] != b.tag) { std::printf("FAIL pattern (step %d)\n", step); return 1; }
            if (b.p[b.n - 1] != b.tag) { std::printf("FAIL tail pattern (step %d)\n", step); return 1; }
            pool.release(b.p);
        }
        if (redzone && step % 20 == 0) {                         // a call's end: every zone intact (all writes were inside), the quarantine goes
            char msg[320];
            if (pool.check(msg, sizeof msg) != 0) { std::printf("FAIL red zone (step %d): %s\n", step, msg); return 1; }
            pool.flush();
        }
        if (step % 1000 == 0) {
            if (pool.bytes_live + pool.bytes_cached != pool.bytes_mapped() || pool.bytes_mapped() != g_mapped) { std::printf("FAIL accounting %zu + %zu != %zu (%zu)\n", pool.bytes_live, pool.bytes_cached, pool.bytes_mapped(), g_mapped); return 1; }
            // segments tile their regions without gaps or overlaps
            for (auto &r : pool.regions) {
                char *at = r.first; 
                for (auto it = pool.segs.find(r.first); it != pool.segs.end() && it->second.region == r.first; ++it) { if (it->first != at) { std::printf("FAIL gap\n"); return 1; } at += it->second.size; }
                if (at != r.first + r.second) { std::printf("FAIL region not covered\n"); return 1; }
            }
            // no two adjacent free segments of one region (they must have joined)
            for (auto it = pool.segs.begin(); it != pool.segs.end(); ++it) { auto nx = std::next(it); if (nx != pool.segs.end() && it->second.free && nx->second.free && it->second.region == nx->second.region) { std::printf("FAIL uncoalesced\n"); return 1; } }
            if (live_blocks(pool) != live.size()) { std::printf("FAIL live blocks\n"); return 1; }
        }
    }
    // rollback to a mark releases exactly the blocks handed out after it
    const unsigned long long m = pool.mark();
    std::vector<void *> keep; for (auto &b : live) keep.push_back(b.p);
    std::sort(keep.begin(), keep.end());
    size_t added = 0;
    for (int i = 0; i < 50; ++i) added += pool.alloc(1 + rng() % (4u << 20)) != nullptr;
    if (pool.rollback(m) != added) { std::printf("FAIL rollback count\n"); return 1; }
    pool.flush();
    if (pool.bytes_live + pool.bytes_cached != pool.bytes_mapped()) { std::printf("FAIL accounting after the rollback\n"); return 1; }
    { std::vector<void *> now; for (auto &kv : pool.segs) if (!kv.second.free && !kv.second.quar) now.push_back(kv.first); if (now != keep) { std::printf("FAIL rollback\n"); return 1; } }
    for (void *p : keep) pool.release(p);
    pool.flush();
    pool.trim();
    if (pool.bytes_mapped() != 0 || g_mapped != 0 || pool.bytes_cached != 0 || pool.bytes_live != 0) { std::printf("FAIL trim left %zu\n", pool.bytes_mapped()); return 1; }
    std::fprintf(stderr, "seed %u, red zone %zu: %zu allocations refused at the limit, peak live %zu\n", seed, redzone, fails, pool.peak);
    return 0;
}

int main(int argc, char **argv)
{
    const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1;
    if (random_sequence(seed, 0) || random_sequence(seed, 64) || redzone_cases() || rollback_cases(0) || rollback_cases(64)) return 1;
    std::printf("OK seed %u\n", seed);
    return 0;
}
