// CPU exerciser of hysortk_amd/csrc/hsk_pairdecode.h (record index -> occurrence pair of an entry), built with
// -fsanitize=address,undefined by tests/test_pairs_cpu.py.  The decode is held to its definition: r = T(j) + i, T(j) = j (j - 1) / 2,
// i < j -- around every T(j) up to the largest count an entry can have, at both ends of the range, and for every pair of every count
// up to 64 against the pairs written out column by column.
#include <cstdint>
#include <cstdio>

#include "../hysortk_amd/csrc/hsk_pairdecode.h"

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static uint64_t T(uint64_t j) { return j * (j - 1) / 2; }

static void check_one(uint64_t r, uint32_t want_i, uint32_t want_j)
{
    uint32_t i = ~0u, j = ~0u;
    hsk::pair_decode((uint32_t)r, &i, &j);
    CHECK(i == want_i && j == want_j && i < j, "r %llu: (%u, %u), expected (%u, %u)", (unsigned long long)r, i, j, want_i, want_j);
}

int main()
{
    const uint64_t total = hsk::pair_count(hsk::PAIR_MAX_CNT);            // records of the largest entry
    CHECK(total == 2147385345ull, "pair_count(65535) = %llu", (unsigned long long)total);
    CHECK(hsk::pair_count(0) == 0 && hsk::pair_count(1) == 0 && hsk::pair_count(2) == 1 && hsk::pair_count(3) == 3, "small counts");
    check_one(0, 0, 1);
    check_one(total - 1, 65533, 65534);
    uint64_t checked = 0;
    for (uint64_t j = 1; j <= 65534; ++j) {
        // T(j) - 1 is the last pair of column j - 1, T(j) the first of column j, T(j) + 1 its second (or, for j = 1, the first of column 2)
        const uint64_t t = T(j);
        if (t >= 1 && t - 1 < total) { check_one(t - 1, (uint32_t)(j - 2), (uint32_t)(j - 1)); ++checked; }
        if (t < total) { check_one(t, 0, (uint32_t)j); ++checked; }
        if (t + 1 < total) { if (j >= 2) check_one(t + 1, 1, (uint32_t)j); else check_one(t + 1, 0, 2); ++checked; }
    }
    CHECK(checked > 3 * 65000, "only %llu indices checked", (unsigned long long)checked);
    // every pair of every count up to 64, in column order
    for (uint32_t cnt = 0; cnt <= 64; ++cnt) {
        uint32_t r = 0;
        for (uint32_t j = 1; j < cnt; ++j) for (uint32_t i = 0; i < j; ++i) check_one(r++, i, j);
        CHECK(r == hsk::pair_count(cnt), "cnt %u: %u pairs enumerated, pair_count says %u", cnt, r, hsk::pair_count(cnt));
    }
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK %llu boundary indices\n", (unsigned long long)checked);
    return 0;
}
