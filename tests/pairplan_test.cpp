// CPU exerciser of hysortk_amd/csrc/hsk_pairplan.h (the slices of hsk_result_pairs_sliced), built with -fsanitize=address,undefined by
// tests/test_pairplan.py.  Every offset array is a heap block of exactly nent + 1 words and every cut array one of exactly the bound the
// planner states, so a read or write past either is the sanitizer's finding.  The cuts are held to a plain loop over the entries and to
// the definition: strictly increasing up to nent, every slice within the budget or a single entry, no slice able to take one more entry.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../hysortk_amd/csrc/hsk_pairplan.h"

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static uint64_t g_rng = 0x13198a2e03707344ULL;
static uint64_t rnd()
{
    g_rng += 0x9e3779b97f4a7c15ULL;
    uint64_t x = g_rng;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL; x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
    return x ^ (x >> 31);
}

// the plain loop: walk the entries one by one while the slice stays within the budget
static uint64_t next_plain(const uint64_t *off, uint64_t nent, uint64_t from, uint64_t max_records)
{
    uint64_t e = from + 1;
    while (e < nent && off[e + 1] - off[from] <= max_records) ++e;
    return e;
}

static int g_cases = 0;

// t[e] = records of entry e, base = the offset of entry 0 (the planner only takes differences)
static void run_case(const char *what, const std::vector<uint64_t> &t, uint64_t max_records, uint64_t base = 0)
{
    ++g_cases;
    const uint64_t nent = t.size();
    uint64_t *off = new uint64_t[nent + 1];              // exactly nent + 1 words
    off[0] = base;
    for (uint64_t e = 0; e < nent; ++e) off[e + 1] = off[e] + t[e];
    const uint64_t records = off[nent] - off[0];
    const uint64_t cap = hsk::pair_plan_max_slices(nent, records, max_records);
    uint64_t *cut = new uint64_t[cap ? cap : 1];         // exactly the bound the planner states
    const uint64_t n = hsk::pair_plan_all(off, nent, max_records, cut, cap);
    CHECK(nent == 0 ? n == 0 : (n >= 1 && n <= cap && cut[n - 1] == nent), "%s: %llu cuts (bound %llu), the last one %llu of %llu entries", what,
          (unsigned long long)n, (unsigned long long)cap, (unsigned long long)(n ? cut[n - 1] : 0), (unsigned long long)nent);
    uint64_t from = 0, plain = 0;
    for (uint64_t i = 0; i < n && g_fail == 0; ++i) {
        const uint64_t e = cut[i];
        CHECK(e > from && e <= nent, "%s: cut %llu = %llu behind %llu", what, (unsigned long long)i, (unsigned long long)e, (unsigned long long)from);
        if (!(e > from && e <= nent)) break;
        plain = next_plain(off, nent, from, max_records);
        CHECK(e == plain, "%s: cut %llu = %llu, the plain loop says %llu", what, (unsigned long long)i, (unsigned long long)e, (unsigned long long)plain);
        CHECK(hsk::pair_plan_next(off, nent, from, max_records) == e, "%s: pair_plan_next disagrees with pair_plan_all at %llu", what, (unsigned long long)from);
        const uint64_t held = off[e] - off[from];
        CHECK(held <= max_records || e == from + 1, "%s: slice [%llu, %llu) holds %llu records, budget %llu", what, (unsigned long long)from, (unsigned long long)e,
              (unsigned long long)held, (unsigned long long)max_records);
        CHECK(e == nent || off[e + 1] - off[from] > max_records, "%s: slice [%llu, %llu) could have taken entry %llu", what, (unsigned long long)from, (unsigned long long)e, (unsigned long long)e);
        from = e;
    }
    // a cut array that is too small is filled and no further
    if (n >= 2) {
        uint64_t *small = new uint64_t[n - 1];
        const uint64_t m = hsk::pair_plan_all(off, nent, max_records, small, n - 1);
        CHECK(m == n - 1 && small[m - 1] == cut[n - 2], "%s: a cut array of %llu entries", what, (unsigned long long)(n - 1));
        delete[] small;
    }
    delete[] cut;
    delete[] off;
}

int main()
{
    // all entries without records
    run_case("no records, one entry", std::vector<uint64_t>(1, 0), 1);
    run_case("no records", std::vector<uint64_t>(1000, 0), 1);
    run_case("no records, large budget", std::vector<uint64_t>(1000, 0), ~0ULL);
    run_case("no entries", std::vector<uint64_t>(), 5);

    // long runs of equal offsets before and after a cut
    for (uint64_t budget : {1ULL, 9ULL, 10ULL, 11ULL, 19ULL, 20ULL, 21ULL, 1000ULL}) {
        std::vector<uint64_t> t;
        t.insert(t.end(), 3000, 0); t.push_back(10); t.insert(t.end(), 5000, 0); t.push_back(10); t.insert(t.end(), 2000, 0); t.push_back(1); t.insert(t.end(), 4000, 0);
        run_case("runs of equal offsets", t, budget);
        std::vector<uint64_t> u(7, 0); u.push_back(10); u.push_back(10); u.insert(u.end(), 7, 0);
        run_case("runs at both ends", u, budget);
    }

    // one entry larger than the budget at the start, in the middle and at the end
    for (int where = 0; where < 3; ++where)
        for (uint64_t budget : {1ULL, 5ULL, 44849ULL, 44850ULL, 44851ULL, 44860ULL}) {
            std::vector<uint64_t> t(41, 3);
            t[where == 0 ? 0 : where == 1 ? 20 : 40] = 44850;
            run_case("one entry above the budget", t, budget);
            std::vector<uint64_t> z(41, 0);
            z[where == 0 ? 0 : where == 1 ? 20 : 40] = 44850;
            run_case("one entry above the budget among entries without records", z, budget);
        }
    run_case("every entry above the budget", std::vector<uint64_t>(100, 44850), 100);

    // budget 1; a budget at or above the total
    {
        std::vector<uint64_t> t;
        for (int i = 0; i < 500; ++i) t.push_back(rnd() % 4);
        uint64_t total = 0; for (uint64_t x : t) total += x;
        run_case("budget 1", t, 1);
        run_case("budget 2", t, 2);
        run_case("budget total - 1", t, total - 1);
        run_case("budget total", t, total);
        run_case("budget total + 1", t, total + 1);
        run_case("budget 10 x total", t, 10 * total);
        run_case("budget 2^64 - 1", t, ~0ULL);
        run_case("budget 2^64 - 1 on high offsets", t, ~0ULL, ~0ULL - total);
    }

    // offsets near 2^40 (a range of 10^12 records) and beyond 2^63
    for (uint64_t base : {0ULL, 1ULL << 40, (1ULL << 63) + 12345}) {
        std::vector<uint64_t> t;
        for (int i = 0; i < 3000; ++i) t.push_back((rnd() % 5 == 0) ? 0 : rnd() % 2147385346ULL);
        run_case("large entries", t, 1ULL << 33, base);
        run_case("large entries, small budget", t, 1000, base);
        std::vector<uint64_t> w(1100, 1ULL << 30);                       // the offsets themselves reach 2^40
        run_case("offsets up to 2^40", w, (1ULL << 36) + 7, base);
    }

    // random arrays against the plain loop
    for (int it = 0; it < 400; ++it) {
        const uint64_t nent = 1 + rnd() % 300;
        std::vector<uint64_t> t(nent);
        const uint64_t zero_in = 1 + rnd() % 6, top = 1 + rnd() % 50;
        for (auto &x : t) x = (rnd() % zero_in) ? 0 : rnd() % top;
        run_case("random", t, 1 + rnd() % 120);
    }

    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK %d cases\n", g_cases);
    return 0;
}
