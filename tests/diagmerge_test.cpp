// CPU exerciser of the no-HIP parts of hysortk_amd/csrc/hsk_diagmerge.h (the merge of all-bins row lists: the two-word "comes before", the
// merge-path split and the join rule), built with -fsanitize=address,undefined by tests/test_diagmerge.py.  Every list is a heap block of
// exactly n rows of six words, so a read past either list is the sanitizer's finding.  The split is held, for every diagonal d in
// 0 .. na + nb, to the number of A rows among the first d positions of a plain two-pointer merge (A's copy of a (key, bin) in front of
// B's); and the merge that the kernel does tile by tile -- every tile from its two splits alone, a (key, bin) of both lists owned by the
// tile that holds A's copy -- is replayed for several tile sizes and held to the two-pointer merge's joined rows.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../hysortk_amd/csrc/hsk_diagmerge.h"

using hsk::DM_ROW_WORDS;
typedef std::vector<uint64_t> Rows;                      // six words per row

static int g_fail = 0, g_cases = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static uint64_t g_rng = 0x243f6a8885a308d3ULL;
static uint64_t rnd()
{
    g_rng += 0x9e3779b97f4a7c15ULL;
    uint64_t x = g_rng;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL; x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
    return x ^ (x >> 31);
}

static void add_row(Rows &r, uint64_t key, uint64_t bin)
{
    const uint64_t sup = 1 + (rnd() & 7);
    const uint64_t row[6] = {key, sup, bin, sup, rnd(), rnd()};      // first and last use all 64 bits
    r.insert(r.end(), row, row + 6);
}

// a heap block of exactly the list's words (an empty list: a block of no words)
static uint64_t *block_of(const Rows &r)
{
    uint64_t *p = new uint64_t[r.size()];
    if (!r.empty()) std::memcpy(p, r.data(), r.size() * 8);
    return p;
}

// the plain two-pointer merge: the joined rows, and for every position of the merged sequence whether it holds an A row
static void plain_merge(const Rows &A, const Rows &B, Rows &out, std::vector<char> &from_a)
{
    const uint64_t na = A.size() / 6, nb = B.size() / 6;
    uint64_t i = 0, j = 0;
    out.clear(); from_a.clear();
    while (i < na || j < nb) {
        const uint64_t *a = i < na ? &A[i * 6] : nullptr, *b = j < nb ? &B[j * 6] : nullptr;
        if (a && b && a[0] == b[0] && a[2] == b[2]) {
            const uint64_t s = a[1] + b[1];
            const uint64_t row[6] = {a[0], s, a[2], s, a[4] < b[4] ? a[4] : b[4], a[5] > b[5] ? a[5] : b[5]};
            out.insert(out.end(), row, row + 6); from_a.push_back(1); from_a.push_back(0);
            ++i; ++j;
        } else if (!b || (a && (a[0] < b[0] || (a[0] == b[0] && a[2] < b[2])))) { out.insert(out.end(), a, a + 6); from_a.push_back(1); ++i; }
        else { out.insert(out.end(), b, b + 6); from_a.push_back(0); ++j; }
    }
}

// The kernel's merge on the CPU, tile by tile: a tile knows its two splits and nothing else.  Inside its share the rows are merged by
// dm_before (a tie: A first); an A row joins the row behind it where that has its (key, bin) -- B[b1], one past the share, for the
// tile's last position -- and a B row is dropped where the row in front of it has its (key, bin) -- A[a0 - 1] for the first position.
static void tiled_merge(const uint64_t *a, uint64_t na, const uint64_t *b, uint64_t nb, uint64_t tile, Rows &out)
{
    out.clear();
    const uint64_t total = na + nb;
    for (uint64_t d0 = 0; d0 < total; d0 += tile) {
        const uint64_t d1 = d0 + tile < total ? d0 + tile : total;
        const uint64_t a0 = hsk::dm_split(a, na, b, nb, d0), a1 = hsk::dm_split(a, na, b, nb, d1);
        const uint64_t b0 = d0 - a0, b1 = d1 - a1;
        CHECK(a0 <= a1 && a1 <= na && b0 <= b1 && b1 <= nb, "tile %llu: a [%llu, %llu) b [%llu, %llu)", (unsigned long long)d0, (unsigned long long)a0, (unsigned long long)a1, (unsigned long long)b0, (unsigned long long)b1);
        if (!(a0 <= a1 && a1 <= na && b0 <= b1 && b1 <= nb)) return;
        uint64_t i = a0, j = b0;
        const uint64_t *prev = a0 > 0 ? a + (a0 - 1) * 6 : nullptr;      // the look-behind
        while (i < a1 || j < b1) {
            const bool take_a = j >= b1 || (i < a1 && !hsk::dm_before(b[j * 6], b[j * 6 + 2], a[i * 6], a[i * 6 + 2]));
            if (take_a) {
                const uint64_t *r = a + i * 6;
                ++i;
                const uint64_t *nx = nullptr;            // the row at the next position: B's next row of the share, or the look-ahead
                if (j < b1) { if (i >= a1 || hsk::dm_before(b[j * 6], b[j * 6 + 2], a[i * 6], a[i * 6 + 2])) nx = b + j * 6; }
                else if (i >= a1 && b1 < nb) nx = b + b1 * 6;
                uint64_t s = r[1], f = r[4], l = r[5];
                if (nx && nx[0] == r[0] && nx[2] == r[2]) hsk::dm_join(s, f, l, nx[1], nx[4], nx[5]);
                const uint64_t row[6] = {r[0], s, r[2], s, f, l};
                out.insert(out.end(), row, row + 6);
                prev = r;
            } else {
                const uint64_t *r = b + j * 6;
                ++j;
                if (!(prev && prev[0] == r[0] && prev[2] == r[2])) out.insert(out.end(), r, r + 6);
                prev = r;
            }
        }
    }
}

static void run_case(const char *what, const Rows &A, const Rows &B)
{
    ++g_cases;
    const uint64_t na = A.size() / 6, nb = B.size() / 6;
    for (uint64_t i = 1; i < na; ++i) CHECK(hsk::dm_before(A[(i - 1) * 6], A[(i - 1) * 6 + 2], A[i * 6], A[i * 6 + 2]), "%s: A is not ascending at %llu", what, (unsigned long long)i);
    for (uint64_t i = 1; i < nb; ++i) CHECK(hsk::dm_before(B[(i - 1) * 6], B[(i - 1) * 6 + 2], B[i * 6], B[i * 6 + 2]), "%s: B is not ascending at %llu", what, (unsigned long long)i);
    Rows want; std::vector<char> from_a;
    plain_merge(A, B, want, from_a);
    uint64_t *a = block_of(A), *b = block_of(B);
    // every diagonal
    uint64_t cnt = 0;
    for (uint64_t d = 0; d <= na + nb; ++d) {
        const uint64_t got = hsk::dm_split(a, na, b, nb, d);
        CHECK(got == cnt, "%s: split(%llu) = %llu, the plain merge has %llu A rows in front", what, (unsigned long long)d, (unsigned long long)got, (unsigned long long)cnt);
        if (d < na + nb) cnt += from_a[d] ? 1 : 0;
    }
    // the tiles
    static const uint64_t tiles[] = {1, 2, 3, 7, 64, 512};
    Rows got;
    for (uint64_t t : tiles) {
        tiled_merge(a, na, b, nb, t, got);
        CHECK(got == want, "%s: tiles of %llu give %llu rows, the plain merge %llu", what, (unsigned long long)t, (unsigned long long)(got.size() / 6), (unsigned long long)(want.size() / 6));
    }
    delete[] a; delete[] b;
}

// n ascending (key, bin) drawn from a grid of nk keys x nbin bins (offsets key0 / bin0); `which`: bit 0 -> A gets it, bit 1 -> B gets it
template <typename Pick>
static void grid_case(const char *what, uint64_t nk, uint64_t nbin, uint64_t key0, uint64_t kstep, uint64_t bin0, Pick &&pick)
{
    Rows A, B;
    for (uint64_t k = 0; k < nk; ++k)
        for (uint64_t c = 0; c < nbin; ++c) {
            const int w = pick(k, c);
            if (w & 1) add_row(A, key0 + k * kstep, bin0 + c);
            if (w & 2) add_row(B, key0 + k * kstep, bin0 + c);
        }
    run_case(what, A, B);
}

int main()
{
    const uint64_t TOP = 1ULL << 63, NEAR33 = (1ULL << 33) - 40;
    // "comes before" and the join, word by word
    CHECK(hsk::dm_before(1, 9, 2, 0) && !hsk::dm_before(2, 0, 1, 9) && hsk::dm_before(5, 1, 5, 2) && !hsk::dm_before(5, 2, 5, 2) && !hsk::dm_before(5, 3, 5, 2), "two words");
    CHECK(hsk::dm_before(1, 0, TOP, 0) && !hsk::dm_before(TOP, 0, 1, 0) && hsk::dm_before(TOP | 1, 1ULL << 33, TOP | 1, (1ULL << 33) + 1) && hsk::dm_before(7, 1, 7, TOP), "unsigned words");
    { uint64_t s = 3, f = TOP, l = 5; hsk::dm_join(s, f, l, 4, 9, TOP | 2); CHECK(s == 7 && f == 9 && l == (TOP | 2), "join: %llu %llu %llu", (unsigned long long)s, (unsigned long long)f, (unsigned long long)l); }
    { uint64_t s = ~0ULL - 1, f = 0, l = ~0ULL; hsk::dm_join(s, f, l, 1, 1, 1); CHECK(s == ~0ULL && f == 0 && l == ~0ULL, "join keeps the first row's extremes"); }

    run_case("both empty", Rows(), Rows());
    for (uint64_t n : {1, 2, 63, 300}) {
        grid_case("B empty", n, 1, 5, 3, 1, [](uint64_t, uint64_t) { return 1; });
        grid_case("A empty", n, 1, 5, 3, 1, [](uint64_t, uint64_t) { return 2; });
        grid_case("A below B", 2 * n, 1, 5, 3, 1, [n](uint64_t k, uint64_t) { return k < n ? 1 : 2; });
        grid_case("B below A", 2 * n, 1, 5, 3, 1, [n](uint64_t k, uint64_t) { return k < n ? 2 : 1; });
        grid_case("A below B inside one key", 1, 2 * n, 5, 3, NEAR33, [n](uint64_t, uint64_t c) { return c < n ? 1 : 2; });
        grid_case("every row in both", n, 1, 5, 3, 1, [](uint64_t, uint64_t) { return 3; });
        grid_case("every row in both, one key", 1, n, TOP | 5, 3, 1, [](uint64_t, uint64_t) { return 3; });
    }
    // equal keys, interleaved bins: the order inside a key is word two's alone (bins at 1, and around 2^33)
    for (uint64_t bin0 : {(uint64_t)1, NEAR33}) {
        grid_case("interleaved bins", 40, 9, 100, 1, bin0, [](uint64_t, uint64_t c) { return c & 1 ? 1 : 2; });
        grid_case("interleaved bins, reversed", 40, 9, 100, 1, bin0, [](uint64_t, uint64_t c) { return c & 1 ? 2 : 1; });
        grid_case("bins in runs", 17, 30, TOP - 8, 1, bin0, [](uint64_t k, uint64_t c) { return ((c / 5) + k) & 1 ? 1 : 2; });
    }
    // one shared (key, bin) at every position of lists that otherwise interleave
    for (uint64_t n : {1, 5, 64, 130})
        for (uint64_t at = 0; at < n; ++at)
            grid_case("one shared row", 1 + n / 8, 8, TOP - 4, 1, 1, [at](uint64_t k, uint64_t c) { const uint64_t i = k * 8 + c; return i == at ? 3 : (i & 1 ? 1 : 2); });
    // keys with bit 63 set beside keys without; random membership, random sizes up to a few hundred
    for (int rep = 0; rep < 300; ++rep) {
        const uint64_t nk = 1 + rnd() % 60, nbin = 1 + rnd() % 9, pa = rnd() % 101, pb = rnd() % 101;
        grid_case("random", nk, nbin, TOP - nk / 2, 1, rep & 1 ? NEAR33 : 1, [pa, pb](uint64_t, uint64_t) { return (rnd() % 100 < pa ? 1 : 0) | (rnd() % 100 < pb ? 2 : 0); });
    }
    if (g_fail) { std::printf("%d checks failed in %d cases\n", g_fail, g_cases); return 1; }
    std::printf("OK %d cases\n", g_cases);
    return 0;
}
