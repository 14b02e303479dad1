// CPU exerciser of the no-HIP parts of hysortk_amd/csrc/hsk_rowmerge.h (the merge of row lists: the row shapes, "comes before" on one or
// two words, the merge-path split and the join rule), built with -fsanitize=address,undefined by tests/test_rowmerge.py.  Everything runs
// for both shapes: DiagRow (six words, compared on (key, bin)) and PairRow (four words, compared on the key).  Every list is a heap block
// of exactly n rows of Row::WORDS words, so a read past either list is the sanitizer's finding.  The split is held, for every diagonal d
// in 0 .. na + nb, to the number of A rows among the first d positions of a plain two-pointer merge (A's copy of a key in front of B's);
// and the merge that the kernel does tile by tile -- every tile from its two splits alone, a key of both lists owned by the tile that
// holds A's copy -- is replayed for several tile sizes and held to the two-pointer merge's joined rows.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../hysortk_amd/csrc/hsk_rowmerge.h"

using hsk::DiagRow;
using hsk::MpKey;
using hsk::PairRow;
typedef std::vector<uint64_t> Rows;                      // Row::WORDS words per row

static int g_fail = 0, g_cases = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static uint64_t g_rng;
static uint64_t rnd()
{
    g_rng += 0x9e3779b97f4a7c15ULL;
    uint64_t x = g_rng;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL; x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
    return x ^ (x >> 31);
}

// the row { compare words, sum (both copies), first, last }; a shape compared on one word has no bin
template <typename Row>
static void put_row(Rows &r, uint64_t key, uint64_t bin, uint64_t sum, uint64_t first, uint64_t last)
{
    const int W = Row::WORDS;
    uint64_t row[W];
    row[Row::CMP0] = key; if (Row::NCMP == 2) row[Row::CMP1] = bin;
    row[Row::SUM] = sum; if (Row::SUM2 < W) row[Row::SUM2] = sum;
    row[W - 2] = first; row[W - 1] = last;
    r.insert(r.end(), row, row + W);
}

template <typename Row>
static void add_row(Rows &r, uint64_t key, uint64_t bin)
{
    const uint64_t sup = 1 + (rnd() & 7), first = rnd(), last = rnd();      // first and last use all 64 bits
    put_row<Row>(r, key, bin, sup, first, last);
}

// a heap block of exactly the list's words (an empty list: a block of no words)
static uint64_t *block_of(const Rows &r)
{
    uint64_t *p = new uint64_t[r.size()];
    if (!r.empty()) std::memcpy(p, r.data(), r.size() * 8);
    return p;
}

// the plain two-pointer merge: the joined rows, and for every position of the merged sequence whether it holds an A row.  The order and
// the equality are written out word by word here, not taken from the header.
template <typename Row>
static void plain_merge(const Rows &A, const Rows &B, Rows &out, std::vector<char> &from_a)
{
    const int W = Row::WORDS, K = Row::CMP0, C = Row::CMP1;
    const bool two = Row::NCMP == 2;
    const uint64_t na = A.size() / W, nb = B.size() / W;
    uint64_t i = 0, j = 0;
    out.clear(); from_a.clear();
    while (i < na || j < nb) {
        const uint64_t *a = i < na ? &A[i * W] : nullptr, *b = j < nb ? &B[j * W] : nullptr;
        if (a && b && a[K] == b[K] && (!two || a[C] == b[C])) {
            put_row<Row>(out, a[K], a[C], a[Row::SUM] + b[Row::SUM], a[W - 2] < b[W - 2] ? a[W - 2] : b[W - 2], a[W - 1] > b[W - 1] ? a[W - 1] : b[W - 1]);
            from_a.push_back(1); from_a.push_back(0);
            ++i; ++j;
        } else if (!b || (a && (a[K] < b[K] || (two && a[K] == b[K] && a[C] < b[C])))) { out.insert(out.end(), a, a + W); from_a.push_back(1); ++i; }
        else { out.insert(out.end(), b, b + W); from_a.push_back(0); ++j; }
    }
}

// The kernel's merge on the CPU, tile by tile: a tile knows its two splits and nothing else.  Inside its share the rows are merged by
// mp_before (a tie: A first); an A row joins the row behind it where that has its key -- B[b1], one past the share, for the tile's last
// position -- and a B row is dropped where the row in front of it has its key -- A[a0 - 1] for the first position.
template <typename Row>
static void tiled_merge(const uint64_t *a, uint64_t na, const uint64_t *b, uint64_t nb, uint64_t tile, Rows &out)
{
    const int W = Row::WORDS;
    out.clear();
    const uint64_t total = na + nb;
    for (uint64_t d0 = 0; d0 < total; d0 += tile) {
        const uint64_t d1 = d0 + tile < total ? d0 + tile : total;
        const uint64_t a0 = hsk::mp_split<Row>(a, na, b, nb, d0), a1 = hsk::mp_split<Row>(a, na, b, nb, d1);
        const uint64_t b0 = d0 - a0, b1 = d1 - a1;
        CHECK(a0 <= a1 && a1 <= na && b0 <= b1 && b1 <= nb, "tile %llu: a [%llu, %llu) b [%llu, %llu)", (unsigned long long)d0, (unsigned long long)a0, (unsigned long long)a1, (unsigned long long)b0, (unsigned long long)b1);
        if (!(a0 <= a1 && a1 <= na && b0 <= b1 && b1 <= nb)) return;
        uint64_t i = a0, j = b0;
        const uint64_t *prev = a0 > 0 ? a + (a0 - 1) * W : nullptr;      // the look-behind
        while (i < a1 || j < b1) {
            const bool take_a = j >= b1 || (i < a1 && !hsk::mp_before<Row>(b + j * W, a + i * W));
            if (take_a) {
                const uint64_t *r = a + i * W;
                ++i;
                const uint64_t *nx = nullptr;            // the row at the next position: B's next row of the share, or the look-ahead
                if (j < b1) { if (i >= a1 || hsk::mp_before<Row>(b + j * W, a + i * W)) nx = b + j * W; }
                else if (i >= a1 && b1 < nb) nx = b + b1 * W;
                uint64_t s = r[Row::SUM], f = r[W - 2], l = r[W - 1];
                if (nx && hsk::mp_same<Row>(nx, r)) hsk::mp_join(s, f, l, nx[Row::SUM], nx[W - 2], nx[W - 1]);
                put_row<Row>(out, r[Row::CMP0], r[Row::CMP1], s, f, l);
                prev = r;
            } else {
                const uint64_t *r = b + j * W;
                ++j;
                if (!(prev && hsk::mp_same<Row>(prev, r))) out.insert(out.end(), r, r + W);
                prev = r;
            }
        }
    }
}

template <typename Row>
static void run_case(const char *what, const Rows &A, const Rows &B)
{
    ++g_cases;
    const int W = Row::WORDS;
    const uint64_t na = A.size() / W, nb = B.size() / W;
    for (uint64_t i = 1; i < na; ++i) CHECK(hsk::mp_before<Row>(&A[(i - 1) * W], &A[i * W]), "%s: A is not ascending at %llu", what, (unsigned long long)i);
    for (uint64_t i = 1; i < nb; ++i) CHECK(hsk::mp_before<Row>(&B[(i - 1) * W], &B[i * W]), "%s: B is not ascending at %llu", what, (unsigned long long)i);
    Rows want; std::vector<char> from_a;
    plain_merge<Row>(A, B, want, from_a);
    uint64_t *a = block_of(A), *b = block_of(B);
    // every diagonal
    uint64_t cnt = 0;
    for (uint64_t d = 0; d <= na + nb; ++d) {
        const uint64_t got = hsk::mp_split<Row>(a, na, b, nb, d);
        CHECK(got == cnt, "%s: split(%llu) = %llu, the plain merge has %llu A rows in front", what, (unsigned long long)d, (unsigned long long)got, (unsigned long long)cnt);
        if (d < na + nb) cnt += from_a[d] ? 1 : 0;
    }
    // the tiles
    static const uint64_t tiles[] = {1, 2, 3, 7, 64, 512};
    Rows got;
    for (uint64_t t : tiles) {
        tiled_merge<Row>(a, na, b, nb, t, got);
        CHECK(got == want, "%s: tiles of %llu give %llu rows, the plain merge %llu", what, (unsigned long long)t, (unsigned long long)(got.size() / W), (unsigned long long)(want.size() / W));
    }
    delete[] a; delete[] b;
}

// Ascending rows drawn from a grid of nk keys x nbin bins (offsets key0 / bin0); `which`: bit 0 -> A gets it, bit 1 -> B gets it.  Two
// compare words: cell (k, c) is (key0 + k * kstep, bin0 + c).  One: the cells in the same order are the keys key0 + (k * nbin + c) * kstep.
template <typename Row, typename Pick>
static void grid_case(const char *what, uint64_t nk, uint64_t nbin, uint64_t key0, uint64_t kstep, uint64_t bin0, Pick &&pick)
{
    Rows A, B;
    for (uint64_t k = 0; k < nk; ++k)
        for (uint64_t c = 0; c < nbin; ++c) {
            const int w = pick(k, c);
            const uint64_t key = Row::NCMP == 2 ? key0 + k * kstep : key0 + (k * nbin + c) * kstep;
            if (w & 1) add_row<Row>(A, key, bin0 + c);
            if (w & 2) add_row<Row>(B, key, bin0 + c);
        }
    run_case<Row>(what, A, B);
}

template <typename Row>
static void suite()
{
    const uint64_t TOP = 1ULL << 63, NEAR33 = (1ULL << 33) - 40;
    g_rng = 0x243f6a8885a308d3ULL;
    run_case<Row>("both empty", Rows(), Rows());
    for (uint64_t n : {1, 2, 63, 300}) {
        grid_case<Row>("B empty", n, 1, 5, 3, 1, [](uint64_t, uint64_t) { return 1; });
        grid_case<Row>("A empty", n, 1, 5, 3, 1, [](uint64_t, uint64_t) { return 2; });
        grid_case<Row>("A below B", 2 * n, 1, 5, 3, 1, [n](uint64_t k, uint64_t) { return k < n ? 1 : 2; });
        grid_case<Row>("B below A", 2 * n, 1, 5, 3, 1, [n](uint64_t k, uint64_t) { return k < n ? 2 : 1; });
        grid_case<Row>("A below B inside one key", 1, 2 * n, 5, 3, NEAR33, [n](uint64_t, uint64_t c) { return c < n ? 1 : 2; });
        grid_case<Row>("every row in both", n, 1, 5, 3, 1, [](uint64_t, uint64_t) { return 3; });
        grid_case<Row>("every row in both, one key", 1, n, TOP | 5, 3, 1, [](uint64_t, uint64_t) { return 3; });
    }
    // equal keys, interleaved bins: the order inside a key is word two's alone (bins at 1, and around 2^33)
    if (Row::NCMP == 2)
        for (uint64_t bin0 : {(uint64_t)1, NEAR33}) {
            grid_case<Row>("interleaved bins", 40, 9, 100, 1, bin0, [](uint64_t, uint64_t c) { return c & 1 ? 1 : 2; });
            grid_case<Row>("interleaved bins, reversed", 40, 9, 100, 1, bin0, [](uint64_t, uint64_t c) { return c & 1 ? 2 : 1; });
            grid_case<Row>("bins in runs", 17, 30, TOP - 8, 1, bin0, [](uint64_t k, uint64_t c) { return ((c / 5) + k) & 1 ? 1 : 2; });
        }
    // one shared key at every position of lists that otherwise interleave
    for (uint64_t n : {1, 5, 64, 130})
        for (uint64_t at = 0; at < n; ++at)
            grid_case<Row>("one shared row", 1 + n / 8, 8, TOP - 4, 1, 1, [at](uint64_t k, uint64_t c) { const uint64_t i = k * 8 + c; return i == at ? 3 : (i & 1 ? 1 : 2); });
    // keys with bit 63 set beside keys without; random membership, random sizes up to a few hundred
    for (int rep = 0; rep < 300; ++rep) {
        const uint64_t nk = 1 + rnd() % 60, nbin = 1 + rnd() % 9, pa = rnd() % 101, pb = rnd() % 101;
        grid_case<Row>("random", nk, nbin, TOP - nk / 2, 1, rep & 1 ? NEAR33 : 1, [pa, pb](uint64_t, uint64_t) { return (rnd() % 100 < pa ? 1 : 0) | (rnd() % 100 < pb ? 2 : 0); });
    }
}

static bool before(uint64_t ka, uint64_t ba, uint64_t kb, uint64_t bb) { const MpKey x = {ka, ba}, y = {kb, bb}; return hsk::mp_before(x, y); }

int main()
{
    const uint64_t TOP = 1ULL << 63;
    // "comes before" and the join, word by word
    CHECK(before(1, 9, 2, 0) && !before(2, 0, 1, 9) && before(5, 1, 5, 2) && !before(5, 2, 5, 2) && !before(5, 3, 5, 2), "two words");
    CHECK(before(1, 0, TOP, 0) && !before(TOP, 0, 1, 0) && before(TOP | 1, 1ULL << 33, TOP | 1, (1ULL << 33) + 1) && before(7, 1, 7, TOP), "unsigned words");
    { uint64_t s = 3, f = TOP, l = 5; hsk::mp_join(s, f, l, 4, 9, TOP | 2); CHECK(s == 7 && f == 9 && l == (TOP | 2), "join: %llu %llu %llu", (unsigned long long)s, (unsigned long long)f, (unsigned long long)l); }
    { uint64_t s = ~0ULL - 1, f = 0, l = ~0ULL; hsk::mp_join(s, f, l, 1, 1, 1); CHECK(s == ~0ULL && f == 0 && l == ~0ULL, "join keeps the first row's extremes"); }
    // which words of a row count: (key, bin) of six, the key alone of four
    {
        const uint64_t d1[6] = {5, 9, 1, 9, 8, 8}, d2[6] = {5, 1, 2, 1, 0, 0}, p1[4] = {5, 9, 8, 8}, p2[4] = {5, 1, 0, 0}, p3[4] = {TOP, 0, 0, 0};
        CHECK(hsk::mp_before<DiagRow>(d1, d2) && !hsk::mp_before<DiagRow>(d2, d1) && !hsk::mp_same<DiagRow>(d1, d2) && hsk::mp_same<DiagRow>(d1, d1), "six words: key, then bin");
        CHECK(!hsk::mp_before<PairRow>(p1, p2) && !hsk::mp_before<PairRow>(p2, p1) && hsk::mp_same<PairRow>(p1, p2), "four words: the key alone");
        CHECK(hsk::mp_before<PairRow>(p1, p3) && !hsk::mp_before<PairRow>(p3, p1) && !hsk::mp_same<PairRow>(p1, p3), "four words: unsigned");
    }
    suite<DiagRow>();
    const int diag_cases = g_cases;
    suite<PairRow>();
    if (g_fail) { std::printf("%d checks failed in %d cases\n", g_fail, g_cases); return 1; }
    std::printf("OK %d cases (%d of six-word rows, %d of four-word rows)\n", g_cases, diag_cases, g_cases - diag_cases);
    return 0;
}
