// CPU exerciser of hysortk_amd/csrc/hsk_passplan.h (the radix sort's digit plans), built with -fsanitize=address,undefined by
// tests/test_passplan.py.  Every plan is written into a heap block of exactly the capacity handed to the builder, so a builder that writes
// past it is the sanitizer's finding; the plan itself is held to the definition: the digits of a word tile its used bits, least
// significant first, and an LSD sort that follows the plan orders random keys like a multiword comparison.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../hysortk_amd/csrc/hsk_passplan.h"

using hsk::PassDesc;
using hsk::MAX_PASSES;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// a plan buffer of exactly `cap` entries (no slack: one entry too many is a heap overflow)
struct PlanBuf {
    PassDesc *p; int cap;
    explicit PlanBuf(int cap_) : p(new PassDesc[cap_ > 0 ? cap_ : 1]), cap(cap_) { for (int i = 0; i < cap; ++i) p[i] = PassDesc{-7, -7, -7}; }
    ~PlanBuf() { delete[] p; }
    bool untouched() const { for (int i = 0; i < cap; ++i) if (p[i].word != -7 || p[i].shift != -7 || p[i].bits != -7) return false; return true; }
};

static uint64_t g_rng = 0x243f6a8885a308d3ULL;
static uint64_t rnd()
{
    g_rng += 0x9e3779b97f4a7c15ULL;
    uint64_t x = g_rng;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL; x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
    return x ^ (x >> 31);
}

static int used_bits(int K, int w) { return 2 * std::min(32, K - 32 * w); }

// the pass count by the definition: sum over the words of ceil(used bits / rb)
static int expected_passes(int K, int nw, int rb)
{
    int n = 0;
    for (int w = 0; w < nw; ++w) n += (used_bits(K, w) + rb - 1) / rb;
    return n;
}

struct Key { uint64_t w[3]; uint32_t id; };

// LSD: one stable counting pass per digit of the plan, the digit taken as the kernels take it
static void lsd_sort(std::vector<Key> &a, const PassDesc *plan, int np)
{
    std::vector<Key> b(a.size());
    for (int p = 0; p < np; ++p) {
        const PassDesc pd = plan[p];
        size_t cnt[257] = {0};
        auto digit = [&](const Key &k) { return (uint32_t)(k.w[pd.word] >> pd.shift) & ((1u << pd.bits) - 1); };
        for (const Key &k : a) cnt[digit(k) + 1]++;
        for (int d = 0; d < 256; ++d) cnt[d + 1] += cnt[d];
        for (const Key &k : a) b[cnt[digit(k)]++] = k;
        a.swap(b);
    }
}

static void check_full_plan(int K, int nw, int rb, int *longest, int *beyond24)
{
    const int want = expected_passes(K, nw, rb);
    CHECK(want <= MAX_PASSES, "K=%d nw=%d rb=%d: %d passes, MAX_PASSES=%d", K, nw, rb, want, MAX_PASSES);
    CHECK(hsk::pass_plan_length(K, nw, rb) == want, "K=%d nw=%d rb=%d: pass_plan_length %d, want %d", K, nw, rb, hsk::pass_plan_length(K, nw, rb), want);
    *longest = std::max(*longest, want);
    if (want > 24) ++*beyond24;

    PlanBuf full(MAX_PASSES);
    const int np = hsk::make_pass_plan(K, nw, rb, full.p, full.cap);
    CHECK(np == want, "K=%d nw=%d rb=%d: %d passes, want %d", K, nw, rb, np, want);
    if (np != want || np > MAX_PASSES) return;

    // exactly fitting, and one short: the first is written, the second reported and not written
    PlanBuf exact(want), tight(want - 1);
    CHECK(hsk::make_pass_plan(K, nw, rb, exact.p, exact.cap) == want, "K=%d nw=%d rb=%d: capacity %d refused", K, nw, rb, want);
    CHECK(hsk::make_pass_plan(K, nw, rb, tight.p, tight.cap) == -1, "K=%d nw=%d rb=%d: capacity %d accepted", K, nw, rb, want - 1);
    CHECK(tight.untouched(), "K=%d nw=%d rb=%d: a plan that does not fit was written", K, nw, rb);
    for (int i = 0; i < want; ++i)
        CHECK(exact.p[i].word == full.p[i].word && exact.p[i].shift == full.p[i].shift && exact.p[i].bits == full.p[i].bits, "K=%d nw=%d rb=%d: digit %d depends on the capacity", K, nw, rb, i);

    // the digits of word w tile [64 - used, 64) from the bottom, words ascending; none wider than rb, none across a word; only the last
    // digit of a word is narrower than rb
    int p = 0;
    for (int w = 0; w < nw; ++w) {
        int lo = 64 - used_bits(K, w);
        while (lo < 64 && p < np) {
            const PassDesc pd = full.p[p];
            CHECK(pd.word == w, "K=%d nw=%d rb=%d: digit %d in word %d, want %d", K, nw, rb, p, pd.word, w);
            CHECK(pd.shift == lo, "K=%d nw=%d rb=%d: digit %d at bit %d, want %d", K, nw, rb, p, pd.shift, lo);
            CHECK(pd.bits >= 1 && pd.bits <= rb, "K=%d nw=%d rb=%d: digit %d of %d bits", K, nw, rb, p, pd.bits);
            CHECK(pd.shift + pd.bits <= 64, "K=%d nw=%d rb=%d: digit %d crosses its word (%d + %d)", K, nw, rb, p, pd.shift, pd.bits);
            CHECK(pd.bits == rb || pd.shift + pd.bits == 64, "K=%d nw=%d rb=%d: digit %d is narrow (%d bits) below the top of its word", K, nw, rb, p, pd.bits);
            if (pd.bits < 1) return;
            lo = pd.shift + pd.bits; ++p;
        }
        CHECK(lo == 64, "K=%d nw=%d rb=%d: word %d covered up to bit %d", K, nw, rb, w, lo);
    }
    CHECK(p == np, "K=%d nw=%d rb=%d: %d digits behind the last word", K, nw, rb, np - p);
    if (g_fail) return;

    // what the plan is for: LSD over its digits == order by (word nw-1, ..., word 0), stable
    std::vector<Key> a(300);
    for (size_t i = 0; i < a.size(); ++i) {
        a[i].id = (uint32_t)i;
        for (int w = 0; w < 3; ++w) {
            const int ub = w < nw ? used_bits(K, w) : 0;
            uint64_t v = ub ? (rnd() & (~0ULL << (64 - ub))) : 0;
            if (i % 3 == 1 && w != 0) v = a[i - 1].w[w];                              // neighbours that differ in word 0 only
            if (i % 3 == 2 && ub) v = a[i - 1].w[w] ^ ((rnd() & 1) << (64 - ub));     // ... and in the lowest used bit of a word
            if (i % 5 == 4 && w == nw - 1 && ub) v = a[i - 1].w[w] ^ (1ULL << 63);    // ... and in the top bit of the key
            a[i].w[w] = v;
        }
        if (i % 11 == 10) { for (int w = 0; w < 3; ++w) a[i].w[w] = a[i - 4].w[w]; }   // duplicates: stability
    }
    std::vector<Key> want_order = a;
    std::stable_sort(want_order.begin(), want_order.end(), [&](const Key &x, const Key &y) {
        for (int w = nw - 1; w >= 0; --w) if (x.w[w] != y.w[w]) return x.w[w] < y.w[w];
        return false;
    });
    lsd_sort(a, full.p, np);
    bool same = true;
    for (size_t i = 0; i < a.size(); ++i) if (a[i].id != want_order[i].id) same = false;
    CHECK(same, "K=%d nw=%d rb=%d: LSD over the plan does not order the keys", K, nw, rb);
}

static void check_split_prefix(int top, int nw)
{
    const int low = 16 - top, want = (low + 7) / 8 + (top + 7) / 8;
    PlanBuf exact(want), tight(want - 1);
    const int np = hsk::make_split_prefix_plan(exact.p, exact.cap, top, nw);
    CHECK(np == want, "split prefix top=%d nw=%d: %d passes, want %d", top, nw, np, want);
    CHECK(hsk::make_split_prefix_plan(tight.p, tight.cap, top, nw) == -1 && tight.untouched(), "split prefix top=%d nw=%d: capacity %d not refused", top, nw, want - 1);
    if (np != want) return;
    // the low 16 - top prefix bits are the TOP bits of word nw-2, then the `top` significant bits of word nw-1: 16 bits in all
    int p = 0, total = 0;
    const int words[2] = {nw - 2, nw - 1}, nbits[2] = {low, top};
    for (int h = 0; h < 2; ++h) {
        int lo = 64 - nbits[h];
        while (lo < 64 && p < np) {
            const PassDesc pd = exact.p[p];
            CHECK(pd.word == words[h] && pd.shift == lo, "split prefix top=%d nw=%d: digit %d is word %d bit %d, want word %d bit %d", top, nw, p, pd.word, pd.shift, words[h], lo);
            CHECK(pd.bits >= 1 && pd.bits <= 8 && pd.shift + pd.bits <= 64, "split prefix top=%d nw=%d: digit %d of %d bits at %d", top, nw, p, pd.bits, pd.shift);
            if (pd.bits < 1) return;
            total += pd.bits; lo = pd.shift + pd.bits; ++p;
        }
        CHECK(lo == 64, "split prefix top=%d nw=%d: word %d covered up to bit %d", top, nw, words[h], lo);
    }
    CHECK(p == np && total == 16, "split prefix top=%d nw=%d: %d digits, %d bits", top, nw, np, total);
}

int main()
{
    int ncfg = 0, longest = 0, beyond24 = 0;
    for (int rb = hsk::MIN_RADIX_BITS; rb <= hsk::MAX_RADIX_BITS; ++rb) {
        for (int K = 3; K <= 95; ++K) { if (K % 32 == 0) continue; check_full_plan(K, (K + 31) / 32, rb, &longest, &beyond24); ++ncfg; }
        for (int nw = 1; nw <= 3; ++nw) { check_full_plan(32 * nw, nw, rb, &longest, &beyond24); ++ncfg; }       // hsk_stage_sort: full words
    }
    CHECK(longest == MAX_PASSES, "the longest plan has %d passes, MAX_PASSES = %d", longest, MAX_PASSES);
    CHECK(expected_passes(95, 3, 8) == 24 && expected_passes(51, 2, 4) == 26 && expected_passes(95, 3, 4) == 48 && expected_passes(77, 3, 5) == 32 &&
          expected_passes(96, 3, 4) == 48, "the pass counts of the known cases");

    // outside the ABI's ranges: reported, nothing written
    {
        PlanBuf b(MAX_PASSES);
        CHECK(hsk::make_pass_plan(31, 1, 3, b.p, b.cap) == -1 && hsk::make_pass_plan(31, 1, 9, b.p, b.cap) == -1 && hsk::make_pass_plan(31, 1, 0, b.p, b.cap) == -1, "radix_bits out of range accepted");
        CHECK(hsk::make_pass_plan(31, 2, 8, b.p, b.cap) == -1 && hsk::make_pass_plan(65, 2, 8, b.p, b.cap) == -1 && hsk::make_pass_plan(31, 0, 8, b.p, b.cap) == -1, "K outside its words accepted");
        CHECK(hsk::make_pass_plan(95, 3, 4, b.p, 24) == -1 && hsk::make_pass_plan(51, 2, 4, b.p, 24) == -1, "a plan longer than 24 accepted at capacity 24");
        CHECK(b.untouched(), "a refused plan was written");
    }

    // the split 16-bit prefix: every width the most significant word can hold below 16
    std::set<int> tops;
    for (int K = 3; K <= 95; ++K) { const int nw = (K + 31) / 32; if (K % 32 && nw >= 2 && hsk::prefix_top_bits(K, nw) < 16) tops.insert(hsk::prefix_top_bits(K, nw)); }
    CHECK(tops.size() == 7 && *tops.begin() == 2 && *tops.rbegin() == 14, "prefix_top_bits below 16: %zu widths", tops.size());
    for (int nw = 2; nw <= 3; ++nw) for (int top : tops) check_split_prefix(top, nw);
    for (int K = 3; K <= 95; ++K) { if (K % 32 == 0) continue; const int nw = (K + 31) / 32; CHECK(hsk::prefix_top_bits(K, nw) == std::min(16, used_bits(K, nw - 1)), "prefix_top_bits(%d, %d)", K, nw); }
    {
        PlanBuf b(4);
        CHECK(hsk::make_split_prefix_plan(b.p, b.cap, 16, 2) == -1 && hsk::make_split_prefix_plan(b.p, b.cap, 0, 2) == -1 && hsk::make_split_prefix_plan(b.p, b.cap, 8, 1) == -1 && b.untouched(),
              "split prefix outside its range accepted");
    }

    // the prefix plan: prefix_bits / 8 digits of 8 bits, from bit 64 - prefix_bits of the given word up
    for (int pb = 8; pb <= 64; pb += 8) for (int word = 0; word < 3; ++word) {
        PlanBuf exact(pb / 8), tight(pb / 8 - 1);
        const int np = hsk::make_hybrid_plan(exact.p, exact.cap, pb, word);
        CHECK(np == pb / 8, "prefix plan of %d bits: %d passes", pb, np);
        for (int i = 0; i < np && np == pb / 8; ++i) CHECK(exact.p[i].word == word && exact.p[i].shift == 64 - pb + 8 * i && exact.p[i].bits == 8, "prefix plan of %d bits: digit %d", pb, i);
        CHECK(hsk::make_hybrid_plan(tight.p, tight.cap, pb, word) == -1 && tight.untouched(), "prefix plan of %d bits: capacity %d not refused", pb, pb / 8 - 1);
    }
    {
        PlanBuf b(4);
        CHECK(hsk::make_hybrid_plan(b.p, b.cap) == 4 && b.p[0].shift == hsk::HYBRID_SHIFT && b.p[3].shift == 56, "the default prefix plan");
        PlanBuf u(8);
        CHECK(hsk::make_hybrid_plan(u.p, u.cap, 12, 0) == -1 && hsk::make_hybrid_plan(u.p, u.cap, 0, 0) == -1 && hsk::make_hybrid_plan(u.p, u.cap, 72, 0) == -1 && u.untouched(), "prefix widths outside 8..64 step 8 accepted");
    }

    if (g_fail) { std::printf("FAILED: %d checks\n", g_fail); return 1; }
    std::printf("OK %d full-width plans (radix_bits %d..%d), longest %d passes, %d longer than 24; %zu split prefixes x 2 key widths\n",
                ncfg, hsk::MIN_RADIX_BITS, hsk::MAX_RADIX_BITS, longest, beyond24, tops.size());
    return 0;
}
