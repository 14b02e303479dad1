// CPU exerciser of hysortk_amd/csrc/hsk_fmin.h (scan_kernel's window minima as double-precision minima of clamped hashes), built with
// -fsanitize=address,undefined by tests/test_fmin.py.  Held to a brute-force unsigned 64-bit minimum:
//   * a minimum of clamped values that says it is exact IS the minimum of the unclamped ones, and it says so exactly when the true minimum's
//     top word is below the sentinel (so the integer compares run only for windows that lie in the sentinel class as a whole);
//   * the same for a lane's eight windows built as the kernel builds them (the shared middle, a suffix minimum over the lane's own seven, a
//     running minimum over the seven behind), with the wave's second pass through integer compares where a window is not exact.
// Patterns: around the sentinel and 0x7FF00000 (infinity, NaN), zero, all ones, the sign bit, denormals (top word below 0x00100000), equal top
// words with different low words, equal values.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../hysortk_amd/csrc/hsk_fmin.h"

using namespace hsk;
typedef uint64_t u64;
typedef uint32_t u32;

static int g_fail = 0;
static long g_checks = 0;
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static u64 brute_min(const u64 *v, int n) { u64 m = v[0]; for (int i = 1; i < n; ++i) if (v[i] < m) m = v[i]; return m; }

static std::vector<u64> patterns()
{
    const u32 tops[] = {0u, 1u, 0x000FFFFEu, 0x000FFFFFu, 0x00100000u, 0x00100001u, 0x3FF00000u, 0x7FEFFFFDu, 0x7FEFFFFEu, 0x7FEFFFFFu, 0x7FF00000u, 0x7FF00001u,
                        0x7FF80000u, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0x800FFFFFu, 0xBFF00000u, 0xFFEFFFFFu, 0xFFF00000u, 0xFFF80000u, 0xFFFFFFFFu};
    const u32 lows[] = {0u, 1u, 2u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    std::vector<u64> p;
    for (u32 t : tops) for (u32 l : lows) p.push_back(((u64)t << 32) | l);
    return p;
}

// one minimum over v[0..n): clamped chain against brute force
static void check_chain(const u64 *v, int n, const char *what)
{
    u64 m = fmin_clamp(v[0]);
    for (int i = 1; i < n; ++i) m = fmin_u64(m, fmin_clamp(v[i]));
    const u64 want = brute_min(v, n);
    const bool below = (u32)(want >> 32) < FMIN_SENTINEL;
    CHECK(fmin_exact(m) == below, "%s: n %d, exact %d, true minimum %016llx", what, n, (int)fmin_exact(m), (unsigned long long)want);
    if (fmin_exact(m)) CHECK(m == want, "%s: n %d, got %016llx, want %016llx", what, n, (unsigned long long)m, (unsigned long long)want);
    else CHECK((u32)(m >> 32) == FMIN_SENTINEL, "%s: n %d, an inexact minimum %016llx is not at the sentinel", what, n, (unsigned long long)m);
}

// a lane's eight windows of W hashes over s[0 .. W + 7): h = s[0..8) are the lane's own, the rest is what it reads back
template <bool FAST>
static void lane_minima(const u64 *s, int W, u64 (&mn)[8])
{
    auto in = [](u64 v) -> u64 { return FAST ? fmin_clamp(v) : v; };
    auto lower = [](u64 x, u64 y) -> u64 { return FAST ? fmin_u64(x, y) : (y < x ? y : x); };
    u64 c = in(s[7]);
    for (int j = 8; j <= W - 1; ++j) c = lower(c, in(s[j]));
    mn[7] = c;
    u64 suf = in(s[6]);
    mn[6] = lower(suf, c);
    for (int i = 5; i >= 0; --i) { suf = lower(suf, in(s[i])); mn[i] = lower(suf, c); }
    u64 run = in(s[W]);
    mn[1] = lower(run, mn[1]);
    for (int i = 2; i < 8; ++i) { run = lower(run, in(s[W + i - 1])); mn[i] = lower(run, mn[i]); }
}

static long g_second_pass = 0, g_denormal_minima = 0;
static void check_lane(const u64 *s, int W, const char *what)
{
    u64 mn[8];
    lane_minima<true>(s, W, mn);
    bool all_exact = true;
    for (int i = 0; i < 8; ++i) {
        const u64 want = brute_min(s + i, W);
        CHECK(fmin_exact(mn[i]) == ((u32)(want >> 32) < FMIN_SENTINEL), "%s: W %d position %d: exact %d, true minimum %016llx", what, W, i, (int)fmin_exact(mn[i]), (unsigned long long)want);
        if (fmin_exact(mn[i])) { CHECK(mn[i] == want, "%s: W %d position %d: got %016llx, want %016llx", what, W, i, (unsigned long long)mn[i], (unsigned long long)want); if ((want >> 52) == 0) ++g_denormal_minima; }
        else all_exact = false;
    }
    if (!all_exact) { ++g_second_pass; lane_minima<false>(s, W, mn); }
    for (int i = 0; i < 8; ++i) {
        const u64 want = brute_min(s + i, W);
        CHECK(mn[i] == want, "%s: W %d position %d after the second pass: got %016llx, want %016llx", what, W, i, (unsigned long long)mn[i], (unsigned long long)want);
    }
}

int main()
{
    const std::vector<u64> pat = patterns();
    const int np = (int)pat.size();
    // the clamp alone
    for (u64 v : pat) {
        const u64 c = fmin_clamp(v);
        CHECK((u32)c == (u32)v && (u32)(c >> 32) <= FMIN_SENTINEL && (c == v) == ((u32)(v >> 32) <= FMIN_SENTINEL), "clamp of %016llx gives %016llx", (unsigned long long)v, (unsigned long long)c);
    }
    // every pair and every triple of the patterns, in every order
    for (int a = 0; a < np; ++a)
        for (int b = 0; b < np; ++b) {
            const u64 two[2] = {pat[a], pat[b]};
            check_chain(two, 2, "pair");
            for (int c = 0; c < np; c += 3) { const u64 three[3] = {pat[a], pat[b], pat[c]}; check_chain(three, 3, "triple"); }
        }
    // windows drawn from the patterns and from random words, with more or less of the sentinel class
    std::mt19937_64 rng(20240607);
    std::vector<u64> s(64 + 7);
    const int widths[] = {8, 9, 15, 16, 35, 64};
    for (int round = 0; round < 60000; ++round) {
        const int W = widths[round % 6];
        const int kind = (round / 6) % 5;
        for (int i = 0; i < W + 7; ++i) {
            u64 v = rng();
            if (kind == 1) v |= 1ULL << 63;                                                  // all in the class: the second pass every time
            else if (kind == 2) { if (rng() % 8) v |= 1ULL << 63; }                          // mostly in the class
            else if (kind == 3) v = pat[rng() % np];                                         // the edges only
            else if (kind == 4) { if (rng() % 16 == 0) v &= 0x000FFFFFFFFFFFFFULL; else if (rng() % 4 == 0) v = ((u64)FMIN_SENTINEL << 32) | (u32)v; }   // denormals, the sentinel's own top word
            s[i] = v;
        }
        check_lane(s.data(), W, "window");
    }
    CHECK(g_second_pass > 10000 && g_second_pass < 50000, "second passes: %ld of 60000 lanes", g_second_pass);
    CHECK(g_denormal_minima > 10000, "denormal minima: %ld", g_denormal_minima);
    if (g_fail) { std::printf("%d of %ld checks failed\n", g_fail, g_checks); return 1; }
    std::printf("OK %ld checks, %ld second passes, %ld denormal minima\n", g_checks, g_second_pass, g_denormal_minima);
    return 0;
}
