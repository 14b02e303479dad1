// CPU exerciser of hysortk_amd/csrc/hsk_xdrop.h (the 32-column windows of two reads, their mismatch masks, the x-drop step by runs, the
// valid columns and the overlap row), built with -fsanitize=address,undefined by tests/test_xdrop.py.  Every packed buffer is a heap block of
// exactly the bytes the reads take, so a load that touches a byte behind the last read's last base is an AddressSanitizer report.
// Windows are held to strings, the step to the column-by-column loop of the definition (include/hsk.h: hsk_pair_diags_extend).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../hysortk_amd/csrc/hsk_xdrop.h"

using namespace hsk;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }

static int code(char c) { return c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 0; }      // (N is A)
static std::string revcomp(const std::string &s)
{
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = "TGCA"[code(c)];
    return r;
}
static std::string random_read(size_t n) { std::string s(n, 'A'); for (char &c : s) c = "ACGT"[rnd() & 3]; return s; }

// reads packed as hsk_count reads them, every read from a byte boundary, in a heap block of exactly their bytes
struct Packed {
    uint8_t *p = nullptr; uint64_t nbytes = 0; std::vector<uint64_t> off;
    explicit Packed(const std::vector<std::string> &reads)
    {
        for (const auto &r : reads) { off.push_back(nbytes); nbytes += (r.size() + 3) / 4; }
        p = (uint8_t *)std::malloc(nbytes ? nbytes : 1);                               // (16-byte aligned, and the block ends at the last byte)
        std::memset(p, 0, nbytes);
        for (size_t k = 0; k < reads.size(); ++k)
            for (size_t i = 0; i < reads[k].size(); ++i) p[off[k] + i / 4] |= (uint8_t)(code(reads[k][i]) << (6 - 2 * (i % 4)));
    }
    ~Packed() { std::free(p); }
};

static uint64_t g_windows = 0, g_steps = 0, g_walks = 0;

// ---- the definition, column by column on strings ------------------------------------------------------------------------------------
struct RefSide { int64_t best; int64_t edge; uint32_t mm; };     // edge: columns taken at best

static bool col_match(const std::string &a, const std::string &b, int64_t pa, int64_t pb, int k, int o, int64_t t)
{
    const int x = code(a[pa + t]);
    const int y = o ? 3 - code(b[pb + k - 1 - t]) : code(b[pb + t]);
    return x == y;
}

static void ref_range(int64_t la, int64_t lb, int64_t pa, int64_t pb, int64_t k, int o, int64_t *lo, int64_t *hi)
{
    if (!o) { *lo = -std::min(pa, pb); *hi = std::min(la - pa, lb - pb); }
    else { *lo = std::max(-pa, pb + k - lb); *hi = std::min(la - pa, pb + k); }
}

static RefSide ref_side(const std::string &a, const std::string &b, int64_t pa, int64_t pb, int k, int o, bool right, int64_t match, int64_t mismatch, int64_t xdrop)
{
    int64_t lo, hi; ref_range(a.size(), b.size(), pa, pb, k, o, &lo, &hi);
    int64_t s = 0, best = 0, edge = 0;
    if (right) { for (int64_t t = k; t < hi; ++t) { s += col_match(a, b, pa, pb, k, o, t) ? match : -mismatch; if (s > best) { best = s; edge = t + 1 - k; } if (best - s > xdrop) break; } }
    else { for (int64_t t = -1; t >= lo; --t) { s += col_match(a, b, pa, pb, k, o, t) ? match : -mismatch; if (s > best) { best = s; edge = -t; } if (best - s > xdrop) break; } }
    uint32_t mm = 0;
    for (int64_t c = 0; c < edge; ++c) mm += !col_match(a, b, pa, pb, k, o, right ? k + c : -1 - c);
    return RefSide{best, edge, mm};
}

// ---- windows: every base offset of the last read(s) of a block, forward and reverse-complemented, against the strings --------------------
static void check_windows(const std::vector<std::string> &reads)
{
    const Packed pk(reads);
    const size_t last = reads.size() - 1;
    const std::string &rd = reads[last];
    const std::string rc = revcomp(rd);
    XdPair p; std::memset(&p, 0, sizeof p);
    p.bit_a = p.bit_b = 8 * pk.off[last]; p.la = p.lb = (uint32_t)rd.size(); p.k = 3;
    for (int64_t i = -40; i < (int64_t)rd.size() + 8; ++i) {
        // forward: bases i .. i + 31 (those inside the read are checked; the others are whatever lies there)
        p.pa = 0; p.o = 0; p.pb = 0;
        const uint64_t w = xd_window_a(pk.p, pk.nbytes, p, i), wb = xd_window_b(pk.p, pk.nbytes, p, i);
        CHECK(w == wb, "forward windows of one read differ at %lld", (long long)i);
        for (int c = 0; c < 32; ++c) {
            const int64_t j = i + c;
            if (j < 0 || j >= (int64_t)rd.size()) continue;
            CHECK((int)((w >> (62 - 2 * c)) & 3) == code(rd[j]), "base %lld of a read of %zu (window at %lld)", (long long)j, rd.size(), (long long)i);
        }
        // opposite strand with pb = 0, k = 3: column t + c is the complement of B[2 - t - c] = base (lb - 3 + t + c) of the reverse complement
        p.o = 1;
        const uint64_t wr = xd_window_b(pk.p, pk.nbytes, p, i);
        for (int c = 0; c < 32; ++c) {
            const int64_t j = 2 - i - c;
            if (j < 0 || j >= (int64_t)rd.size()) continue;
            CHECK((int)((wr >> (62 - 2 * c)) & 3) == 3 - code(rd[j]), "complement of base %lld of a read of %zu (window at %lld)", (long long)j, rd.size(), (long long)i);
            CHECK((int)((wr >> (62 - 2 * c)) & 3) == code(rc[rd.size() - 1 - j]), "reverse complement string");
        }
        ++g_windows;
    }
}

// ---- the step by runs against the column loop, on masks ---------------------------------------------------------------------------------
static void check_step(uint32_t total, uint32_t density, int64_t match, int64_t mismatch, int64_t xdrop, uint32_t first_n)
{
    // a walk of `total` positions whose first window has first_n of them (every start column mod 32), then whole windows
    std::vector<int> mis(total);
    for (auto &b : mis) b = (rnd() % 100) < density;
    int64_t s = 0, best = 0; uint32_t edge = 0, stopped_at = total;
    for (uint32_t c = 0; c < total; ++c) { s += mis[c] ? -mismatch : match; if (s > best) { best = s; edge = c + 1; } if (best - s > xdrop) { stopped_at = c; break; } }
    uint32_t mm = 0; for (uint32_t c = 0; c < edge; ++c) mm += mis[c];
    XdSide st; bool drop = false; uint32_t c0 = 0, drop_window_end = 0;
    while (c0 < total && !drop) {
        const uint32_t n = std::min<uint32_t>(c0 == 0 ? first_n : 32, total - c0);
        uint64_t m = 0; for (uint32_t i = 0; i < n; ++i) if (mis[c0 + i]) m |= 1ULL << (2 * i);
        drop = xd_step(st, m, n, c0, match, mismatch, xdrop);
        c0 += n; drop_window_end = c0;
    }
    CHECK(st.best == best && st.len == edge && st.mm == mm, "step: best %lld/%lld len %u/%u mm %u/%u (total %u match %lld mismatch %lld xdrop %lld)", (long long)st.best, (long long)best, st.len, edge, st.mm, mm,
          total, (long long)match, (long long)mismatch, (long long)xdrop);
    CHECK(drop == (stopped_at < total), "step: stop %d, the loop stops at %u of %u", (int)drop, stopped_at, total);
    if (drop) CHECK(stopped_at < drop_window_end && stopped_at + 32 >= drop_window_end, "the stop lies in the window that reported it");
    ++g_steps;
}

// ---- whole walks on packed reads, and the row ---------------------------------------------------------------------------------------------
static std::string mutate(std::string s, uint32_t percent, size_t keep_lo, size_t keep_hi)
{
    for (size_t i = 0; i < s.size(); ++i) if ((i < keep_lo || i >= keep_hi) && rnd() % 100 < percent) s[i] = "ACGT"[(code(s[i]) + 1 + rnd() % 3) & 3];
    return s;
}

static void check_pair(const std::vector<std::string> &front, const std::string &a, const std::string &b, uint32_t pa, uint32_t pb, int k, int o, int64_t match, int64_t mismatch, int64_t xdrop)
{
    std::vector<std::string> reads = front; reads.push_back(a); reads.push_back(b);
    const Packed pk(reads);
    XdPair p; std::memset(&p, 0, sizeof p);
    p.bit_a = 8 * pk.off[reads.size() - 2]; p.bit_b = 8 * pk.off[reads.size() - 1];
    p.pa = pa; p.pb = pb; p.la = (uint32_t)a.size(); p.lb = (uint32_t)b.size(); p.k = k; p.o = o;
    xd_range(p);
    int64_t lo, hi; ref_range(a.size(), b.size(), pa, pb, k, o, &lo, &hi);
    CHECK(p.t_lo == lo && p.t_hi == hi && lo <= 0 && hi >= k, "range [%lld, %lld) / [%lld, %lld)", (long long)p.t_lo, (long long)p.t_hi, (long long)lo, (long long)hi);
    bool seed = true; for (int t = 0; t < k; ++t) seed = seed && col_match(a, b, pa, pb, k, o, t);
    CHECK(xd_seed_matches(pk.p, pk.nbytes, p) == seed, "seed check (%d)", (int)seed);
    if (!seed) return;
    const XdSide r = xd_walk(pk.p, pk.nbytes, p, true, match, mismatch, xdrop), l = xd_walk(pk.p, pk.nbytes, p, false, match, mismatch, xdrop);
    const RefSide rr = ref_side(a, b, pa, pb, k, o, true, match, mismatch, xdrop), rl = ref_side(a, b, pa, pb, k, o, false, match, mismatch, xdrop);
    CHECK(r.best == rr.best && r.len == rr.edge && r.mm == rr.mm, "right: best %lld/%lld len %u/%lld mm %u/%u (la %zu lb %zu pa %u pb %u k %d o %d)", (long long)r.best, (long long)rr.best, r.len, (long long)rr.edge, r.mm, rr.mm,
          a.size(), b.size(), pa, pb, k, o);
    CHECK(l.best == rl.best && l.len == rl.edge && l.mm == rl.mm, "left: best %lld/%lld len %u/%lld mm %u/%u (la %zu lb %zu pa %u pb %u k %d o %d)", (long long)l.best, (long long)rl.best, l.len, (long long)rl.edge, l.mm, rl.mm,
          a.size(), b.size(), pa, pb, k, o);
    uint64_t row[XD_ROW_WORDS];
    xd_row(p, 0x8000000100000002ULL, 77, match, l, r, row);
    const int64_t begin = -rl.edge, end = k + rr.edge;
    const uint64_t a_lo = pa + begin, a_hi = pa + end, b_lo = o ? pb + k - end : pb + begin, b_hi = o ? pb + k - begin : pb + end;
    const uint64_t ends = (a_lo == 0) | (a_hi == a.size()) << 1 | (b_lo == 0) << 2 | (b_hi == b.size()) << 3;
    CHECK(row[0] == 0x8000000100000002ULL && row[5] == 77, "key and support pass through");
    CHECK(row[1] == (uint64_t)(k * match + rr.best + rl.best), "score");
    CHECK(row[2] == (a_lo << 32 | a_hi) && row[3] == (b_lo << 32 | b_hi), "coordinates a [%llu, %llu) b [%llu, %llu)", (unsigned long long)a_lo, (unsigned long long)a_hi, (unsigned long long)b_lo, (unsigned long long)b_hi);
    CHECK(row[4] == ((uint64_t)(rr.mm + rl.mm) << 32 | ends), "mismatches and ends (%llu)", (unsigned long long)ends);
    CHECK(b_hi <= b.size() && a_hi <= a.size() && b_hi - b_lo == a_hi - a_lo, "the overlap lies inside both reads");
    ++g_walks;
}

// an overlap of two reads cut from one genome: A = g[sa, sa + la), B = g[sb, sb + lb) or its reverse complement, the seed at genome position gs
static void check_overlap(const std::string &g, size_t sa, size_t la, size_t sb, size_t lb, size_t gs, int k, int o, uint32_t percent, int64_t match, int64_t mismatch, int64_t xdrop, size_t nfront)
{
    std::string a = g.substr(sa, la), bf = g.substr(sb, lb);
    a = mutate(a, percent, gs - sa, gs - sa + k);
    bf = mutate(bf, percent, gs - sb, gs - sb + k);
    const uint32_t pa = (uint32_t)(gs - sa);
    const uint32_t pbf = (uint32_t)(gs - sb);
    std::vector<std::string> front;
    for (size_t i = 0; i < nfront; ++i) front.push_back(random_read(1 + rnd() % 9));      // every byte phase of the reads against the aligned words
    if (!o) check_pair(front, a, bf, pa, pbf, k, 0, match, mismatch, xdrop);
    else check_pair(front, a, revcomp(bf), pa, (uint32_t)(lb - pbf - k), k, 1, match, mismatch, xdrop);
}

int main()
{
    // windows: reads of every length 1 .. 70 behind 0 .. 3 bytes of other reads, ending in the block's last byte
    for (size_t len = 1; len <= 70; ++len)
        for (size_t phase = 0; phase < 4; ++phase) {
            std::vector<std::string> reads;
            if (phase) reads.push_back(random_read(4 * phase - (rnd() % 4)));
            reads.push_back(random_read(len));
            check_windows(reads);
        }
    { std::vector<std::string> reads = {random_read(13), random_read(333)}; check_windows(reads); }

    // the step: every start column mod 32, spans around the window sizes, the parameters' edges
    const uint32_t totals[] = {1, 2, 31, 32, 33, 63, 64, 65, 100, 257};
    const int64_t scores[][3] = {{1, 1, 7}, {1, 1, 0}, {2, 3, 5}, {1, 0, 3}, {5, 0, 0}, {1 << 15, 1 << 15, 0x7fffffff}, {1 << 15, 1 << 15, 1 << 15}, {1, 1 << 15, 1 << 15}, {3, 1, 1}};
    for (uint32_t total : totals)
        for (uint32_t first_n = 1; first_n <= 32; ++first_n)
            for (const auto &sc : scores)
                for (uint32_t density : {0u, 3u, 20u, 50u, 100u}) check_step(total, density, sc[0], sc[1], sc[2], first_n);
    {   // a drop of exactly xdrop goes on, xdrop + 1 stops: match 1, mismatch 2, xdrop 6 -- three mismatches in a row drop 6, a fourth 8
        XdSide st;
        bool d = xd_step(st, 0x15ULL << 4, 8, 0, 1, 2, 6);      // M M X X X M M M
        CHECK(!d && st.best == 2 && st.len == 2 && st.s == -1 && st.mm == 0 && st.seen == 3, "a drop of exactly xdrop goes on (s %lld best %lld)", (long long)st.s, (long long)st.best);
        XdSide s2;
        d = xd_step(s2, 0x15ULL << 4, 8, 0, 1, 2, 5);
        CHECK(d && s2.best == 2 && s2.len == 2 && s2.seen == 3, "a drop of xdrop + 1 stops at the third mismatch");
        XdSide s3;                                           // the 64-bit score: 2^15 x 2^17 columns
        for (uint32_t c0 = 0; c0 < (1u << 17); c0 += 32) (void)xd_step(s3, 0, 32, c0, 1 << 15, 1 << 15, 0);
        CHECK(s3.best == (1LL << 32) && s3.len == (1u << 17), "a score of 2^32");
    }

    // walks: overlaps of reads cut from a genome, both orientations, seeds flush with a read's start or end, K of one, two and three words
    const std::string g = random_read(3000);
    const int ks[] = {31, 51, 77, 3};
    for (int k : ks) {
        for (int o = 0; o < 2; ++o) {
            for (uint32_t percent : {0u, 3u, 15u}) {
                for (int it = 0; it < 60; ++it) {
                    const size_t la = k + rnd() % 400, lb = k + rnd() % 400;
                    const size_t gs = 500 + rnd() % 1500;                  // the seed
                    const size_t sa = gs - std::min<size_t>(rnd() % (la - k + 1), gs), sb = gs - std::min<size_t>(rnd() % (lb - k + 1), gs);
                    check_overlap(g, sa, la, sb, lb, gs, k, o, percent, 1, 1, 7, it % 4);
                    check_overlap(g, sa, la, sb, lb, gs, k, o, percent, 2, 3, it % 2 ? 0 : 11, it % 4);
                }
                // flush: the seed is A's start, A's end, B's start, B's end, a whole read, both reads
                check_overlap(g, 700, 200, 600, 300, 700, k, o, percent, 1, 1, 7, 1);
                check_overlap(g, 700, 200, 800, 300, 900 - k, k, o, percent, 1, 1, 7, 2);
                check_overlap(g, 600, 300, 700, 200, 700, k, o, percent, 1, 1, 7, 3);
                check_overlap(g, 600, 300, 500, 200, 700 - k, k, o, percent, 1, 1, 7, 0);
                check_overlap(g, 600, 300, 700, k, 700, k, o, percent, 1, 1, 7, 1);
                check_overlap(g, 700, k, 700, k, 700, k, o, percent, 1, 1, 7, 2);
                for (size_t len : {31u + 0u, 32u, 33u, 63u, 64u, 65u, 95u, 96u, 97u})      // spans around the window sizes, from either end
                    if ((int)len >= k) {
                        check_overlap(g, 1000, len, 1000, len, 1000, k, o, percent, 1, 1, 7, 1);
                        check_overlap(g, 1000, len, 1000, len, 1000 + len - k, k, o, percent, 1, 1, 7, 3);
                        check_overlap(g, 1000, len + k, 1000, len + k, 1000 + len / 2, k, o, percent, 1, 1, 7, 2);
                    }
            }
        }
    }
    {   // a seed that is none, and an N against an A (the packed bytes hold N as A)
        std::string a = g.substr(100, 120), b = g.substr(100, 120);
        b[40] = b[40] == 'A' ? 'C' : 'A';
        check_pair({}, a, b, 30, 30, 31, 0, 1, 1, 7);
        std::string c = a; for (char &ch : c) if (ch == 'A') { ch = 'N'; break; }
        check_pair({}, a, c, 0, 0, 31, 0, 1, 1, 7);
    }
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK %llu windows, %llu step cases, %llu walks\n", (unsigned long long)g_windows, (unsigned long long)g_steps, (unsigned long long)g_walks);
    return 0;
}
