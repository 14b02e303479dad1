// CPU exerciser of hysortk_amd/csrc/hsk_gapped.h (the base accessors of the four sides, the cell with the packed (score, edits) pair, the
// best rule of an antidiagonal, the serial walk of a side and the overlap row), built with -fsanitize=address,undefined by
// tests/test_gapped.py.  Every packed buffer is a heap block of exactly the bytes the reads take, so a load that touches a byte behind the
// last read's last base is an AddressSanitizer report.  Everything is held to a plain full-matrix DP on strings, written here from the
// definition (include/hsk.h: hsk_pair_diags_extend_gapped) with (score, edits) as two numbers and the candidates as a list.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../hysortk_amd/csrc/hsk_gapped.h"

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
        p = (uint8_t *)std::malloc(nbytes ? nbytes : 1);
        std::memset(p, 0, nbytes);
        for (size_t k = 0; k < reads.size(); ++k)
            for (size_t i = 0; i < reads[k].size(); ++i) p[off[k] + i / 4] |= (uint8_t)(code(reads[k][i]) << (6 - 2 * (i % 4)));
    }
    ~Packed() { std::free(p); }
};

static uint64_t g_sides = 0, g_rows = 0, g_bases = 0;

struct Score { int64_t match, mismatch, gap, xdrop; int band; };
struct RefSide { int64_t best = 0; int64_t i = 0, j = 0, e = 0; uint64_t cells = 0; };

// ---- the definition on code vectors: x[0] is x_1.  The whole (na + 1) x (nb + 1) matrix, walked by antidiagonals ----------------------------
static RefSide ref_side(const std::vector<int> &x, const std::vector<int> &y, const Score &sc)
{
    const int64_t na = (int64_t)x.size(), nb = (int64_t)y.size();
    struct Cell { bool live = false; int64_t s = 0, e = 0; };
    std::vector<Cell> m((size_t)((na + 1) * (nb + 1)));
    auto at = [&](int64_t i, int64_t j) -> Cell & { return m[(size_t)(i * (nb + 1) + j)]; };
    auto better = [](const Cell &a, const Cell &b) { return a.s > b.s || (a.s == b.s && a.e < b.e); };
    at(0, 0).live = true;
    RefSide r;
    int dead = 0;
    for (int64_t d = 1; d <= na + nb && dead < 2; ++d) {
        Cell top; int64_t top_i = 0;
        for (int64_t i = std::max<int64_t>(0, d - nb); i <= std::min(na, d); ++i) {
            const int64_t j = d - i;
            if (std::llabs(i - j) > sc.band) continue;
            Cell cands[3]; int nc = 0;
            if (i >= 1 && j >= 1 && at(i - 1, j - 1).live) {
                Cell c = at(i - 1, j - 1);
                if (x[(size_t)i - 1] == y[(size_t)j - 1]) c.s += sc.match; else { c.s -= sc.mismatch; ++c.e; }
                cands[nc++] = c;
            }
            if (i >= 1 && at(i - 1, j).live) { Cell c = at(i - 1, j); c.s -= sc.gap; ++c.e; cands[nc++] = c; }
            if (j >= 1 && at(i, j - 1).live) { Cell c = at(i, j - 1); c.s -= sc.gap; ++c.e; cands[nc++] = c; }
            if (!nc) continue;
            Cell c = cands[0];
            for (int t = 1; t < nc; ++t) if (better(cands[t], c)) c = cands[t];
            if (r.best - c.s > sc.xdrop) continue;
            at(i, j) = c;
            ++r.cells;
            if (!top.live || better(c, top)) { top = c; top_i = i; }       // (i ascends: a tie keeps the smaller i)
        }
        if (top.live && top.s > r.best) { r.best = top.s; r.i = top_i; r.j = d - top_i; r.e = top.e; }
        dead = top.live ? 0 : dead + 1;
    }
    return r;
}

static std::vector<int> codes_of(const std::string &s, bool reverse, bool comp, size_t cap = ~(size_t)0)
{
    std::vector<int> v;
    for (size_t t = 0; t < s.size() && t < cap; ++t) { const int b = code(reverse ? s[s.size() - 1 - t] : s[t]); v.push_back(comp ? 3 - b : b); }
    return v;
}

// the table of include/hsk.h on strings; cap: no more than this many bases of a side (a walk that is known to stop before)
static void ref_xy(const std::string &a, const std::string &b, size_t pa, size_t pb, size_t k, int o, bool right, std::vector<int> &x, std::vector<int> &y, size_t cap = ~(size_t)0)
{
    if (right) { x = codes_of(a.substr(pa + k), false, false, cap); y = o ? codes_of(b.substr(0, pb), true, true, cap) : codes_of(b.substr(pb + k), false, false, cap); }
    else { x = codes_of(a.substr(0, pa), true, false, cap); y = o ? codes_of(b.substr(pb + k), false, true, cap) : codes_of(b.substr(0, pb), true, false, cap); }
}

// one row of reads[ia], reads[ib] against the reference: the accessors base by base, both sides, the row
static void check_row(const std::vector<std::string> &reads, const Packed &pk, size_t ia, size_t ib, size_t pa, size_t pb, int k, int o, const Score &sc, bool bases, size_t cap = ~(size_t)0)
{
    const std::string &a = reads[ia], &b = reads[ib];
    XdPair p; std::memset(&p, 0, sizeof p);
    p.bit_a = 8 * pk.off[ia]; p.bit_b = 8 * pk.off[ib]; p.pa = (uint32_t)pa; p.pb = (uint32_t)pb; p.la = (uint32_t)a.size(); p.lb = (uint32_t)b.size(); p.k = k; p.o = o;
    CHECK(xd_seed_matches(pk.p, pk.nbytes, p), "the seed (%zu, %zu) o %d k %d", pa, pb, o, k);
    const GpScore gs = gp_score(sc.match, sc.mismatch, sc.gap, (uint32_t)sc.xdrop, (uint32_t)sc.band);
    GpSide side[2]; RefSide ref[2];
    for (int r = 0; r < 2; ++r) {
        const bool right = r == 0;
        std::vector<int> x, y;
        ref_xy(a, b, pa, pb, (size_t)k, o, right, x, y, cap);
        uint32_t na, nb;
        gp_lengths(p, right, na, nb);
        if (cap == ~(size_t)0) CHECK(na == x.size() && nb == y.size(), "lengths of the %s side: %u %u, the strings have %zu %zu", right ? "right" : "left", na, nb, x.size(), y.size());
        if (bases) {                                     // every base of the side, as the first of its 32 and as a later one; and the indices around the ends
            for (int64_t i = -40; i <= (int64_t)na + 40; ++i) {
                const uint64_t w = gp_x32(pk.p, pk.nbytes, p, right, i);
                for (int t = 0; t < 32; t += (t == 0 ? 13 : 18)) if (i + t >= 1 && i + t <= (int64_t)na) { CHECK((int)((w >> (62 - 2 * t)) & 3) == x[(size_t)(i + t - 1)], "x_%lld from %lld", (long long)(i + t), (long long)i); ++g_bases; }
            }
            for (int64_t j = -40; j <= (int64_t)nb + 40; ++j) {
                const uint64_t w = gp_y32(pk.p, pk.nbytes, p, right, j);
                for (int t = 0; t < 32; t += (t == 0 ? 13 : 18)) if (j + t >= 1 && j + t <= (int64_t)nb) { CHECK((int)((w >> (62 - 2 * t)) & 3) == y[(size_t)(j + t - 1)], "y_%lld from %lld", (long long)(j + t), (long long)j); ++g_bases; }
            }
        }
        side[r] = gp_side(pk.p, pk.nbytes, p, right, gs);
        ref[r] = ref_side(x, y, sc);
        CHECK(side[r].best == ref[r].best && side[r].i == ref[r].i && side[r].j == ref[r].j && side[r].e == ref[r].e && side[r].cells == ref[r].cells,
              "%s side of (%zu, %zu) o %d k %d band %d scores %lld %lld %lld xdrop %lld: (%d, %u, %u, %u, %llu), the matrix has (%lld, %lld, %lld, %lld, %llu)", right ? "right" : "left", pa, pb, o, k, sc.band,
              (long long)sc.match, (long long)sc.mismatch, (long long)sc.gap, (long long)sc.xdrop, side[r].best, side[r].i, side[r].j, side[r].e, (unsigned long long)side[r].cells,
              (long long)ref[r].best, (long long)ref[r].i, (long long)ref[r].j, (long long)ref[r].e, (unsigned long long)ref[r].cells);
        ++g_sides;
    }
    uint64_t row[XD_ROW_WORDS];
    gp_row(p, 0x8000000100000002ULL, 77, sc.match, side[1], side[0], row);
    const int64_t a_lo = (int64_t)pa - ref[1].i, a_hi = (int64_t)pa + k + ref[0].i;
    const int64_t b_lo = (int64_t)pb - (o ? ref[0].j : ref[1].j), b_hi = (int64_t)pb + k + (o ? ref[1].j : ref[0].j);
    const uint64_t ends = (a_lo == 0) | (a_hi == (int64_t)a.size()) << 1 | (b_lo == 0) << 2 | (b_hi == (int64_t)b.size()) << 3;
    CHECK(row[0] == 0x8000000100000002ULL && row[5] == 77 && row[1] == (uint64_t)(k * sc.match + ref[0].best + ref[1].best), "key, support, score %llu", (unsigned long long)row[1]);
    CHECK(row[2] == ((uint64_t)a_lo << 32 | (uint64_t)a_hi) && row[3] == ((uint64_t)b_lo << 32 | (uint64_t)b_hi), "coordinates of (%zu, %zu) o %d", pa, pb, o);
    CHECK(row[4] == ((uint64_t)(ref[0].e + ref[1].e) << 32 | ends), "edits and ends of (%zu, %zu) o %d", pa, pb, o);
    CHECK(a_lo >= 0 && b_lo >= 0 && a_hi <= (int64_t)a.size() && b_hi <= (int64_t)b.size(), "inside the reads");
    ++g_rows;
}

// a copy with substitutions and indels outside [keep0, keep1)
static std::string noisy(const std::string &s, size_t keep0, size_t keep1, uint32_t sub_pm, uint32_t indel_pm)
{
    std::string r;
    for (size_t t = 0; t < s.size(); ++t) {
        const uint32_t u = rnd() % 1000;
        if (t >= keep0 && t < keep1) { r.push_back(s[t]); continue; }
        if (u < indel_pm / 2) continue;
        if (u < indel_pm) r.push_back("ACGT"[rnd() & 3]);
        r.push_back(u < indel_pm + sub_pm ? "ACGT"[(code(s[t]) + 1 + rnd() % 3) & 3] : s[t]);
    }
    return r;
}

// overlaps cut from a genome: the two reads in front of the block's last bytes, behind filler reads that set the byte phase
static void check_overlaps(int k, int o, const Score &sc, size_t filler, bool bases)
{
    const std::string g = random_read(420);
    const size_t sa = rnd() % 40, sb = rnd() % 40, gs = 150 + rnd() % 60;         // the seed's place in the genome
    const size_t ea = 330 + rnd() % 80, eb = 330 + rnd() % 80;
    // each read has its own noise and the seed as it is; the indels in front of the seed move it, so a read is built in three parts
    const std::string left_a = noisy(g.substr(sa, gs - sa), 0, 0, 30, 20), left_b = noisy(g.substr(sb, gs - sb), 0, 0, 30, 20);
    const std::string seed = g.substr(gs, (size_t)k);
    const std::string ra = left_a + seed + noisy(g.substr(gs + k, ea - gs - k), 0, 0, 30, 20);
    const std::string fb = left_b + seed + noisy(g.substr(gs + k, eb - gs - k), 0, 0, 30, 20);
    const std::string rb = o ? revcomp(fb) : fb;
    const size_t pb = o ? fb.size() - left_b.size() - (size_t)k : left_b.size();
    const std::vector<std::string> reads = {random_read(filler), ra, rb};
    const Packed pk(reads);
    check_row(reads, pk, 1, 2, left_a.size(), pb, k, o, sc, bases);
    check_row(reads, pk, 2, 1, pb, left_a.size(), k, o, sc, bases);              // B's bases from the block's end as x
}

int main()
{
    const int bands[] = {0, 1, 7, 8, 63};
    const int ks[] = {3, 31, 51, 77};
    // every K, band, orientation and byte phase; the accessors base by base on the first score set
    for (int k : ks)
        for (int band : bands)
            for (int o = 0; o < 2; ++o)
                for (size_t filler = 0; filler < 4; ++filler) {
                    check_overlaps(k, o, Score{1, 1, 1, 7, band}, filler, band == 7);
                    check_overlaps(k, o, Score{2, 3, 1, 5, band}, filler, false);
                    check_overlaps(k, o, Score{1, 0, 1, 2, band}, filler, false);      // mismatch 0
                    check_overlaps(k, o, Score{3, 2, 0, 4, band}, filler, false);      // gap 0
                    check_overlaps(k, o, Score{1, 0, 0, 0, band}, filler, false);      // both, xdrop 0: nothing ever drops
                    check_overlaps(k, o, Score{1, 1, 1, 0, band}, filler, false);      // xdrop 0: the first edit ends a side
                }
    // every seed offset of short reads (K = 3): all base offsets and byte phases of both reads, seeds flush with a read's start and end
    for (int o = 0; o < 2; ++o)
        for (size_t la = 3; la <= 22; ++la) {
            const std::string a = random_read(la);
            for (size_t pa = 0; pa + 3 <= la; ++pa) {
                const size_t before = rnd() % 9, after = rnd() % 9;
                std::string fb = random_read(before) + a.substr(pa, 3) + random_read(after);
                // half of the time B continues A around the seed, so that the walks go somewhere
                if (rnd() & 1) { const size_t l = std::min(before, pa), r = std::min(after, la - pa - 3); fb = random_read(before - l) + a.substr(pa - l, l + 3 + r) + random_read(after - r); }
                const std::string b = o ? revcomp(fb) : fb;
                const size_t pb = o ? after : before;
                const std::vector<std::string> reads = {random_read(la % 5), a, b};
                const Packed pk(reads);
                check_row(reads, pk, 1, 2, pa, pb, 3, o, Score{1, 1, 1, 3, (int)(la % 4)}, true);
                check_row(reads, pk, 2, 1, pb, pa, 3, o, Score{1, 1, 1, 3, 2}, true);
            }
        }
    // a drop of exactly xdrop goes on, of xdrop + 1 stops: ten matching bases, a burst of substitutions, forty matching bases.  The diagonal
    // crosses a burst of 3 in every band, so the side reaches the reads' ends with at least 47 - 3; what a wider band finds by chance beside
    // the diagonal is the matrix's to say.  Band 0 has the diagonal alone: a burst of 4 ends the side behind the ten.
    for (int burst = 3; burst <= 4; ++burst)
        for (int band : bands) {
            const std::string seed = random_read(31), tail = random_read(50);
            std::string other = tail;
            for (int t = 10; t < 10 + burst; ++t) other[(size_t)t] = "ACGT"[(code(tail[(size_t)t]) + 2) & 3];
            const std::vector<std::string> reads = {seed + tail, seed + other};
            const Packed pk(reads);
            const Score sc{1, 1, 1, 3, band};
            check_row(reads, pk, 0, 1, 0, 0, 31, 0, sc, false);
            XdPair p; std::memset(&p, 0, sizeof p);
            p.bit_a = 8 * pk.off[0]; p.bit_b = 8 * pk.off[1]; p.la = p.lb = 81; p.k = 31;
            const GpSide s = gp_side(pk.p, pk.nbytes, p, true, gp_score(1, 1, 1, 3, (uint32_t)band));
            if (burst == 3) CHECK(s.best >= 47 - 3 && s.i == 50 && s.j == 50 && (band != 0 || (s.best == 44 && s.e == 3)), "a burst of 3 under xdrop 3, band %d: (%d, %u, %u, %u)", band, s.best, s.i, s.j, s.e);
            else if (band == 0) CHECK(s.best == 10 && s.i == 10 && s.j == 10 && s.e == 0, "a burst of 4 under xdrop 3, band %d: (%d, %u, %u, %u)", band, s.best, s.i, s.j, s.e);
        }
    // the score range: match = mismatch = gap = 255 and la + lb = 2^22 - 1.  The reads share 300 bases around the seed and nothing else, so
    // the walks are short and the matrix is cut at 600 bases a side
    {
        const size_t la = (1u << 21) - 1, lb = 1u << 21, pa = la / 2 + 1, pb = 777777;
        std::string a = random_read(la), b = random_read(lb);
        for (size_t t = 0; t < 300; ++t) b[pb - 120 + t] = a[pa - 120 + t];
        b[pb + 100] = "ACGT"[(code(b[pb + 100]) + 1) & 3];
        const std::vector<std::string> reads = {a, b};
        const Packed pk(reads);
        for (int band : {0, 15, 63}) check_row(reads, pk, 0, 1, pa, pb, 51, 0, Score{255, 255, 255, 255 * 4, band}, false, 600);
        XdPair p; std::memset(&p, 0, sizeof p);
        p.bit_a = 0; p.bit_b = 8 * pk.off[1]; p.pa = (uint32_t)pa; p.pb = (uint32_t)pb; p.la = (uint32_t)la; p.lb = (uint32_t)lb; p.k = 51;
        CHECK((uint64_t)p.la + p.lb == GP_MAX_SPAN - 1, "just under the limit");
        const GpSide s = gp_side(pk.p, pk.nbytes, p, true, gp_score(255, 255, 255, 255 * 4, 15));
        CHECK(s.best >= 255 * (129 - 1 - 2) && s.cells < 600 * 31, "the right side of the long reads: best %d, %llu cells", s.best, (unsigned long long)s.cells);
        CHECK(gp_s(gp_pack(-(1 << 30), 1u << 22)) == -(1 << 30) && gp_e(gp_pack(-(1 << 30), 1u << 22)) == 1u << 22 && gp_s(gp_pack((1 << 30), 0)) == 1 << 30, "the packed pair at its ends");
    }
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK %llu sides, %llu rows, %llu bases\n", (unsigned long long)g_sides, (unsigned long long)g_rows, (unsigned long long)g_bases);
    return 0;
}
