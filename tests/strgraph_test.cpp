// CPU exerciser of hysortk_amd/csrc/hsk_strgraph.h (the class of a row, the two arcs of a dovetail, the check against the lengths, the
// duplicate rule, the witness test, the search in the sorted arc array and the walk of one arc), built with -fsanitize=address,undefined by
// tests/test_strgraph.py.  Every array is a heap block of exactly its size, so a search that leaves its range is an AddressSanitizer
// report.  The steps of the kernels (hsk_reduce.h) are run one after the other on the header's functions and held to a brute-force
// reduction written here from the definition (include/hsk.h: hsk_overlaps_reduce): classes by the rules in their order, arcs by the table,
// duplicates by comparing all pairs, and the transitive test as three nested loops over the arc list.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../hysortk_amd/csrc/hsk_strgraph.h"

using namespace hsk;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }
static uint32_t rnd_in(uint32_t lo, uint32_t hi) { return lo + rnd() % (hi - lo + 1); }      // inclusive

struct Row { uint64_t w[6]; };
static Row make_row(uint32_t rid_a, uint32_t rid_b, uint32_t o, uint32_t a_lo, uint32_t a_hi, uint32_t b_lo, uint32_t b_hi, uint32_t la, uint32_t lb, uint64_t score)
{
    const uint64_t ends = (a_lo == 0 ? 1 : 0) | (a_hi == la ? 2 : 0) | (b_lo == 0 ? 4 : 0) | (b_hi == lb ? 8 : 0);
    Row r; r.w[0] = (uint64_t)o << 63 | (uint64_t)rid_a << 32 | rid_b; r.w[1] = score; r.w[2] = (uint64_t)a_lo << 32 | a_hi; r.w[3] = (uint64_t)b_lo << 32 | b_hi; r.w[4] = ends; r.w[5] = 1;
    return r;
}

// an exact-size heap copy of a vector: what the header's functions get to read
template <typename T> struct Heap {
    T *p; size_t n;
    explicit Heap(const std::vector<T> &v) : p((T *)std::malloc(v.size() ? v.size() * sizeof(T) : 1)), n(v.size()) { if (n) std::memcpy(p, v.data(), n * sizeof(T)); }
    ~Heap() { std::free(p); }
};

// ---- the definition, brute force ------------------------------------------------------------------------------------------------------------
struct BArc { uint32_t v, w; uint64_t len; size_t row; };

static std::vector<int> brute(const std::vector<Row> &rows, const std::vector<uint32_t> &lens, uint32_t fuzz, std::vector<bool> *contained_out, uint64_t *arcs_out)
{
    const size_t n = rows.size();
    std::vector<int> cls(n, -1);
    std::vector<bool> contained(lens.size(), false);
    auto o_of = [&](size_t i) { return (int)(rows[i].w[0] >> 63); };
    auto a_of = [&](size_t i) { return (uint32_t)((rows[i].w[0] >> 32) & 0x7fffffffu); };
    auto b_of = [&](size_t i) { return (uint32_t)rows[i].w[0]; };
    auto e_of = [&](size_t i) { return (int)(rows[i].w[4] & 15); };
    for (size_t i = 0; i < n; ++i) {
        const int o = o_of(i), e = e_of(i);
        if (a_of(i) == b_of(i)) cls[i] = 7;
        else if ((e & 1) && (e & 2)) { cls[i] = 3; contained[a_of(i)] = true; }
        else if ((e & 4) && (e & 8)) { cls[i] = 4; contained[b_of(i)] = true; }
        else if ((o == 0 && (e == 6 || e == 9)) || (o == 1 && (e == 10 || e == 5))) cls[i] = 0;
        else cls[i] = 2;
    }
    for (size_t i = 0; i < n; ++i) if (cls[i] == 0 && (contained[a_of(i)] || contained[b_of(i)])) cls[i] = 5;
    for (size_t i = 0; i < n; ++i) {
        if (cls[i] != 0 && cls[i] != 6) continue;
        for (size_t j = 0; j < n; ++j) {
            if (j == i || (cls[j] != 0 && cls[j] != 6) || rows[j].w[0] != rows[i].w[0] || e_of(j) != e_of(i)) continue;
            if (rows[j].w[1] > rows[i].w[1] || (rows[j].w[1] == rows[i].w[1] && j < i)) cls[i] = 6;
        }
    }
    std::vector<BArc> arcs;
    for (size_t i = 0; i < n; ++i) {
        if (cls[i] != 0) continue;
        const uint32_t a = a_of(i), b = b_of(i);
        const uint64_t la = lens[a], lb = lens[b], a_lo = rows[i].w[2] >> 32, a_hi = rows[i].w[2] & 0xffffffffu, b_lo = rows[i].w[3] >> 32, b_hi = rows[i].w[3] & 0xffffffffu;
        const int o = o_of(i), e = e_of(i);
        if (o == 0 && e == 6) { arcs.push_back({2 * a, 2 * b, a_lo, i}); arcs.push_back({2 * b + 1, 2 * a + 1, lb - b_hi, i}); }
        if (o == 0 && e == 9) { arcs.push_back({2 * b, 2 * a, b_lo, i}); arcs.push_back({2 * a + 1, 2 * b + 1, la - a_hi, i}); }
        if (o == 1 && e == 10) { arcs.push_back({2 * a, 2 * b + 1, a_lo, i}); arcs.push_back({2 * b, 2 * a + 1, b_lo, i}); }
        if (o == 1 && e == 5) { arcs.push_back({2 * b + 1, 2 * a, lb - b_hi, i}); arcs.push_back({2 * a + 1, 2 * b, la - a_hi, i}); }
    }
    std::vector<bool> red(n, false);
    for (const BArc &vx : arcs)
        for (const BArc &vw : arcs)
            for (const BArc &wx : arcs)
                if (vw.v == vx.v && wx.v == vw.w && wx.w == vx.w && vw.w / 2 != vx.v / 2 && vw.w / 2 != vx.w / 2 && vw.len + wx.len <= vx.len + (uint64_t)fuzz) red[vx.row] = true;
    for (size_t i = 0; i < n; ++i) if (red[i]) cls[i] = 1;
    *contained_out = contained; *arcs_out = arcs.size();
    return cls;
}

// ---- the kernels' steps on the header's functions -----------------------------------------------------------------------------------------
static std::vector<int> by_header(const std::vector<Row> &rows, const std::vector<uint32_t> &lens, uint32_t fuzz, std::vector<bool> *contained_out, uint64_t *arcs_out)
{
    const size_t n = rows.size();
    std::vector<int> cls(n, -1);
    std::vector<bool> contained(lens.size(), false);
    for (size_t i = 0; i < n; ++i) {
        const uint64_t key = rows[i].w[0];
        const uint32_t a = (uint32_t)((key >> 32) & 0x7fffffffu), b = (uint32_t)key, e = (uint32_t)rows[i].w[4] & 15u;
        CHECK(sg_consistent(e, lens[a], lens[b], sg_span(rows[i].w[2], rows[i].w[3])), "row %zu", i);
        cls[i] = sg_row_class((uint32_t)(key >> 63), e, a, b);
        if (cls[i] == SG_A_CONTAINED) contained[a] = true;
        if (cls[i] == SG_B_CONTAINED) contained[b] = true;
    }
    std::vector<std::pair<uint64_t, uint64_t>> rec;
    for (size_t i = 0; i < n; ++i) {
        if (cls[i] != SG_KEPT) continue;
        const uint64_t key = rows[i].w[0];
        const uint32_t a = (uint32_t)((key >> 32) & 0x7fffffffu), b = (uint32_t)key;
        if (contained[a] || contained[b]) { cls[i] = SG_DROPPED_READ; continue; }
        SgArc x, y;
        sg_arcs((uint32_t)(key >> 63), (uint32_t)rows[i].w[4] & 15u, a, b, lens[a], lens[b], sg_span(rows[i].w[2], rows[i].w[3]), x, y);
        rec.push_back({sg_arc_key(x.v, x.w), sg_arc_val(x.len, (uint32_t)i)}); rec.push_back({sg_arc_key(y.v, y.w), sg_arc_val(y.len, (uint32_t)i)});
    }
    std::stable_sort(rec.begin(), rec.end(), [](const std::pair<uint64_t, uint64_t> &p, const std::pair<uint64_t, uint64_t> &q) { return p.first < q.first; });
    std::vector<uint64_t> keys_v, vals_v;
    for (auto &r : rec) { keys_v.push_back(r.first); vals_v.push_back(r.second); }
    const size_t m = rec.size();
    std::vector<uint64_t> live_v(vals_v);
    uint64_t live = 0;
    for (size_t j = 0; j < m; ++j) {
        const size_t row = (size_t)(vals_v[j] & 0xffffffffu);
        bool lost = false;
        size_t h = j;
        while (h > 0 && keys_v[h - 1] == keys_v[j]) --h;
        for (size_t i = h; i < m && keys_v[i] == keys_v[j]; ++i) {
            const size_t ri = (size_t)(vals_v[i] & 0xffffffffu);
            if (i != j && rows[ri].w[0] == rows[row].w[0] && (rows[ri].w[4] & 15) == (rows[row].w[4] & 15) && sg_dup_beats(rows[ri].w[1], ri, rows[row].w[1], row)) lost = true;
        }
        if (lost) { live_v[j] = SG_DEAD; cls[row] = SG_DUPLICATE; } else ++live;
    }
    const Heap<uint64_t> keys(keys_v), vals(live_v);
    const uint64_t nv = 2 * lens.size();
    std::vector<uint64_t> off_v(nv + 1);
    for (uint64_t v = 0; v <= nv; ++v) off_v[v] = v == nv ? m : sg_lower_bound(keys.p, 0, m, v << 32);
    const Heap<uint64_t> off(off_v);
    for (size_t j = 0; j < m; ++j)
        if (sg_arc_transitive(keys.p, vals.p, off.p, j, fuzz)) cls[(size_t)(vals.p[j] & 0xffffffffu)] = SG_REDUCED;
    *contained_out = contained; *arcs_out = live;
    return cls;
}

static uint64_t g_graphs = 0, g_rows = 0, g_seen[8] = {0, 0, 0, 0, 0, 0, 0, 0};

// random rows on `nreads` reads: mostly dovetails of all four kinds, some doubled with other scores, some exchanged, a few contained,
// internal and self rows; `huge`: lengths next to 2^32, so that the sums need 64 bits
static void random_graph(uint32_t nreads, uint32_t nrows, bool huge, uint32_t fuzz)
{
    std::vector<uint32_t> lens(nreads);
    for (auto &l : lens) l = huge ? 0xffffffffu - rnd_in(0, 40) : rnd_in(30, 60);
    std::vector<Row> rows;
    while (rows.size() < nrows) {
        uint32_t a = rnd() % nreads, b = rnd() % nreads;
        const uint32_t what = rnd() % 40, o = rnd() & 1;
        if (what == 0) b = a;
        if (a == b && what != 0) continue;
        const uint32_t la = lens[a], lb = lens[b];
        // an inner coordinate: small or next to the read's length, so that arc lengths cover 0 .. 2^32 when the reads are huge
        auto inner = [&](uint32_t l) { return (rnd() & 1) ? rnd_in(1, 20) : l - rnd_in(1, 20); };
        Row r;
        if (what == 1) r = make_row(a, b, o, 0, la, rnd_in(0, 5), lb - rnd_in(0, 5), la, lb, rnd() % 4);                  // a contained (sometimes e == 15)
        else if (what == 2) r = make_row(a, b, o, rnd_in(1, 5), la - rnd_in(0, 5), 0, lb, la, lb, rnd() % 4);             // b contained
        else if (what == 3) r = make_row(a, b, o, rnd_in(1, 9), la - rnd_in(1, 9), rnd_in(0, 9), lb - rnd_in(1, 9), la, lb, rnd() % 4);      // internal
        else {
            const bool first = rnd() & 1;                 // a in front (a_hi == la) or behind (a_lo == 0)
            uint32_t a_lo = first ? inner(la) : 0, a_hi = first ? la : inner(la);
            uint32_t b_lo, b_hi;
            if ((o == 0) == first) { b_lo = 0; b_hi = inner(lb); } else { b_lo = inner(lb); b_hi = lb; }
            r = make_row(a, b, o, a_lo, a_hi, b_lo, b_hi, la, lb, rnd() % 4);
        }
        rows.push_back(r);
        if (rnd() % 6 == 0) { Row d = r; d.w[1] = rnd() % 4; rows.push_back(d); }                                            // doubled, any score
    }
    std::vector<bool> c1, c2; uint64_t n1 = 0, n2 = 0;
    const std::vector<int> want = brute(rows, lens, fuzz, &c1, &n1), got = by_header(rows, lens, fuzz, &c2, &n2);
    CHECK(c1 == c2 && n1 == n2, "contained reads or arcs differ (%llu, %llu arcs)", (unsigned long long)n1, (unsigned long long)n2);
    for (size_t i = 0; i < rows.size(); ++i) {
        CHECK(want[i] == got[i], "row %zu of %zu: class %d, the definition says %d (huge %d, fuzz %u)", i, rows.size(), got[i], want[i], (int)huge, fuzz);
        g_seen[want[i] & 7]++;
    }
    g_graphs++; g_rows += rows.size();
}

int main()
{
    // ---- the class of every (o, e) of the 2 x 16, with and without rid_a == rid_b -------------------------------------------------------
    for (uint32_t o = 0; o < 2; ++o)
        for (uint32_t e = 0; e < 16; ++e) {
            const bool dove = o == 0 ? (e == 6 || e == 9) : (e == 10 || e == 5);
            const int want = (e & 3) == 3 ? 3 : ((e & 12) == 12 ? 4 : (dove ? 0 : 2));
            CHECK(sg_row_class(o, e, 4, 9) == want, "o %u e %u", o, e);
            CHECK(sg_row_class(o, e, 9, 9) == 7, "o %u e %u self", o, e);
            CHECK(sg_dovetail(o, e) == dove, "o %u e %u", o, e);
        }
    CHECK(sg_row_class(0, 15, 1, 2) == SG_A_CONTAINED && sg_row_class(1, 15, 1, 2) == SG_A_CONTAINED, "e == 15 drops a");
    // ---- coordinates and ends bits against the lengths: every combination on two short reads ------------------------------------------------
    for (uint32_t la = 1; la <= 3; ++la) for (uint32_t lb = 1; lb <= 3; ++lb)
        for (uint32_t a_lo = 0; a_lo <= 4; ++a_lo) for (uint32_t a_hi = 0; a_hi <= 4; ++a_hi) for (uint32_t b_lo = 0; b_lo <= 4; ++b_lo) for (uint32_t b_hi = 0; b_hi <= 4; ++b_hi)
            for (uint32_t e = 0; e < 16; ++e) {
                bool ok = a_lo < a_hi && a_hi <= la && b_lo < b_hi && b_hi <= lb;
                ok = ok && ((e & 1) != 0) == (a_lo == 0) && ((e & 2) != 0) == (a_hi == la) && ((e & 4) != 0) == (b_lo == 0) && ((e & 8) != 0) == (b_hi == lb);
                SgSpan s; s.a_lo = a_lo; s.a_hi = a_hi; s.b_lo = b_lo; s.b_hi = b_hi;
                CHECK(sg_consistent(e, la, lb, s) == ok, "la %u lb %u [%u, %u) [%u, %u) e %u", la, lb, a_lo, a_hi, b_lo, b_hi, e);
            }
    {   // sg_span takes the words apart
        const SgSpan s = sg_span(0xfffffffe00000007ull, 0x00000003fffffffdull);
        CHECK(s.a_lo == 0xfffffffeu && s.a_hi == 7 && s.b_lo == 3 && s.b_hi == 0xfffffffdu, "sg_span");
    }
    // ---- the table of the arcs, with numbers ------------------------------------------------------------------------------------------------
    {
        SgArc x, y; SgSpan s;
        s.a_lo = 30; s.a_hi = 100; s.b_lo = 0; s.b_hi = 70;   sg_arcs(0, 6, 5, 8, 100, 90, s, x, y);
        CHECK(x.v == 10 && x.w == 16 && x.len == 30 && y.v == 17 && y.w == 11 && y.len == 20, "0, 6");
        s.a_lo = 0; s.a_hi = 70; s.b_lo = 25; s.b_hi = 90;    sg_arcs(0, 9, 5, 8, 100, 90, s, x, y);
        CHECK(x.v == 16 && x.w == 10 && x.len == 25 && y.v == 11 && y.w == 17 && y.len == 30, "0, 9");
        s.a_lo = 30; s.a_hi = 100; s.b_lo = 25; s.b_hi = 90;  sg_arcs(1, 10, 5, 8, 100, 90, s, x, y);
        CHECK(x.v == 10 && x.w == 17 && x.len == 30 && y.v == 16 && y.w == 11 && y.len == 25, "1, 10");
        s.a_lo = 0; s.a_hi = 70; s.b_lo = 0; s.b_hi = 70;     sg_arcs(1, 5, 5, 8, 100, 90, s, x, y);
        CHECK(x.v == 17 && x.w == 10 && x.len == 20 && y.v == 11 && y.w == 16 && y.len == 30, "1, 5");
        s.a_lo = 0xfffffff0u; s.a_hi = 0xffffffffu; s.b_lo = 0; s.b_hi = 15; sg_arcs(0, 6, 0x7fffffffu, 0x7ffffffeu, 0xffffffffu, 0xffffffffu, s, x, y);
        CHECK(x.v == 0xfffffffeu && x.w == 0xfffffffcu && x.len == 0xfffffff0u && y.v == 0xfffffffdu && y.w == 0xffffffffu && y.len == 0xfffffff0u, "the last read");
        CHECK(sg_arc_key(0xfffffffeu, 3) == 0xfffffffe00000003ull && sg_arc_val(0xffffffffu, 0xfffffffeu) == 0xfffffffffffffffeull && sg_arc_val(0xffffffffu, 0xfffffffeu) != SG_DEAD, "records");
    }
    // ---- the duplicate rule -------------------------------------------------------------------------------------------------------------------
    CHECK(sg_dup_beats(5, 9, 4, 1) && !sg_dup_beats(4, 1, 5, 9) && sg_dup_beats(5, 1, 5, 9) && !sg_dup_beats(5, 9, 5, 1) && !sg_dup_beats(5, 3, 5, 3), "sg_dup_beats");
    // ---- the witness: the reads of v and x do not count; the sum in 64 bits --------------------------------------------------------------------
    CHECK(sg_witness(0, 4, 8, 10, 10, 20, 0) && !sg_witness(0, 4, 8, 10, 11, 20, 0) && sg_witness(0, 4, 8, 10, 11, 20, 1), "the fuzz edge");
    CHECK(!sg_witness(0, 1, 8, 0, 0, 20, 0) && !sg_witness(0, 0, 8, 0, 0, 20, 0) && !sg_witness(0, 9, 8, 0, 0, 20, 0) && !sg_witness(0, 8, 8, 0, 0, 20, 0) && sg_witness(0, 10, 8, 0, 0, 20, 0), "a witness on v's or x's read");
    CHECK(!sg_witness(0, 4, 8, 0xfffffff0u, 0x20u, 0x0fu, 0), "a sum that wraps in 32 bits is no witness");
    CHECK(sg_witness(0, 4, 8, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu) && !sg_witness(0, 4, 8, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xfffffffeu), "L + fuzz in 64 bits");
    // ---- the search: runs of 0, 1 and 2 records, dead records, ranges of 0 records --------------------------------------------------------------
    {
        const std::vector<uint64_t> kv = {sg_arc_key(2, 5), sg_arc_key(2, 7), sg_arc_key(2, 7), sg_arc_key(2, 9), sg_arc_key(3, 1), sg_arc_key(3, 1), sg_arc_key(6, 0)};
        const std::vector<uint64_t> vv = {sg_arc_val(10, 0), sg_arc_val(30, 1), sg_arc_val(20, 2), SG_DEAD, SG_DEAD, sg_arc_val(7, 4), sg_arc_val(0, 5)};
        const Heap<uint64_t> k(kv), v(vv);
        CHECK(sg_lower_bound(k.p, 0, 7, 0) == 0 && sg_lower_bound(k.p, 0, 7, sg_arc_key(2, 7)) == 1 && sg_lower_bound(k.p, 0, 7, sg_arc_key(2, 8)) == 3 && sg_lower_bound(k.p, 0, 7, ~0ull) == 7, "sg_lower_bound");
        CHECK(sg_lower_bound(k.p, 3, 3, 0) == 3 && sg_lower_bound(k.p, 7, 7, 0) == 7 && sg_lower_bound(k.p, 2, 4, sg_arc_key(9, 9)) == 4, "empty and partial ranges");
        CHECK(!sg_search(k.p, v.p, 0, 4, 2, 6, ~0ull) && !sg_search(k.p, v.p, 0, 4, 2, 4, ~0ull) && !sg_search(k.p, v.p, 0, 4, 2, 10, ~0ull), "a run of 0 records");
        CHECK(sg_search(k.p, v.p, 0, 4, 2, 5, 10) && !sg_search(k.p, v.p, 0, 4, 2, 5, 9), "a run of 1 record");
        CHECK(sg_search(k.p, v.p, 0, 4, 2, 7, 20) && !sg_search(k.p, v.p, 0, 4, 2, 7, 19) && sg_search(k.p, v.p, 0, 4, 2, 7, 30), "a run of 2 records: the shorter arc is behind the longer one");
        CHECK(!sg_search(k.p, v.p, 0, 4, 2, 9, ~0ull), "a dead record");
        CHECK(sg_search(k.p, v.p, 4, 6, 3, 1, 7) && !sg_search(k.p, v.p, 4, 6, 3, 1, 6), "a dead record in front of a live one");
        CHECK(!sg_search(k.p, v.p, 4, 5, 3, 1, 7), "a range that ends inside the run");
        CHECK(sg_search(k.p, v.p, 6, 7, 6, 0, 0) && !sg_search(k.p, v.p, 7, 7, 6, 0, 0) && !sg_search(k.p, v.p, 6, 6, 6, 0, 0), "the last record; empty ranges");
    }
    // ---- whole graphs against the brute-force reduction ---------------------------------------------------------------------------------------
    for (int t = 0; t < 60; ++t) random_graph(6 + rnd() % 10, 20 + rnd() % 60, false, t % 3 == 0 ? 0 : rnd() % 25);
    for (int t = 0; t < 60; ++t) random_graph(4 + rnd() % 6, 20 + rnd() % 50, true, t % 4 == 0 ? 0xffffffffu : (t % 4 == 1 ? 0 : rnd()));
    for (int c = 0; c < 8; ++c) CHECK(g_seen[c] > 0, "class %d never occurred", c);
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK %llu graphs, %llu rows; rows per class:", (unsigned long long)g_graphs, (unsigned long long)g_rows);
    for (int c = 0; c < 8; ++c) std::printf(" %llu", (unsigned long long)g_seen[c]);
    std::printf("\n");
    return 0;
}
