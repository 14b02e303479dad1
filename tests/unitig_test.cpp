// CPU exerciser of hysortk_amd/csrc/hsk_unitig.h (the out-arcs of a vertex over its run of the sorted arc array, the link test, the state of a
// vertex and the step that doubles it, the cut of a cycle, the canonical rule and the row packers), built with -fsanitize=address,undefined
// by tests/test_unitig.py.  Every array is a heap block of exactly its size.  The steps of the kernels (hsk_unitig_kernels.h) are run one
// after the other on the header's functions -- the ranking as a host loop that applies ut_step round by round, reading one buffer and
// writing the other -- and held to a sequential walk written here from the definition (include/hsk.h: hsk_overlaps_unitigs) with maps: on
// lines and rings around the powers of two, and on random graphs with forks, joins, parallel arcs and contained reads.  The rounds must
// stay within 2 ceil(log2(2 nreads)) + 4.  (A ring of one read would be a SELF row, which the call refuses: the rings start at two.)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "../hysortk_amd/csrc/hsk_unitig.h"

using namespace hsk;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }
static uint32_t rnd_in(uint32_t lo, uint32_t hi) { return lo + rnd() % (hi - lo + 1); }      // inclusive

// an exact-size heap block: what the header's functions get to read and write
template <typename T> struct Heap {
    T *p; size_t n;
    explicit Heap(size_t n_) : p((T *)std::malloc(n_ ? n_ * sizeof(T) : 1)), n(n_) {}
    explicit Heap(const std::vector<T> &v) : Heap(v.size()) { if (n) std::memcpy(p, v.data(), n * sizeof(T)); }
    ~Heap() { std::free(p); }
    Heap(const Heap &) = delete;
};

struct Arc { uint32_t v, w, len, row; };
struct Graph {
    uint64_t nreads = 0, rows = 0;
    std::vector<uint32_t> rlen; std::vector<bool> contained; std::vector<Arc> arcs;
    // a row: the arc v -> w of len1 bases and its complement of len2
    void edge(uint32_t v, uint32_t w, uint32_t len1, uint32_t len2) { const uint32_t r = (uint32_t)rows++; arcs.push_back({v, w, len1, r}); arcs.push_back({w ^ 1u, v ^ 1u, len2, r}); }
};
struct Result { std::vector<uint64_t> layout, table; uint64_t rounds = 0; };

// ---- the definition, one link at a time -------------------------------------------------------------------------------------------------------
static Result walk(const Graph &g, int64_t rid_base)
{
    std::map<std::pair<uint32_t, uint32_t>, uint64_t> rep;
    for (const Arc &a : g.arcs) {
        const uint64_t val = (uint64_t)a.len << 32 | a.row;
        auto it = rep.find({a.v, a.w});
        if (it == rep.end()) rep[{a.v, a.w}] = val; else if (val < it->second) it->second = val;
    }
    std::map<uint32_t, std::set<uint32_t>> out;
    for (auto &kv : rep) out[kv.first.first].insert(kv.first.second);
    auto deg = [&](uint32_t v) { auto it = out.find(v); return it == out.end() ? (size_t)0 : it->second.size(); };
    std::map<uint32_t, uint32_t> succ, pred;
    for (auto &kv : out)
        if (kv.second.size() == 1) { const uint32_t w = *kv.second.begin(); if (deg(w ^ 1u) == 1) { succ[kv.first] = w; pred[w] = kv.first; } }
    std::set<uint32_t> seen;
    Result r;
    std::vector<std::pair<uint32_t, std::vector<uint32_t>>> chains; std::vector<bool> circ;
    for (uint32_t v = 0; v < 2 * g.nreads; ++v) {
        if (g.contained[v >> 1] || seen.count(v)) continue;
        CHECK((v & 1) == 0, "the first vertex of a pair of chains is odd: %u", v);
        uint32_t h = v; bool circular = false;
        while (pred.count(h)) { h = pred[h]; if (h == v) { circular = true; break; } }
        std::vector<uint32_t> chain{h};
        for (uint32_t x = h; succ.count(x) && succ[x] != h;) { x = succ[x]; chain.push_back(x); }
        for (uint32_t x : chain) { CHECK(!seen.count(x) && !seen.count(x ^ 1u), "vertex %u twice", x); seen.insert(x); seen.insert(x ^ 1u); }
        chains.push_back({h, chain}); circ.push_back(circular);
    }
    // (the heads come out in increasing order only per pair: order the unitigs by their first vertex)
    std::vector<size_t> order(chains.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return chains[x].first < chains[y].first; });
    for (size_t u = 0; u < order.size(); ++u) {
        const std::vector<uint32_t> &chain = chains[order[u]].second;
        const uint64_t first = r.layout.size() / 4;
        uint64_t offset = 0, last_offset = 0;
        for (size_t k = 0; k < chain.size(); ++k) {
            const uint32_t x = chain[k];
            const bool has = succ.count(x) != 0;
            const uint64_t link = has ? rep[{x, succ[x]}] : ~0ULL;
            r.layout.insert(r.layout.end(), {(uint64_t)u << 32 | k, ((uint64_t)((int64_t)(x >> 1) + rid_base) << 1) | (x & 1u), offset, link});
            last_offset = offset;
            if (has) offset += link >> 32;
        }
        const bool c = circ[order[u]];
        r.table.insert(r.table.end(), {first, (uint64_t)chain.size(), c ? offset : last_offset + g.rlen[chain.back() >> 1], c ? 1ULL : 0ULL});
    }
    return r;
}

// ---- the steps of the kernels on the header's functions -------------------------------------------------------------------------------------
static Result doubling(const Graph &g, int64_t rid_base)
{
    const uint64_t nv = 2 * g.nreads, narcs = g.arcs.size();
    std::vector<Arc> sorted = g.arcs;
    for (size_t i = sorted.size(); i > 1; --i) std::swap(sorted[i - 1], sorted[rnd() % i]);      // (the sort keeps no order among equal keys)
    std::stable_sort(sorted.begin(), sorted.end(), [](const Arc &x, const Arc &y) { return sg_arc_key(x.v, x.w) < sg_arc_key(y.v, y.w); });
    std::vector<uint64_t> kv, vv, ov(nv + 1);
    for (const Arc &a : sorted) { kv.push_back(sg_arc_key(a.v, a.w)); vv.push_back(sg_arc_val(a.len, a.row)); }
    Heap<uint64_t> keys(kv), vals(vv);
    for (uint64_t v = 0; v <= nv; ++v) ov[v] = v == nv ? narcs : sg_lower_bound(keys.p, 0, narcs, v << 32);
    Heap<uint64_t> off(ov), rep(nv);
    Heap<uint32_t> deg(nv), cand(nv), pred(nv), uid(nv);
    for (uint64_t v = 0; v < nv; ++v) { const UtOut o = ut_out(keys.p, vals.p, off.p[v], off.p[v + 1]); deg.p[v] = o.deg; cand.p[v] = o.w; rep.p[v] = o.rep; }
    Heap<UtState> sa(nv), sb(nv);
    for (uint64_t v = 0; v < nv; ++v) {
        const uint32_t p = ut_pred(deg.p, cand.p, nv, (uint32_t)v);
        pred.p[v] = p;
        sa.p[v] = ut_init((uint32_t)v, p, p == UT_NONE ? 0u : (uint32_t)(rep.p[p] >> 32));
    }
    UtState *cur = sa.p, *nxt = sb.p;
    Result r;
    const uint32_t steps = g.rows ? ut_rounds(std::min<uint64_t>(g.nreads, g.rows + 1)) : 0;
    for (int phase = 0; phase < 2 && steps; ++phase) {
        if (phase)
            for (uint64_t v = 0; v < nv; ++v) { const uint32_t p = pred.p[v]; cur[v] = ut_cut(cur[v], (uint32_t)v, p, p == UT_NONE ? 0u : (uint32_t)(rep.p[p] >> 32)); }
        for (uint32_t k = 0; k < steps; ++k, ++r.rounds) {
            for (uint64_t v = 0; v < nv; ++v) {
                const UtState mine = cur[v];
                nxt[v] = ut_step(mine, mine.ptr == UT_NONE ? mine : cur[mine.ptr]);
            }
            std::swap(cur, nxt);
        }
        if (!phase)                                       // behind the first phase every path is ranked, and a cycle knows its smallest vertex
            for (uint64_t v = 0; v < nv; ++v) if (cur[v].ptr != UT_NONE) CHECK(cur[cur[v].minv].minv == cur[v].minv && cur[v].minv <= v, "cycle of %llu", (unsigned long long)v);
    }
    for (uint64_t v = 0; v < nv; ++v) CHECK(cur[v].ptr == UT_NONE, "vertex %llu still has a pointer behind %llu rounds", (unsigned long long)v, (unsigned long long)r.rounds);
    // heads, their unitigs and first rows in the order of the vertices
    uint64_t nu = 0, nm = 0;
    std::vector<uint64_t> first(nv, 0);
    for (uint64_t v = 0; v < nv; ++v) {
        uid.p[v] = UT_NONE;
        if (g.contained[v >> 1] || cur[v].far != v || !ut_canonical(cur[v], cur[v ^ 1])) continue;      // a head is where its own window starts
        const uint32_t t = ut_tail(cur[v], cur[v ^ 1], pred.p[v]);
        const bool circular = cur[v].cyc != UT_NONE;
        uint64_t row[4];
        ut_unitig_row(row, nm, (uint64_t)cur[t].cnt + 1, circular, cur[t].sum, g.rlen[t >> 1], circular ? (uint32_t)(rep.p[pred.p[v]] >> 32) : 0u);
        r.table.insert(r.table.end(), row, row + 4);
        uid.p[v] = (uint32_t)nu++; first[v] = nm; nm += cur[t].cnt + 1;
    }
    r.layout.assign(nm * 4, 0xdeadbeefULL);
    for (uint64_t v = 0; v < nv; ++v) {
        if (g.contained[v >> 1]) continue;
        const UtState &s = cur[v];
        if (uid.p[s.far] == UT_NONE) { CHECK(uid.p[cur[v ^ 1].far] != UT_NONE, "neither chain of read %llu is a unitig", (unsigned long long)(v >> 1)); continue; }
        const uint64_t at = first[s.far] + s.cnt;
        CHECK(at < nm && r.layout[at * 4] == 0xdeadbeefULL, "layout row %llu twice or outside", (unsigned long long)at);
        if (at < nm) ut_layout_row(&r.layout[at * 4], uid.p[s.far], s.cnt, (uint32_t)v, rid_base, s.sum, ut_succ(deg.p, cand.p, nv, (uint32_t)v) == UT_NONE ? UT_NO_LINK : rep.p[v]);
    }
    return r;
}

static uint32_t log2_ceil(uint64_t x) { uint32_t k = 0; while ((1ULL << k) < x) ++k; return k; }

static void run(const Graph &g, const char *what, uint64_t size, int64_t rid_base = 0)
{
    const Result a = walk(g, rid_base), b = doubling(g, rid_base);
    CHECK(a.layout == b.layout, "%s %llu: the layout rows differ (%zu and %zu words)", what, (unsigned long long)size, a.layout.size(), b.layout.size());
    CHECK(a.table == b.table, "%s %llu: the unitig rows differ (%zu and %zu words)", what, (unsigned long long)size, a.table.size(), b.table.size());
    CHECK(b.rounds <= 2 * log2_ceil(2 * g.nreads) + 4, "%s %llu: %llu rounds", what, (unsigned long long)size, (unsigned long long)b.rounds);
    uint64_t live = 0;
    for (uint64_t r = 0; r < g.nreads; ++r) live += !g.contained[r];
    CHECK(a.layout.size() == 4 * live, "%s %llu: %zu members of %llu live reads", what, (unsigned long long)size, a.layout.size() / 4, (unsigned long long)live);
}

// n reads in a row (ring: and back to the first), each on a random strand, at random distances, numbered along the line or shuffled
static Graph chain_graph(uint32_t n, bool ring, bool shuffled, uint32_t len_lo, uint32_t len_hi)
{
    Graph g; g.nreads = n; g.contained.assign(n, false);
    std::vector<uint32_t> id(n), strand(n);
    for (uint32_t i = 0; i < n; ++i) { id[i] = i; strand[i] = rnd() & 1u; g.rlen.push_back(len_hi); }
    if (shuffled) for (uint32_t i = n; i > 1; --i) std::swap(id[i - 1], id[rnd() % i]);
    for (uint32_t i = 0; i + 1 < n + (ring ? 1u : 0u); ++i) {
        const uint32_t j = (i + 1) % n;
        g.edge(2 * id[i] + strand[i], 2 * id[j] + strand[j], rnd_in(len_lo, len_hi), rnd_in(len_lo, len_hi));
    }
    return g;
}

int main()
{
    // the rules by hand
    {
        const uint64_t k[5] = {sg_arc_key(4, 2), sg_arc_key(4, 2), sg_arc_key(4, 2), sg_arc_key(4, 9), sg_arc_key(6, 1)};
        const uint64_t v[5] = {sg_arc_val(40, 7), sg_arc_val(38, 9), sg_arc_val(38, 8), sg_arc_val(5, 0), sg_arc_val(1, 1)};
        Heap<uint64_t> keys(std::vector<uint64_t>(k, k + 5)), vals(std::vector<uint64_t>(v, v + 5));
        UtOut o = ut_out(keys.p, vals.p, 0, 3);
        CHECK(o.deg == 1 && o.w == 2 && o.rep == sg_arc_val(38, 8), "the smallest len, then the smallest row: %u %u %llx", o.deg, o.w, (unsigned long long)o.rep);
        o = ut_out(keys.p, vals.p, 0, 4);
        CHECK(o.deg == 2, "two targets: %u", o.deg);
        o = ut_out(keys.p, vals.p, 4, 4);
        CHECK(o.deg == 0 && o.w == UT_NONE, "no record: %u", o.deg);
        o = ut_out(keys.p, vals.p, 4, 5);
        CHECK(o.deg == 1 && o.w == 1 && o.rep == sg_arc_val(1, 1), "one record");
        CHECK(ut_link(1, 1) && !ut_link(2, 1) && !ut_link(1, 2) && !ut_link(0, 1) && !ut_link(1, 0), "the link test");
        CHECK(ut_rounds(0) == 0 && ut_rounds(1) == 0 && ut_rounds(2) == 1 && ut_rounds(3) == 2 && ut_rounds(1024) == 10 && ut_rounds(1025) == 11 && ut_rounds(1ULL << 31) == 31, "the rounds");
        UtState a = ut_init(8, 6, 10), b = ut_init(6, UT_NONE, 0);
        UtState s = ut_step(a, b);
        CHECK(s.ptr == UT_NONE && s.cnt == 1 && s.sum == 10 && s.minv == 6 && s.far == 6 && s.cyc == UT_NONE, "one step to the head");
        CHECK(ut_step(s, a).cnt == 1, "a window at its head stays");
        UtState big = ut_init(1, 0, 0xffffffffu), big2 = ut_init(0, 3, 0xffffffffu);
        CHECK(ut_step(big, big2).sum == 2 * 0xffffffffULL && ut_step(big, big2).cnt == 2 && ut_step(big, big2).ptr == 3, "sums in 64 bits");
        UtState cy = ut_init(9, 4, 7); cy.minv = 4;
        CHECK(ut_cut(cy, 9, 4, 7).cyc == 4 && ut_cut(cy, 9, 4, 7).ptr == 4 && ut_cut(cy, 9, 4, 7).minv == 9, "a cycle's vertex starts again");
        cy = ut_init(4, 9, 7);
        CHECK(ut_cut(cy, 4, 9, 7).ptr == UT_NONE && ut_cut(cy, 4, 9, 7).cnt == 0 && ut_cut(cy, 4, 9, 7).sum == 0 && ut_cut(cy, 4, 9, 7).cyc == 4, "the cycle is cut in front of its smallest vertex");
        UtState m = ut_init(7, UT_NONE, 0), c = ut_init(6, UT_NONE, 0);
        CHECK(!ut_canonical(m, c) && ut_canonical(c, m), "a read alone: the even vertex");
        m.minv = 5; c.minv = 2;                          // in front of v the smallest is 5 (read 2, reverse), behind it the complement of 2: 3 (read 1, reverse)
        CHECK(!ut_canonical(m, c), "read 1 is reverse in this chain");
        c.minv = 3;                                      // behind v: the complement of 3, vertex 2: read 1 forward
        CHECK(ut_canonical(m, c), "read 1 is forward in this chain");
        uint64_t row[4];
        ut_layout_row(row, 3, 5, 11, 7, 1ULL << 40, UT_NO_LINK);
        CHECK(row[0] == (3ULL << 32 | 5) && row[1] == ((5 + 7) << 1 | 1) && row[2] == 1ULL << 40 && row[3] == ~0ULL, "the layout row");
        ut_unitig_row(row, 9, 4, false, 1ULL << 33, 100, 55);
        CHECK(row[0] == 9 && row[1] == 4 && row[2] == (1ULL << 33) + 100 && row[3] == 0, "a path's row");
        ut_unitig_row(row, 9, 4, true, 1ULL << 33, 100, 55);
        CHECK(row[2] == (1ULL << 33) + 55 && row[3] == 1, "a cycle's row");
    }
    // lines and rings around the powers of two
    static const uint32_t sizes[] = {1, 2, 3, 63, 64, 65, 1023, 1024, 1025};
    for (uint32_t n : sizes)
        for (int shuffled = 0; shuffled < 2; ++shuffled) {
            run(chain_graph(n, false, shuffled != 0, 1, 300), shuffled ? "shuffled line" : "line", n, shuffled ? 7 : 0);
            if (n >= 2) run(chain_graph(n, true, shuffled != 0, 1, 300), shuffled ? "shuffled ring" : "ring", n);
        }
    run(chain_graph(3, false, false, 0xfffffff0u, 0xffffffffu), "line near 2^32", 3);
    run(chain_graph(3, true, true, 0xfffffff0u, 0xffffffffu), "ring near 2^32", 3);
    // random graphs: lines and rings side by side, then stray edges (forks and joins), parallel arcs and contained reads
    for (int t = 0; t < 400; ++t) {
        const uint32_t n = rnd_in(1, 60);
        Graph g; g.nreads = n; g.contained.assign(n, false);
        for (uint32_t i = 0; i < n; ++i) { g.rlen.push_back(rnd_in(50, 500)); g.contained[i] = rnd() % 8 == 0; }
        std::vector<uint32_t> live;
        for (uint32_t i = 0; i < n; ++i) if (!g.contained[i]) live.push_back(i);
        for (size_t i = live.size(); i > 1; --i) std::swap(live[i - 1], live[rnd() % i]);
        std::vector<uint32_t> strand(n);
        for (uint32_t i = 0; i < n; ++i) strand[i] = rnd() & 1u;
        for (size_t i = 0; i < live.size();) {          // pieces of 1 to 12 reads
            const size_t m = std::min<size_t>(live.size() - i, rnd_in(1, 12));
            for (size_t k = 0; k + 1 < m; ++k) g.edge(2 * live[i + k] + strand[live[i + k]], 2 * live[i + k + 1] + strand[live[i + k + 1]], rnd_in(1, 400), rnd_in(1, 400));
            if (m >= 2 && rnd() % 3 == 0) g.edge(2 * live[i + m - 1] + strand[live[i + m - 1]], 2 * live[i] + strand[live[i]], rnd_in(1, 400), rnd_in(1, 400));
            i += m;
        }
        if (live.size() >= 2) {
            for (uint32_t k = rnd_in(0, 3); k > 0; --k) {      // stray edges
                const uint32_t a = live[rnd() % live.size()], b = live[rnd() % live.size()];
                if (a != b) g.edge(2 * a + (rnd() & 1u), 2 * b + (rnd() & 1u), rnd_in(1, 400), rnd_in(1, 400));
            }
            for (uint32_t k = rnd_in(0, 3); k > 0 && !g.arcs.empty(); --k) {      // an arc and its complement once more, from a row of its own
                const Arc x = g.arcs[2 * (rnd() % (g.arcs.size() / 2))], y = g.arcs[2 * (x.row) + 1];
                g.edge(x.v, x.w, rnd() & 1u ? x.len : rnd_in(1, 400), rnd() & 1u ? y.len : rnd_in(1, 400));
            }
        }
        run(g, "random graph", (uint64_t)t, t % 5);
    }
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK\n");
    return 0;
}
