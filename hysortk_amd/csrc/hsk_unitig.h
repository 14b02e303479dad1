// hsk_unitig.h -- the unitigs of a list of string graph edges: the out-arcs of a vertex over its run of the sorted arc array (degree and
// representative), the link test, the state of one vertex during ranking and the step that doubles it, the canonical rule and the packers of
// the two kinds of rows (kernels: hsk_unitig_kernels.h; host: hsk_host_unitig.h; include/hsk.h: hsk_overlaps_unitigs has the definition this
// file is held to, word for word).  Vertices, arcs and the arc array are those of hsk_strgraph.h.
//
// RANKING.  Every vertex v holds a WINDOW: v and the `cnt` vertices in front of it along the links.  ptr is the vertex in front of the
// window (UT_NONE: the window starts at the head of v's path), sum the `len` of the cnt links inside the window and in front of v, minv
// the smallest vertex of the window, far its first vertex.  One step joins v's window with the window of ptr; after k steps a window holds
// 2^k links or reaches the head.  A vertex on a cycle never loses its pointer: once the windows hold the whole cycle, minv is the cycle's
// smallest vertex, every other word is thrown away, the cycle is cut in front of that vertex (ut_cut) and ranked once more as a path.
// The structure is complement-symmetric, so only this direction is ranked: what lies behind v in its chain is what lies in front of v ^ 1
// in the complement chain.
//
// No HIP in here: everything runs on the CPU under the sanitizers (tests/unitig_test.cpp).
#pragma once
#include <cstdint>
#include "hsk_strgraph.h"

namespace hsk {

// No vertex.  Vertices lie below 2 nreads <= 2^32, so only the call with nreads == 2^31 has a vertex of this value (read 2^31 - 1, reverse).
// That call asks for 104 bytes x 2^32 vertices of device memory before the first kernel that writes a pointer and ends as HSK_ERR_OOM:
// no state ever holds the last vertex.
constexpr uint32_t UT_NONE = 0xffffffffu;
constexpr uint64_t UT_NO_LINK = ~0ULL;                   // the link word of a path's last member

// out(v) from the records [lo, hi) of v: deg = the distinct w; of the FIRST distinct w -- the only one if deg == 1 -- the arc's
// representative: the record with the smallest len, then the smallest row, which is the smallest value
struct UtOut { uint32_t deg, w; uint64_t rep; };
HSK_SB_FN UtOut ut_out(const uint64_t *keys, const uint64_t *vals, uint64_t lo, uint64_t hi)
{
    UtOut o; o.deg = 0; o.w = UT_NONE; o.rep = UT_NO_LINK;
    for (uint64_t i = lo; i < hi; ++i) {
        if (i == lo || keys[i] != keys[i - 1]) { if (++o.deg == 1) { o.w = (uint32_t)keys[i]; o.rep = vals[i]; } }
        else if (o.deg == 1 && vals[i] < o.rep) o.rep = vals[i];
    }
    return o;
}

// is the arc v -> w a link?  (deg_wc: the degree of w ^ 1)
HSK_SB_FN bool ut_link(uint32_t deg_v, uint32_t deg_wc) { return deg_v == 1 && deg_wc == 1; }

// succ(v), or UT_NONE: deg and cand are ut_out's deg and w of every vertex
HSK_SB_FN uint32_t ut_succ(const uint32_t *deg, const uint32_t *cand, uint64_t nv, uint32_t v)
{
    if (deg[v] != 1) return UT_NONE;
    const uint32_t w = cand[v];
    return (uint64_t)(w ^ 1u) < nv && ut_link(1, deg[w ^ 1u]) ? w : UT_NONE;
}
// pred(v), or UT_NONE: the complement of succ(v ^ 1).  The link pred(v) -> v is represented by rep[pred(v)].
HSK_SB_FN uint32_t ut_pred(const uint32_t *deg, const uint32_t *cand, uint64_t nv, uint32_t v)
{
    const uint32_t x = ut_succ(deg, cand, nv, v ^ 1u);
    return x == UT_NONE ? UT_NONE : (x ^ 1u);
}

// 32 bytes per vertex, 16-byte aligned: two loads, two stores
struct alignas(16) UtState {
    uint64_t sum;                                        // the len of the links inside the window
    uint32_t ptr, cnt;                                   // the vertex in front of the window; the links inside it
    uint32_t minv, far;                                  // the window's smallest and first vertex
    uint32_t cyc, pad_;                                  // the smallest vertex of v's cycle once it is cut; UT_NONE on a path
};
static_assert(sizeof(UtState) == 32, "a round moves 32 bytes per vertex each way");

// the window of v before the first step: v, and the link from pred (UT_NONE: none) of plen bases
HSK_SB_FN UtState ut_init(uint32_t v, uint32_t pred, uint32_t plen)
{
    UtState s; s.ptr = pred; s.cnt = pred == UT_NONE ? 0u : 1u; s.sum = pred == UT_NONE ? 0u : plen; s.minv = s.far = v; s.cyc = UT_NONE; s.pad_ = 0;
    return s;
}

// one step: mine joined with theirs = the state of the vertex mine.ptr names (not read when mine.ptr is UT_NONE).  Sums of a cycle's
// windows may wrap: they are never used.
HSK_SB_FN UtState ut_step(const UtState &mine, const UtState &theirs)
{
    UtState s = mine;
    if (mine.ptr == UT_NONE) return s;
    s.ptr = theirs.ptr; s.cnt = mine.cnt + theirs.cnt; s.sum = mine.sum + theirs.sum;
    s.minv = theirs.minv < mine.minv ? theirs.minv : mine.minv; s.far = theirs.far;
    return s;
}

// steps after which every window of a graph of nreads reads has reached its head or holds its whole cycle: a chain has at most nreads
// vertices (never v and v ^ 1), so nreads - 1 links
HSK_SB_FN uint32_t ut_rounds(uint64_t nreads)
{
    uint32_t k = 0;
    while (k < 63 && (1ULL << k) < nreads) ++k;
    return k;
}

// behind the first phase: a vertex that still has a pointer lies on a cycle whose smallest vertex is its minv.  The cycle starts
// there: that vertex loses its pred, every other one starts again with the window ut_init gave it.
HSK_SB_FN UtState ut_cut(const UtState &s, uint32_t v, uint32_t pred, uint32_t plen)
{
    if (s.ptr == UT_NONE) return s;
    UtState c = ut_init(v, v == s.minv ? UT_NONE : pred, plen);
    c.cyc = s.minv;
    return c;
}

// Is the chain of v the unitig of its complement pair: is its smallest vertex even?  mine, comp: the final states of v and v ^ 1.  The
// vertices in front of v are mine's window, those behind it are the complements of comp's; the smaller READ of the two minima decides.
HSK_SB_FN bool ut_canonical(const UtState &mine, const UtState &comp)
{
    if (mine.cyc != UT_NONE) return (mine.cyc & 1u) == 0;
    return (mine.minv >> 1) <= (comp.minv >> 1) ? (mine.minv & 1u) == 0 : (comp.minv & 1u) == 1;
}

// the last vertex of the chain that starts at `head` (final states): on a path the complement of where head ^ 1 came from, on a cut
// cycle the pred of the head
HSK_SB_FN uint32_t ut_tail(const UtState &head_state, const UtState &head_comp, uint32_t pred_of_head)
{
    return head_state.cyc != UT_NONE ? pred_of_head : (head_comp.far ^ 1u);
}

// { unitig << 32 | rank, rid << 1 | s, offset, link }
HSK_SB_FN void ut_layout_row(uint64_t *row, uint64_t unitig, uint32_t rank, uint32_t v, int64_t rid_base, uint64_t offset, uint64_t link)
{
    row[0] = unitig << 32 | rank; row[1] = ((uint64_t)((int64_t)(v >> 1) + rid_base) << 1) | (v & 1u); row[2] = offset; row[3] = link;
}
// { first layout row, reads, bases, circular }: tail_offset and tail_len are the last member's offset and read length; back_len the len
// of a cycle's link back to rank 0
HSK_SB_FN void ut_unitig_row(uint64_t *row, uint64_t first, uint64_t reads, bool circular, uint64_t tail_offset, uint32_t tail_len, uint32_t back_len)
{
    row[0] = first; row[1] = reads; row[2] = tail_offset + (circular ? (uint64_t)back_len : (uint64_t)tail_len); row[3] = circular ? 1 : 0;
}

} // namespace hsk
