// hsk_strgraph.h -- the string graph of a list of overlap rows: the class of a row, the two arcs of a dovetail, the check of a row against
// the reads' lengths, the duplicate rule, the witness test and the search of an arc in the sorted arc array (kernels: hsk_reduce.h; host:
// hsk_host_reduce.h; include/hsk.h: hsk_overlaps_reduce has the definition this file is held to, word for word).
//
// A VERTEX is an oriented read, v = 2 r + s (s = 1: the reverse complement; v ^ 1 is the complement).  An ARC v -> w says that a suffix of
// v overlaps a prefix of w; its length is the number of bases of v in front of the overlap.  The ARC ARRAY holds one record per arc, sorted
// by key = v << 32 | w, with value = len << 32 | row; a record whose arc lost against a duplicate keeps its key (the searches stay binary)
// and has the value SG_DEAD.  off[v] is the first record of vertex v (off[2 nreads] = the number of records), so out(v) = [off[v], off[v + 1]).
// Two rows with a and b exchanged can give the same arc twice: such records are no duplicates of each other, both stay in the graph, and
// every search walks the whole run of equal keys.
//
// No HIP in here: everything runs on the CPU under the sanitizers (tests/strgraph_test.cpp).
#pragma once
#include <cstdint>
#include "hsk_strandbits.h"

namespace hsk {

// the class byte of a row; REDUCED is KEPT with bit 0 set
enum { SG_KEPT = 0, SG_REDUCED = 1, SG_INTERNAL = 2, SG_A_CONTAINED = 3, SG_B_CONTAINED = 4, SG_DROPPED_READ = 5, SG_DUPLICATE = 6, SG_SELF = 7, SG_CLASSES = 8 };
constexpr uint64_t SG_DEAD = ~0ULL;                     // the value of a record whose arc is out (no row has index 2^32 - 1)

struct SgSpan { uint32_t a_lo, a_hi, b_lo, b_hi; };      // words 2 and 3 of a row
struct SgArc { uint32_t v, w, len; };

HSK_SB_FN SgSpan sg_span(uint64_t word2, uint64_t word3)
{
    SgSpan s; s.a_lo = (uint32_t)(word2 >> 32); s.a_hi = (uint32_t)word2; s.b_lo = (uint32_t)(word3 >> 32); s.b_hi = (uint32_t)word3;
    return s;
}

HSK_SB_FN bool sg_dovetail(uint32_t o, uint32_t e) { return o ? (e == 10 || e == 5) : (e == 6 || e == 9); }

// what a row is by itself (the first rule that applies): SELF, A_CONTAINED, B_CONTAINED, INTERNAL, or KEPT for a dovetail -- which the
// rules that need the whole list (DROPPED_READ, DUPLICATE, REDUCED) may still change
HSK_SB_FN int sg_row_class(uint32_t o, uint32_t e, uint64_t rid_a, uint64_t rid_b)
{
    if (rid_a == rid_b) return SG_SELF;
    if ((e & 3) == 3) return SG_A_CONTAINED;
    if ((e & 12) == 12) return SG_B_CONTAINED;
    return sg_dovetail(o, e) ? SG_KEPT : SG_INTERNAL;
}

// do the coordinates and the ends bits agree with the reads' lengths?
HSK_SB_FN bool sg_consistent(uint32_t e, uint32_t la, uint32_t lb, const SgSpan &s)
{
    if (!(s.a_lo < s.a_hi && s.a_hi <= la && s.b_lo < s.b_hi && s.b_hi <= lb)) return false;
    const uint32_t want = (s.a_lo == 0 ? 1u : 0u) | (s.a_hi == la ? 2u : 0u) | (s.b_lo == 0 ? 4u : 0u) | (s.b_hi == lb ? 8u : 0u);
    return e == want;
}

// the two arcs of a dovetail row (sg_dovetail(o, e)) of the reads a, b (indices from 0): complements of each other
HSK_SB_FN void sg_arcs(uint32_t o, uint32_t e, uint32_t a, uint32_t b, uint32_t la, uint32_t lb, const SgSpan &s, SgArc &x, SgArc &y)
{
    if (!o) {
        if (e == 6) { x.v = 2 * a; x.w = 2 * b; x.len = s.a_lo; y.v = 2 * b + 1; y.w = 2 * a + 1; y.len = lb - s.b_hi; }
        else { x.v = 2 * b; x.w = 2 * a; x.len = s.b_lo; y.v = 2 * a + 1; y.w = 2 * b + 1; y.len = la - s.a_hi; }
    } else {
        if (e == 10) { x.v = 2 * a; x.w = 2 * b + 1; x.len = s.a_lo; y.v = 2 * b; y.w = 2 * a + 1; y.len = s.b_lo; }
        else { x.v = 2 * b + 1; x.w = 2 * a; x.len = lb - s.b_hi; y.v = 2 * a + 1; y.w = 2 * b; y.len = la - s.a_hi; }
    }
}

HSK_SB_FN uint64_t sg_arc_key(uint32_t v, uint32_t w) { return (uint64_t)v << 32 | w; }
HSK_SB_FN uint64_t sg_arc_val(uint32_t len, uint32_t row) { return (uint64_t)len << 32 | row; }

// of two dovetail rows with equal (key, e): does the row with score sx and index ix stay in front of the one with sy, iy?
HSK_SB_FN bool sg_dup_beats(uint64_t sx, uint64_t ix, uint64_t sy, uint64_t iy) { return sx > sy || (sx == sy && ix < iy); }

// v -> w (len_vw) and w -> x (len_wx) explain v -> x (L)
HSK_SB_FN bool sg_witness(uint32_t v, uint32_t w, uint32_t x, uint32_t len_vw, uint32_t len_wx, uint32_t L, uint32_t fuzz)
{
    return (w >> 1) != (v >> 1) && (w >> 1) != (x >> 1) && (uint64_t)len_vw + (uint64_t)len_wx <= (uint64_t)L + (uint64_t)fuzz;
}

// the first record of [lo, hi) whose key is not below `key`; hi if there is none
HSK_SB_FN uint64_t sg_lower_bound(const uint64_t *keys, uint64_t lo, uint64_t hi, uint64_t key)
{
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// is there a live arc w -> x of at most `most` bases among the records [lo, hi) -- out(w), or any range of the array that holds its run?
HSK_SB_FN bool sg_search(const uint64_t *keys, const uint64_t *vals, uint64_t lo, uint64_t hi, uint32_t w, uint32_t x, uint64_t most)
{
    const uint64_t key = sg_arc_key(w, x);
    for (uint64_t i = sg_lower_bound(keys, lo, hi, key); i < hi && keys[i] == key; ++i)
        if (vals[i] != SG_DEAD && (vals[i] >> 32) <= most) return true;
    return false;
}

// Is the arc of record j transitive?  One walk over out(v): a w on v's or x's read, a dead record, and a w whose own length is already
// above L + fuzz are passed over; else (w, x) is searched in out(w); the first witness ends the walk.  (The lane path of the reduce kernel.)
HSK_SB_FN bool sg_arc_transitive(const uint64_t *keys, const uint64_t *vals, const uint64_t *off, uint64_t j, uint32_t fuzz)
{
    if (vals[j] == SG_DEAD) return false;
    const uint32_t v = (uint32_t)(keys[j] >> 32), x = (uint32_t)keys[j];
    const uint64_t reach = (vals[j] >> 32) + (uint64_t)fuzz;
    for (uint64_t i = off[v], end = off[(uint64_t)v + 1]; i < end; ++i) {
        const uint32_t w = (uint32_t)keys[i];
        const uint64_t len_vw = vals[i] >> 32;
        if (vals[i] == SG_DEAD || (w >> 1) == (v >> 1) || (w >> 1) == (x >> 1) || len_vw > reach) continue;
        if (sg_search(keys, vals, off[w], off[(uint64_t)w + 1], w, x, reach - len_vw)) return true;
    }
    return false;
}

} // namespace hsk
