// hsk_gapped.h -- banded, gapped x-drop extension of a seed of two reads, antidiagonal by antidiagonal (kernel: hsk_extend_gapped.h; host:
// hsk_host_extend.h; include/hsk.h: hsk_pair_diags_extend_gapped has the definition this file is held to, word for word).
//
// A SIDE walks two base sequences x (from A) and y (from B) away from the seed, indices from 1: gp_lengths gives their lengths na and nb,
// gp_x32 / gp_y32 the 32 bases x_i .. x_i+31 / y_j .. y_j+31 as a 64-bit word with the first in the top bits, on top of xd_bases and
// strand_rev2 (hsk_xdrop.h, hsk_strandbits.h: no byte at or beyond `nbytes` is read; bases outside 1 .. na are whatever lies there).
// A CELL (i, j) lies on diagonal k = i - j and antidiagonal d = i + j.  A live cell is a pair (s, e), score and edits, held as ONE signed
// 64-bit word s * 2^32 + (2^32 - 1 - e) (gp_pack): the larger word is the better pair -- larger s first, then smaller e -- so the cell's
// choice among its candidates is a maximum, and a candidate is one addition (gp_score: + match * 2^32; - mismatch * 2^32 - 1; - gap * 2^32 - 1).
// A dead cell is GP_DEAD, so far below zero that a candidate made from it stays below GP_LIVE.  |s| < 2^30 (la + lb < 2^22, scores up to 255)
// and e < 2^22: the halves never borrow from each other.
// gp_cell is the recurrence with the x-drop test; gp_take the best cell of an antidiagonal (cells offered with i ascending: the smallest i
// wins a tie); gp_raise the strict raise of the side's best; gp_row the overlap's row.  gp_side walks one side serially, one cell at a
// time with every base fetched on its own: the CPU's form of what a lane group of the kernel does.
//
// No HIP in here: everything runs on the CPU under the sanitizers (tests/gapped_test.cpp).
#pragma once
#include <cstdint>
#include "hsk_xdrop.h"

namespace hsk {

constexpr int GP_MAX_BAND = 63;
constexpr uint64_t GP_MAX_SPAN = 1ULL << 22;             // la + lb at or above it: the row is refused (a 32-bit score is exact below)
constexpr int64_t GP_DEAD = -(1LL << 62);
constexpr int64_t GP_LIVE = -(1LL << 61);                // v > GP_LIVE: a live cell

struct GpScore {
    int64_t match_add, mis_sub, gap_sub;                 // what a candidate adds to / takes from its predecessor's word
    int32_t xdrop, band;
};

HSK_SB_FN GpScore gp_score(int64_t match, int64_t mismatch, int64_t gap, uint32_t xdrop, uint32_t band)
{
    GpScore sc;
    sc.match_add = match * (1LL << 32); sc.mis_sub = mismatch * (1LL << 32) + 1; sc.gap_sub = gap * (1LL << 32) + 1;
    sc.xdrop = (int32_t)xdrop; sc.band = (int32_t)band;
    return sc;
}

HSK_SB_FN int64_t gp_pack(int32_t s, uint32_t e) { return (int64_t)s * (1LL << 32) + (int64_t)(0xffffffffu - e); }
HSK_SB_FN int32_t gp_s(int64_t v) { return (int32_t)(v >> 32); }
HSK_SB_FN uint32_t gp_e(int64_t v) { return 0xffffffffu - (uint32_t)(uint64_t)v; }

// the side's lengths (the table of include/hsk.h); the seed fits its reads
HSK_SB_FN void gp_lengths(const XdPair &p, bool right, uint32_t &na, uint32_t &nb)
{
    const uint32_t k = (uint32_t)p.k;
    na = right ? p.la - p.pa - k : p.pa;
    nb = right != (p.o != 0) ? p.lb - p.pb - k : p.pb;
}

// x_i .. x_i+31 (right: A[pa + K - 1 + i] onwards; left: A[pa - i] backwards); any i
HSK_SB_FN uint64_t gp_x32(const uint8_t *packed, uint64_t nbytes, const XdPair &p, bool right, int64_t i)
{
    if (right) return xd_bases(packed, nbytes, p.bit_a, (int64_t)p.pa + p.k - 1 + i);
    return strand_rev2(xd_bases(packed, nbytes, p.bit_a, (int64_t)p.pa - i - 31));
}

// y_j .. y_j+31 (B[pb + K - 1 + j] onwards for the right side of o = 0 and the left side of o = 1, B[pb - j] backwards for the other two;
// o = 1: the complement); any j
HSK_SB_FN uint64_t gp_y32(const uint8_t *packed, uint64_t nbytes, const XdPair &p, bool right, int64_t j)
{
    const bool onwards = right != (p.o != 0);
    const uint64_t w = onwards ? xd_bases(packed, nbytes, p.bit_b, (int64_t)p.pb + p.k - 1 + j) : strand_rev2(xd_bases(packed, nbytes, p.bit_b, (int64_t)p.pb - j - 31));
    return p.o ? ~w : w;
}

// Cell (i, j) from its predecessors' words: diag = (i-1, j-1), up = (i-1, j), left = (i, j-1), each GP_DEAD if dead or not there; eq: x_i == y_j;
// exists: the cell lies inside the reads and the band; best: the side's best over the antidiagonals in front of the cell's.
HSK_SB_FN int64_t gp_cell(int64_t diag, int64_t up, int64_t left, bool eq, bool exists, int32_t best, const GpScore &sc)
{
    int64_t c = eq ? diag + sc.match_add : diag - sc.mis_sub;
    const int64_t g = (up > left ? up : left) - sc.gap_sub;
    if (g > c) c = g;
    const bool live = exists && c > GP_LIVE && best - gp_s(c) <= sc.xdrop;
    return live ? c : GP_DEAD;
}

// the best cell of an antidiagonal so far is (v, i): cell (w, iw) with iw > i is offered
HSK_SB_FN void gp_take(int64_t &v, uint32_t &i, int64_t w, uint32_t iw)
{
    if (w > v) { v = w; i = iw; }
}

// one side of the extension
struct GpSide {
    int32_t  best = 0;
    uint32_t i = 0, j = 0, e = 0;                        // the cell that raised `best` last, and its edits
    uint64_t cells = 0;                                  // live cells on antidiagonals d >= 1
};

// after antidiagonal d, whose best live cell is (v, i) (GP_DEAD: none)
HSK_SB_FN void gp_raise(GpSide &st, int64_t v, uint32_t i, uint32_t d)
{
    if (v > GP_LIVE && gp_s(v) > st.best) { st.best = gp_s(v); st.i = i; st.j = d - i; st.e = gp_e(v); }
}

// The overlap's row from the two sides
HSK_SB_FN void gp_row(const XdPair &p, uint64_t key, uint64_t support, int64_t match, const GpSide &left, const GpSide &right, uint64_t (&row)[XD_ROW_WORDS])
{
    const uint64_t a_lo = (uint64_t)p.pa - left.i, a_hi = (uint64_t)p.pa + (uint64_t)p.k + right.i;
    const uint64_t b_lo = (uint64_t)p.pb - (p.o ? right.j : left.j), b_hi = (uint64_t)p.pb + (uint64_t)p.k + (p.o ? left.j : right.j);
    const uint64_t ends = (a_lo == 0 ? 1u : 0u) | (a_hi == p.la ? 2u : 0u) | (b_lo == 0 ? 4u : 0u) | (b_hi == p.lb ? 8u : 0u);
    row[0] = key;
    row[1] = (uint64_t)((int64_t)p.k * match + right.best + left.best);
    row[2] = a_lo << 32 | a_hi;
    row[3] = b_lo << 32 | b_hi;
    row[4] = (uint64_t)(left.e + right.e) << 32 | ends;
    row[5] = support;
}

// One side, serially: the diagonals -band .. band as three arrays (this antidiagonal and the two in front of it).
HSK_SB_FN GpSide gp_side(const uint8_t *packed, uint64_t nbytes, const XdPair &p, bool right, const GpScore &sc)
{
    constexpr int W = 2 * GP_MAX_BAND + 3;               // diagonal k at index k + band + 1; a dead border on either side
    int64_t cur[W], prev[W], prev2[W];
    for (int t = 0; t < W; ++t) cur[t] = prev[t] = prev2[t] = GP_DEAD;
    uint32_t na, nb;
    gp_lengths(p, right, na, nb);
    const int64_t band = sc.band, dmax = (int64_t)na + nb;
    GpSide st;
    prev[band + 1] = gp_pack(0, 0);                      // antidiagonal 0
    int dead = 0;
    for (int64_t d = 1; d <= dmax && dead < 2; ++d) {
        int64_t bv = GP_DEAD; uint32_t bi = 0;
        bool any = false;
        for (int64_t k = -band; k <= band; ++k) {
            const int t = (int)(k + band + 1);
            cur[t] = GP_DEAD;
            if ((d + k) & 1) continue;
            const int64_t i = (d + k) / 2, j = (d - k) / 2;
            if (d + k < 0 || d - k < 0 || i > (int64_t)na || j > (int64_t)nb) continue;
            const bool eq = i >= 1 && j >= 1 && (gp_x32(packed, nbytes, p, right, i) >> 62) == (gp_y32(packed, nbytes, p, right, j) >> 62);
            cur[t] = gp_cell(prev2[t], prev[t - 1], prev[t + 1], eq, true, st.best, sc);
            if (cur[t] > GP_LIVE) { any = true; ++st.cells; gp_take(bv, bi, cur[t], (uint32_t)i); }
        }
        gp_raise(st, bv, bi, (uint32_t)d);
        dead = any ? 0 : dead + 1;
        for (int t = 0; t < W; ++t) { prev2[t] = prev[t]; prev[t] = cur[t]; }
    }
    return st;
}

} // namespace hsk
