// hsk_pairplan.h -- slices of a task range's records for hsk_result_pairs_sliced (host: hsk_host_pairs.h; the kernel is at the end).
//
// pair_tsum_kernel gives entry e of the range its exclusive record offset off[e] (off[0] = 0, off[nent] = records).  A SLICE is a run
// of entries [from, e): its records are the window [off[from], off[e]) of the range's record array, expanded, sorted and reduced on its
// own.  The next cut behind `from` under a budget of max_records is
//     the largest e in (from, nent] with off[e] - off[from] <= max_records,      or from + 1 where there is none:
// an entry alone may hold more records than the budget (up to 2 147 385 345 of them), and is then a slice of its own.  The offsets do not
// fall, so the condition holds for a prefix of the candidates and the cut is found by steps of 1, 2, 4, ... and a bisection.  Entries without
// records (cnt == 1) repeat their successor's offset: "the largest e" takes a whole run of them along with the slice in front of it,
// wherever the run lies, so a run of any length costs no slice and no step.  The differences are taken, never off[from] + max_records:
// a budget near 2^64 does not wrap.
//
// No HIP in the planner: it runs on the CPU under the sanitizers (tests/pairplan_test.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define HSK_PP_FN __host__ __device__ inline
#else
#define HSK_PP_FN inline
#endif

namespace hsk {

// off[0 .. nent], from < nent  ->  the next cut: from < cut <= nent
HSK_PP_FN uint64_t pair_plan_next(const uint64_t *off, uint64_t nent, uint64_t from, uint64_t max_records)
{
    const uint64_t o0 = off[from];
    uint64_t lo = from, hi = nent + 1;                   // off[lo] - o0 <= max_records (0 at lo = from); hi: the first index known not to fit
    // steps of 1, 2, 4, ... from `from` first: a cut that lies d entries on costs ~2 log2(d) loads, not log2(nent) -- one lane walks all
    // cuts of a range (pair_plan_kernel), and with a small budget there are as many cuts as entries
    for (uint64_t step = 1; step <= nent - lo; step <<= 1) {
        if (off[lo + step] - o0 <= max_records) lo += step; else { hi = lo + step; break; }
        if (step >> 62) break;
    }
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] - o0 <= max_records) lo = mid; else hi = mid;
    }
    return lo > from ? lo : from + 1;
}

// All cuts of entries [0, nent) into cut[0 .. return): cut[i] is the END of slice i (slice i = [i ? cut[i - 1] : 0, cut[i])), the last
// one is nent.  Stops when `cap` cuts are written (the return value is then cap and cut[cap - 1] < nent: the caller's bound was too
// small).  Two neighbouring slices hold more than max_records records between them -- the first would have taken the second's first
// entry otherwise -- so there are at most 2 * (records / max_records) + 2 slices, and never more than nent.
HSK_PP_FN uint64_t pair_plan_all(const uint64_t *off, uint64_t nent, uint64_t max_records, uint64_t *cut, uint64_t cap)
{
    uint64_t n = 0, from = 0;
    while (from < nent && n < cap) { from = pair_plan_next(off, nent, from, max_records); cut[n++] = from; }
    return n;
}

// the bound above (max_records >= 1)
HSK_PP_FN uint64_t pair_plan_max_slices(uint64_t nent, uint64_t records, uint64_t max_records)
{
    const uint64_t q = records / max_records;
    const uint64_t b = q > (~0ULL - 2) / 2 ? ~0ULL : 2 * q + 2;
    return b < nent ? b : nent;
}

} // namespace hsk

#if defined(__HIPCC__)
#include "hsk_device.h"

namespace hsk {

// one lane: every cut of the range's entries under the budget, and the record offset at each cut
struct PairPlanArgs {
    const u64 *off; u64 nent, max_records;
    u64 *cut;                // cap pairs { cut, off[cut] }
    u64 cap;
    u64 *ncut;
};

__global__ void pair_plan_kernel(PairPlanArgs p)
{
    if (blockIdx.x || threadIdx.x) return;
    u64 n = 0, from = 0;
    while (from < p.nent && n < p.cap) {
        from = pair_plan_next(p.off, p.nent, from, p.max_records);
        p.cut[2 * n] = from; p.cut[2 * n + 1] = p.off[from];
        ++n;
    }
    p.ncut[0] = from < p.nent ? ~0ULL : n;               // (the bound of the cuts did not hold: never, by the argument above)
}

} // namespace hsk
#endif
