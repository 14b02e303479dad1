// hsk_chunks.h -- the chunk store: the output side of the expand fused with the first scatter pass (hsk_scatter.h) and of the
// combining extraction (hsk_combine.h).
//
// The digit histogram of the keys is not known before they exist, so a bin is not a pre-sized range but a LIST OF CHUNKS
// of CHUNK keys (= one tile of the second pass: 4096 one-word, 2048 two-word keys).  cursor[d] counts the keys reserved
// for digit d; a flush takes its range [p, p + c) with one atomic add; virtual chunk v = p / CHUNK of digit d lives in
// physical chunk map[d][v], allocated (bump counter) by the one reservation that contains the chunk's first slot and
// published through the map; everybody else whose range touches the chunk polls the map entry.  The allocator publishes
// before it waits for anything, so the wait is bounded by one L2 round trip (and by XS_SPIN_LIMIT: error word,
// HSK_ERR_INTERNAL).  A task wastes less than one chunk per digit: the chunk store holds n / CHUNK + 257 chunks.
//
// One task per XCD (HW_REG_XCC_ID, like onesweep_multi_kernel): cursors, map and chunk counter of a task are only ever
// touched from one XCD, so their atomics execute in that XCD's L2 (workgroup-scope RMW, L1-bypassing polls), and the
// short runs that neighbouring reservations of a digit write into the same 128-byte line merge in that L2 before they
// go to HBM.  The host checks afterwards that the cursors add up to the task's k-mer count.
//
// A writer reserves on the cursor itself (as early as it can: the round trip hides behind whatever it does next) and calls
// chunk_resolve for the range it got: {split, d0, d1, d2} per digit, from which chunk_slot gives every staged record its slot.
//
// No HIP in the address arithmetic (chunk_deltas, chunk_slot): it runs on the CPU under the sanitizers (tests/chunks_test.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HSK_CH_FN __host__ __device__ __forceinline__
#else
#define HSK_CH_FN inline
#endif

namespace hsk {

typedef uint64_t u64;
typedef uint32_t u32;
#if !defined(__HIPCC__)
struct uint4 { u32 x, y, z, w; };
inline uint4 make_uint4(u32 x, u32 y, u32 z, u32 w) { return uint4{x, y, z, w}; }
#endif

constexpr int XS_SPAN = 3;                            // chunks one reservation can touch
constexpr u32 XS_SPIN_LIMIT = 1u << 22;

// A reservation of a digit: its records are slots [st, st + c) of the flush's sorted order, its range starts off0 slots into a chunk and
// touches the physical chunks ph[0 .. XS_SPAN) (numbered from 1; 0: not touched).  -> {split, d0, d1, d2}: slot i goes to record
// i + d0 (i < split: the first chunk), i + d1 (i < split + CHUNK), else i + d2 of the store.
template <int CHUNK>
HSK_CH_FN uint4 chunk_deltas(u32 st, u32 off0, const u32 (&ph)[XS_SPAN])
{
    const u32 split = st + ((u32)CHUNK - off0);           // first slot (in the sorted order of the flush) in the second chunk
    return make_uint4(split, (ph[0] - 1) * (u32)CHUNK + off0 - st, ((ph[1] ? ph[1] : 1u) - 1) * (u32)CHUNK - split,
                      ((ph[2] ? ph[2] : 1u) - 1) * (u32)CHUNK - (split + (u32)CHUNK));
}
template <int CHUNK>
HSK_CH_FN u32 chunk_slot(const uint4 &dl, u32 i)
{
    return i + (i < dl.x ? dl.y : (i < dl.x + (u32)CHUNK ? dl.z : dl.w));   // (mod 2^32)
}

struct ChunkStore {
    u64 *chunks, *vchunks;     // chunk store (records of NW words); EXTENSION / combining extraction: payload chunk store (same slots as `chunks`)
    u64 *cursor;               // [256] keys reserved per digit (zeroed)
    u32 *map;                  // [256][vmax] physical chunk + 1 (zeroed)
    u32 *ctl;                  // [0] tile / bucket ticket, [1] chunks handed out (zeroed)
    u32 vmax;                  // map entries per digit (n / CHUNK + 1)
    u32 cap_chunks;            // combining extraction: chunks the pair stores hold; the one behind them takes what does not fit (error bit 512: the host runs the call again
                               // with stores sized for the k-mers -- they are sized for the pairs the call's sketch of the input promises, four times over)
    u64 *ghist;                // [256] histogram of the second pass's digit (zeroed)
};

#if defined(__HIPCC__)
typedef __attribute__((address_space(1))) u32 G32;

// The lane of digit `digit` has reserved [p, p + c), c > 0, on s.cursor[digit]; its records are slots [st, st + c) of the flush.
// GUARD: the store may be full (s.cap_chunks; error bit 512).
template <int CHUNK, bool GUARD>
__device__ __forceinline__ uint4 chunk_resolve(const ChunkStore &s, u32 digit, u64 p, u32 c, u32 st, u32 *err)
{
    const u64 v0 = p / CHUNK;
    const u32 off0 = (u32)(p % CHUNK);
    const u32 nv = (off0 + c - 1) / CHUNK + 1;             // chunks touched
    G32 *mp = (G32 *)(s.map + (u64)digit * s.vmax);
    u32 ph[XS_SPAN] = {0, 0, 0};
    // the chunks whose first slot is mine are allocated and published before anything is waited for
#pragma unroll
    for (int q = 0; q < XS_SPAN; ++q) {
        if ((u32)q >= nv || (q == 0 && off0 != 0)) continue;
        ph[q] = __hip_atomic_fetch_add(&s.ctl[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) + 1;
        if (GUARD) { if (ph[q] > s.cap_chunks) { ph[q] = s.cap_chunks + 1u; atomicOr(err, 512u); } }
        __hip_atomic_store(mp + v0 + q, ph[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (off0 != 0) {                                      // the chunk my range starts in was opened by another reservation
        u32 spins = 0;
        while ((ph[0] = __hip_atomic_load(mp + v0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0) {
            if (++spins > XS_SPIN_LIMIT) { atomicOr(err, 2u); ph[0] = 1; break; }
            __builtin_amdgcn_s_sleep(1);
        }
    }
    return chunk_deltas<CHUNK>(st, off0, ph);
}
#endif

} // namespace hsk
