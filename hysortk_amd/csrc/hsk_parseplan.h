// hsk_parseplan.h -- the shapes of the parse stage that host and kernels must agree on (kernels: hsk_parse.h; host: hsk_host_parse.h).
//
// The packed reads are one stream of 4 * packed_bytes base positions in tiles of PARSE_TILE.  A launch has nblocks <= PARSE_MAX_BLOCKS
// workgroups; workgroup b walks tiles_per_block consecutive tiles.  With slabs (the ingest from pinned host memory: the reads arrive slab by
// slab while the slabs before are hashed) it does so once per slab: inside slab s it owns
//     [s * slab_tiles + b * tiles_per_block, + tiles_per_block), cut at the slab's end  min((s + 1) * slab_tiles, ntiles)
// and with nslabs == 1 the one range [b * tiles_per_block, + tiles_per_block) cut at ntiles (slab_tiles is not used then).  scan_kernel,
// place_kernel, place_items_kernel and place_bytes_kernel compute exactly this from ParseArgs.
//
// Also here: the record capacity of a tile, and how many tiles one step of each placement kernel takes.
//
// No HIP in here: everything runs on the CPU under the sanitizers (tests/parseplan_test.cpp).
#pragma once
#include <algorithm>
#include <stdint.h>

namespace hsk {

typedef uint64_t u64;
typedef uint32_t u32;

constexpr int PARSE_TILE = 2048;                      // positions of a tile = 512 bytes (PARSE_THREADS lanes x PARSE_PPT positions, hsk_parse.h)
constexpr int PARSE_WORDS = PARSE_TILE / 16 + 12;     // 128 tile words + halo (K-1 <= 94 bases = 6 words) + overread
constexpr u32 PARSE_MAX_BLOCKS = 1024;                // workgroups of a parse launch at most: the rows of the COUNT matrix (ParseArgs::blk_cnt)
constexpr u32 SCAN_REC_CAP = 512;                     // default records kept per tile (expected ~270 at K=31, M=17)
constexpr u32 PLACE_MAX_REC = 8192;                   // place_kernel: records of one placement step (rec_cap * place_group) ...
constexpr u32 PLACE_MAX_TILES = 16;                   // ... and its tiles at most (a record's tile: 4 bits)
constexpr int PLACE_ITEM_THREADS = 1024;
#ifndef PLACE_ITEM_RPT
#define PLACE_ITEM_RPT 16
#endif
constexpr u32 PLACE_ITEM_REC = PLACE_ITEM_RPT * 1024;  // place_items_kernel: records of one step (rec_cap * place_group)
constexpr u32 PLACE_ITEM_TILES = PLACE_ITEM_REC / 512; // tiles per step at most
constexpr u32 PLACE_ITEM_WORDS = PLACE_ITEM_TILES * (PARSE_TILE / 16) + 8;      // their packed words + the reach of the last supermer's second word
constexpr int PLACE_BYTES_THREADS = 1024;
constexpr u32 PLACE_BYTES_REC = 8192;                  // place_bytes_kernel: records of one step (rec_cap * place_group)
constexpr u32 PLACE_BYTES_TILES = 16;                  // tiles per step at most (a record's tile: 4 bits)
constexpr u32 PLACE_BYTES_WORDS = PLACE_BYTES_TILES * (PARSE_TILE / 16) + 24;   // their packed words + the overhang of the last supermer (<= 222 bases) + overread
constexpr u64 SLAB_HEAD = 4096;                        // bytes at the start of an ingest slab that the scan of the slab before it reads (its last windows + the prefetch's reach)
static_assert(SLAB_HEAD >= (u64)(PARSE_WORDS - PARSE_TILE / 16) * 4, "a slab's scan reaches PARSE_WORDS - 128 words into the next slab");

struct ParseTiling { u64 ntiles; u32 nblocks, tiles_per_block, nslabs; u64 slab_tiles; };

// max_blocks: 0 = PARSE_MAX_BLOCKS (never more: the COUNT matrix has that many rows); nslabs_wanted > 1: slabs, if every workgroup gets
// a tile in each of them -- else one range per workgroup
inline ParseTiling parse_tiling(u64 packed_bytes, u32 max_blocks, u32 nslabs_wanted)
{
    ParseTiling t{};
    t.ntiles = (packed_bytes * 4 + PARSE_TILE - 1) / PARSE_TILE;
    t.nslabs = 1;
    if (t.ntiles == 0) return t;
    u32 nblocks = (u32)std::min<u64>(t.ntiles, max_blocks ? std::min(max_blocks, PARSE_MAX_BLOCKS) : PARSE_MAX_BLOCKS);
    if (nslabs_wanted > 1 && t.ntiles >= (u64)nblocks * nslabs_wanted) {
        const u64 per_slab = (t.ntiles + nslabs_wanted - 1) / nslabs_wanted;
        t.tiles_per_block = (u32)((per_slab + nblocks - 1) / nblocks);
        t.slab_tiles = (u64)t.tiles_per_block * nblocks;
        t.nslabs = (u32)((t.ntiles + t.slab_tiles - 1) / t.slab_tiles);
        t.nblocks = nblocks;
        return t;
    }
    t.tiles_per_block = (u32)((t.ntiles + nblocks - 1) / nblocks);
    t.nblocks = (u32)((t.ntiles + t.tiles_per_block - 1) / t.tiles_per_block);
    return t;
}

// the bytes of slab sl: [b0, b1), of which [b0, bh) is its head -- all the scan of the slab before it needs of it
struct SlabBytes { u64 b0, bh, b1; };
inline SlabBytes slab_bytes(const ParseTiling &t, u32 sl, u64 packed_bytes)
{
    const u64 per = t.nslabs > 1 ? t.slab_tiles * (PARSE_TILE / 4) : packed_bytes;
    SlabBytes s;
    s.b0 = std::min<u64>((u64)sl * per, packed_bytes); s.b1 = std::min<u64>(((u64)sl + 1) * per, packed_bytes);
    s.bh = std::min<u64>(s.b0 + SLAB_HEAD, s.b1);
    return s;
}

// Record slots per 2048-position tile.  A window of W k-mers starts a supermer every (W + 1) / 2 positions on random
// sequence (+ one per 128 positions and per read): 40 % head room, a power of two from SCAN_REC_CAP (W >= 12) to 2048
// (tiny windows); a tile that still overflows sends the parse through the general kernels.  forced: tuning "parse_rec_cap", 0 = none
inline u32 parse_rec_cap(int W, long long forced = 0)
{
    if (forced) return (u32)std::min<long long>(std::max<long long>(forced, 1), (long long)PLACE_MAX_REC);
    const u32 need = (u32)(1.4 * (2.0 * PARSE_TILE / (W + 1) + 40));
    u32 cap = SCAN_REC_CAP;
    while (cap < need && cap < 2048) cap <<= 1;
    return cap;
}

// tiles one step of a placement kernel takes together (ParseArgs::place_group): as many as its records and its tile bits hold
enum PlaceKind { PLACE_RECORDS = 0, PLACE_ITEMS = 1, PLACE_BYTES = 2 };      // place_kernel, place_items_kernel, place_bytes_kernel
constexpr u32 place_rec(PlaceKind kind) { return kind == PLACE_ITEMS ? PLACE_ITEM_REC : kind == PLACE_BYTES ? PLACE_BYTES_REC : PLACE_MAX_REC; }
constexpr u32 place_tiles(PlaceKind kind) { return kind == PLACE_ITEMS ? PLACE_ITEM_TILES : kind == PLACE_BYTES ? PLACE_BYTES_TILES : PLACE_MAX_TILES; }
inline u32 place_group(PlaceKind kind, u32 rec_cap) { return std::max<u32>(1, std::min<u32>(place_tiles(kind), place_rec(kind) / rec_cap)); }

} // namespace hsk
