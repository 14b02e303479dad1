// hsk_pool.h -- the device memory pool of a context.
//
// Device memory mapped for the FIRST time is what a process's first call pays for (the driver clears it: 17 - 60 ms per GB, tools/exp/
// malloc_cost.hip), and hysortk::kmer_count() is called once per process.  Rounds 1 - 3 kept freed blocks whole and handed one only to a
// request of nearly its size: a 10 Gbp call with 46 GB live at its peak had 89 GB mapped.  Now a freed block is a SEGMENT of the region it was
// allocated in: a request takes the smallest free segment that holds it and leaves the rest behind as a free segment of its own (best fit, split),
// a released segment joins its free neighbours of the same region (coalesce).  Regions go back to the runtime only when they are entirely free
// (trim: on an allocation failure, or when the context goes).
//
// Reuse is stream-ordered by convention (as before): whoever releases a block has enqueued its last user, whoever allocates one enqueues its
// first user on the same stream or behind an event.
//
// The backend (hipMalloc / hipFree) is a pair of function pointers so that the segment logic runs on the CPU against malloc (tests/test_pool.py).
//
// Red zones (tuning pool_redzone=<bytes>, test-size inputs only): a block is handed out with `redzone` bytes behind its requested size, from the
// first 16-byte boundary at or after it, filled with RZ_BYTE (be_fill, on the context's stream).  A released block is QUARANTINED -- neither free
// nor handed out again -- until flush(): a later block of the same call could otherwise legitimately write into the old zone.  check() compares
// the zones of every live and quarantined block with the pattern (be_check: one kernel) and names the allocation site of the first block whose
// zone was written; the entry points call it after their final sync, then flush().  A call's memory peak is then the sum of its allocations.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

struct DevPool {
    typedef int (*MallocFn)(void **, size_t);
    typedef int (*FreeFn)(void *);
    MallocFn be_malloc = nullptr; FreeFn be_free = nullptr;          // set by the owner before the first allocation (0: success)
    struct Zone { char *p; size_t bytes; };
    typedef void (*FillFn)(void *arg, void *p, size_t bytes);          // fill [p, p + bytes) with RZ_BYTE
    typedef int (*CheckFn)(void *arg, const Zone *z, size_t n, size_t *bad_zone, size_t *bad_off);   // 0: every zone intact, 1: *bad_zone / *bad_off
                                                                                                       // name the first byte that is not (lowest zone, lowest offset), else: could not check
    FillFn be_fill = nullptr; CheckFn be_check = nullptr; void *be_arg = nullptr;                    // red zones (set with `redzone`)
    size_t redzone = 0;
    static constexpr unsigned char RZ_BYTE = 0xC5;
    static constexpr size_t ALIGN = 256;
    static constexpr size_t MIN_SPLIT = (size_t)1 << 20;             // a remainder below this stays with the block it was cut from

    struct Seg {
        size_t size; bool free; char *region;
        size_t req = 0, zoff = 0, zbytes = 0;                        // requested bytes; red zone [zoff, zoff + zbytes) (zbytes = 0: none)
        const char *file = nullptr; int line = 0;                    // allocation site
        bool quar = false;                                           // released, quarantined until flush()
        unsigned long long serial = 0;                               // when it was handed out (mark / rollback)
    };
    std::map<char *, Seg> segs;                                      // every segment, live or free, by address
    std::multimap<size_t, char *> free_by_size;
    std::map<char *, size_t> regions;                                // what the backend gave us
    size_t bytes_live = 0, bytes_cached = 0, peak = 0;
    unsigned long long serial = 0;                                   // blocks handed out so far

    void unlist(std::map<char *, Seg>::iterator it)
    {
        auto r = free_by_size.equal_range(it->second.size);
        for (auto q = r.first; q != r.second; ++q) if (q->second == it->first) { free_by_size.erase(q); break; }
    }
    // file / line: the allocation site (DALLOC passes its own; a direct call is tagged with the caller's)
    void *alloc(size_t bytes, const char *file = __builtin_FILE(), int line = __builtin_LINE())
    {
        const size_t req = bytes, zoff = (bytes + 15) & ~(size_t)15;
        char *p = (char *)alloc_seg(redzone ? zoff + redzone : bytes);
        if (!p) return nullptr;
        Seg &s = segs.find(p)->second;
        s.req = req; s.file = file; s.line = line;
        if (redzone) { s.zoff = zoff; s.zbytes = redzone; if (be_fill) be_fill(be_arg, p + zoff, redzone); }
        return p;
    }
    void *alloc_seg(size_t bytes)
    {
        if (bytes == 0) bytes = ALIGN;
        bytes = (bytes + ALIGN - 1) & ~(ALIGN - 1);
        auto f = free_by_size.lower_bound(bytes);
        if (f != free_by_size.end()) {
            auto it = segs.find(f->second);
            free_by_size.erase(f);
            Seg &s = it->second;
            bytes_cached -= s.size;
            if (s.size - bytes >= MIN_SPLIT) {                        // the rest stays behind as a free segment
                char *rest = it->first + bytes;
                const size_t rsz = s.size - bytes;
                s.size = bytes;
                segs[rest] = Seg{rsz, true, s.region};
                free_by_size.insert({rsz, rest});
                bytes_cached += rsz;
            }
            s.free = false; s.zbytes = 0; s.quar = false; s.serial = ++serial;
            bytes_live += s.size; peak = std::max(peak, bytes_live);
            return it->first;
        }
        void *p = nullptr;
        if (be_malloc(&p, bytes) != 0 || !p) {
            trim();
            p = nullptr;
            if (be_malloc(&p, bytes) != 0 || !p) return nullptr;
        }
        regions[(char *)p] = bytes;
        (segs[(char *)p] = Seg{bytes, false, (char *)p}).serial = ++serial;
        bytes_live += bytes; peak = std::max(peak, bytes_live);
        return p;
    }
    void release(void *p)
    {
        if (!p) return;
        auto it = segs.find((char *)p);
        if (it == segs.end() || it->second.free || it->second.quar) return;
        if (redzone) { it->second.quar = true; return; }
        release_seg(it);
    }
    void release_seg(std::map<char *, Seg>::iterator it)
    {
        it->second.quar = false; it->second.zbytes = 0;
        bytes_live -= it->second.size;
        it->second.free = true;
        // free neighbours of the same region join
        auto nx = std::next(it);
        if (nx != segs.end() && nx->second.free && nx->second.region == it->second.region && it->first + it->second.size == nx->first) {
            unlist(nx); bytes_cached -= nx->second.size;
            it->second.size += nx->second.size;
            segs.erase(nx);
        }
        if (it != segs.begin()) {
            auto pv = std::prev(it);
            if (pv->second.free && pv->second.region == it->second.region && pv->first + pv->second.size == it->first) {
                unlist(pv); bytes_cached -= pv->second.size;
                pv->second.size += it->second.size;
                segs.erase(it);
                it = pv;
            }
        }
        free_by_size.insert({it->second.size, it->first});
        bytes_cached += it->second.size;
    }
    // regions that are entirely free go back to the runtime
    void trim()
    {
        for (auto r = regions.begin(); r != regions.end();) {
            auto it = segs.find(r->first);
            if (it != segs.end() && it->second.free && it->second.size == r->second) {
                unlist(it); bytes_cached -= it->second.size;
                segs.erase(it);
                (void)be_free(r->first);
                r = regions.erase(r);
            } else ++r;
        }
    }
    void destroy()
    {
        for (auto &r : regions) (void)be_free(r.first);
        regions.clear(); segs.clear(); free_by_size.clear(); bytes_live = bytes_cached = 0;
    }
    // Error paths return early (DALLOC / HIPCHK) without releasing what they had allocated so far.  A call takes a mark when it
    // opens (ApiCall, hsk_api.hip); when it fails, rollback(mark) releases every block handed out since -- a block released and
    // handed out again at the same address included.  The blocks are free at once: whoever still holds a pointer into one (the
    // call's results) drops it before the rollback and never releases it afterwards.  Returns the number of blocks released.
    unsigned long long mark() const { return serial; }
    size_t rollback(unsigned long long m)
    {
        std::vector<char *> drop;
        for (auto &kv : segs) if (!kv.second.free && !kv.second.quar && kv.second.serial > m) drop.push_back(kv.first);
        for (char *p : drop) release(p);
        return drop.size();
    }
    // Red zones: 0 = every zone of a live or quarantined block holds the pattern, 1 = one does not (msg: the block's allocation site and the first
    // byte written, counted from the block's start), -1 = the check itself failed (msg says so).  The zones of live blocks are filled again after
    // a hit, so that the next call's check reports only what that call wrote.
    int check(char *msg, size_t cap)
    {
        if (msg && cap) msg[0] = 0;
        if (!redzone || !be_check) return 0;
        std::vector<Zone> z; std::vector<const Seg *> owner;
        for (auto &kv : segs) if (!kv.second.free && kv.second.zbytes) { z.push_back(Zone{kv.first + kv.second.zoff, kv.second.zbytes}); owner.push_back(&kv.second); }
        if (z.empty()) return 0;
        size_t bz = 0, bo = 0;
        const int r = be_check(be_arg, z.data(), z.size(), &bz, &bo);
        if (r == 0) return 0;
        if (r != 1 || bz >= z.size()) { if (msg) snprintf(msg, cap, "the red-zone check of %zu blocks could not run", z.size()); return -1; }
        const Seg &s = *owner[bz];
        const char *f = s.file ? s.file : "?"; if (const char *sl = strrchr(f, '/')) f = sl + 1;
        if (msg) snprintf(msg, cap, "a device write past the end of the block allocated at %s:%d (%zu bytes requested): byte %zu of the block was written",
                          f, s.line, s.req, s.zoff + bo);
        for (size_t i = 0; i < z.size(); ++i) if (be_fill) be_fill(be_arg, z[i].p, z[i].bytes);
        return 1;
    }
    // the quarantined blocks go back to the free lists (after check(), behind the call's last sync)
    void flush()
    {
        std::vector<char *> q;
        for (auto &kv : segs) if (kv.second.quar) q.push_back(kv.first);
        for (char *p : q) release_seg(segs.find(p));
    }
    size_t bytes_mapped() const { size_t s = 0; for (auto &r : regions) s += r.second; return s; }
};
