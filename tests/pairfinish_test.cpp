// CPU exerciser of hysortk_amd/csrc/hsk_pairrank.h (how pair_finish_kernel turns the {k-mer, count} pairs of one prefix bin into the bin's
// sorted, merged, filtered entries), built with -fsanitize=address,undefined by tests/test_pairfinish_plan.py.  A bin is run through the
// kernel's steps with the header's functions -- bucket, arrival index in any order the atomics may give, exclusive scan of the buckets, the
// walk over the pair's own bucket, rank, head, summed count, filter, the mask of kept heads and the slot from its popcounts -- and held to a
// brute-force answer: the keys sorted, equal keys' counts summed (32 bits), [L, U] applied to the sums.  Every pair must be accounted for
// exactly once: the ranks are a permutation in key order, and the heads' sums add up to the bin's counts.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <vector>

#include "../hysortk_amd/csrc/hsk_pairrank.h"

using namespace hsk;

static int g_fail = 0;
static long g_bins = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

struct Entry { u64 key; u32 cnt; bool operator==(const Entry &o) const { return key == o.key && cnt == o.cnt; } };

// order: the sequence in which the pairs reach their bucket's counter (a permutation of 0 .. n-1)
static void check_bin(const std::vector<u64> &key, const std::vector<u32> &cnt, const std::vector<u32> &order, int shift, u32 lower, u32 upper, const char *what)
{
    ++g_bins;
    const u32 n = (u32)key.size();
    CHECK(n <= PF_CAP, "%s: %u pairs", what, n);
    if (n > PF_CAP) return;
    // 1. buckets, arrival indices, starts, the bucket-major arrays
    std::vector<u32> bkt(PF_NBKT, 0), start(PF_NBKT + 1, 0), arr(n, 0);
    for (u32 x = 0; x < n; ++x) { const u32 i = order[x]; const u32 b = pf_bucket(key[i], shift); CHECK(b < PF_NBKT, "%s: bucket %u", what, b); if (b >= PF_NBKT) return; arr[i] = bkt[b]++; }
    for (u32 b = 0; b < PF_NBKT; ++b) start[b + 1] = start[b] + bkt[b];
    std::vector<u64> bm_key(n, 0); std::vector<u32> bm_cnt(n, 0); std::vector<unsigned char> placed(n, 0);
    for (u32 i = 0; i < n; ++i) {
        const u32 at = start[pf_bucket(key[i], shift)] + arr[i];
        CHECK(at < n && !placed[at], "%s: pair %u placed at %u", what, i, at);
        if (at >= n) return;
        placed[at] = 1; bm_key[at] = key[i]; bm_cnt[at] = cnt[i];
    }
    // 2. - 4. the walk over the pair's bucket; 5. the mask
    std::vector<u32> rank(n, 0), sum(n, 0), bits(PF_WORDS, 0); std::vector<unsigned char> kept(n, 0), head(n, 0), seen(n, 0);
    u32 heads_total = 0, all_total = 0;
    for (u32 i = 0; i < n; ++i) {
        const u32 b = pf_bucket(key[i], shift), b0 = start[b], b1 = start[b + 1];
        PfRank r = {0, 0, 0};
        for (u32 q = b0; q < b1; ++q) pf_see(r, key[i], arr[i], bm_key[q], q - b0, bm_cnt[q]);
        rank[i] = pf_rank(b0, r); sum[i] = r.sum; head[i] = pf_head(r); kept[i] = pf_keep(r, lower, upper);
        CHECK(rank[i] < n && !seen[rank[i]], "%s: pair %u has rank %u of %u (taken: %d)", what, i, rank[i], n, rank[i] < n ? (int)seen[rank[i]] : -1);
        if (rank[i] >= n) return;
        seen[rank[i]] = 1;
        all_total += cnt[i]; if (head[i]) heads_total += sum[i];
        if (kept[i]) { CHECK(pf_word(rank[i]) < PF_WORDS, "%s: mask word %u", what, pf_word(rank[i])); bits[pf_word(rank[i])] |= pf_bit(rank[i]); }
    }
    CHECK(heads_total == all_total, "%s: the heads carry %u of %u", what, heads_total, all_total);
    // the ranks order the keys, equal keys by arrival
    { std::vector<u32> by_rank(n); for (u32 i = 0; i < n; ++i) by_rank[rank[i]] = i;
      for (u32 r = 1; r < n; ++r) { const u32 p = by_rank[r - 1], q = by_rank[r]; CHECK(key[p] < key[q] || (key[p] == key[q] && arr[p] < arr[q]), "%s: ranks %u and %u out of order", what, r - 1, r); } }
    std::vector<u32> before(PF_WORDS, 0); u32 D = 0;
    for (u32 w = 0; w < PF_WORDS; ++w) { before[w] = D; D += (u32)__builtin_popcount(bits[w]); }
    std::vector<Entry> got(D, Entry{0, 0}); std::vector<unsigned char> filled(D, 0);
    for (u32 i = 0; i < n; ++i) {
        if (!kept[i]) continue;
        const u32 w = pf_word(rank[i]), o = pf_slot(before[w], bits[w], rank[i]);
        CHECK(o < D && !filled[o], "%s: entry of pair %u in slot %u of %u", what, i, o, D);
        if (o >= D) return;
        filled[o] = 1; got[o] = Entry{key[i], sum[i]};
    }
    // brute force
    std::map<u64, u32> m;
    for (u32 i = 0; i < n; ++i) m[key[i]] += cnt[i];
    std::vector<Entry> want;
    for (const auto &kv : m) if (kv.second >= lower && kv.second <= upper) want.push_back(Entry{kv.first, kv.second});
    CHECK(got == want, "%s: %zu entries, want %zu (n %u, L %u, U %u)", what, got.size(), want.size(), n, lower, upper);
}

static std::vector<u32> identity(u32 n) { std::vector<u32> o(n); for (u32 i = 0; i < n; ++i) o[i] = i; return o; }

int main()
{
    const int shift = 50;                                   // bins of 14 key bits; the buckets are bits 41 .. 49
    const u64 prefix = 0x2AAAull << shift;
    // ---- every bin of up to 12 pairs over three keys: two of one bucket (they differ below the bucket bits), one of the last bucket ----------
    const u64 alpha[3] = {prefix | (7ull << 41) | 5, prefix | (7ull << 41) | 9, prefix | ((u64)(PF_NBKT - 1) << 41)};
    for (u32 n = 0; n <= 12; ++n) {
        u64 combos = 1; for (u32 i = 0; i < n; ++i) combos *= 3;
        std::vector<u64> key(n); std::vector<u32> cnt(n);
        const std::vector<u32> fwd = identity(n); std::vector<u32> rev = fwd; std::reverse(rev.begin(), rev.end());
        for (u64 c = 0; c < combos; ++c) {
            u64 x = c; for (u32 i = 0; i < n; ++i) { key[i] = alpha[x % 3]; x /= 3; cnt[i] = 1 + (i * 7 + (u32)c) % 3; }
            check_bin(key, cnt, (c & 1) ? rev : fwd, shift, 2, 5, "enum [2, 5]");       // partial counts below L, sums beyond U
            if (n <= 8) { check_bin(key, cnt, rev, shift, 1, ~0u, "enum [1, max]"); check_bin(key, cnt, fwd, shift, 4, 4, "enum [4, 4]"); }
        }
    }
    // ---- sums on the bounds while the partial counts lie on the other side; 2^16 ------------------------------------------------------------
    for (u32 target : {1u, 2u, 3u, 49u, 50u, 51u, 65535u, 65536u, 65537u}) for (u32 parts = 1; parts <= 4; ++parts) {
        if (target < parts) continue;
        std::vector<u64> key(parts + 2); std::vector<u32> cnt(parts + 2);
        for (u32 i = 0; i < parts; ++i) { key[i] = alpha[0]; cnt[i] = i + 1 < parts ? target / parts : target - (target / parts) * (parts - 1); }
        key[parts] = alpha[1]; cnt[parts] = target; key[parts + 1] = alpha[2]; cnt[parts + 1] = 1;
        std::vector<u32> ord = identity(parts + 2); std::rotate(ord.begin(), ord.begin() + 1, ord.end());
        for (u32 lo : {target - 1 ? target - 1 : 1u, target, target + 1}) for (u32 hi : {target - 1, target, target + 1, 65535u, 0x7FFFFFFFu})
            check_bin(key, cnt, ord, shift, lo, hi, "bounds");
    }
    // a sum that wraps 32 bits, as the table's counter did
    check_bin({alpha[0], alpha[0], alpha[1]}, {0xFFFFFFFFu, 3u, 1u}, {2, 1, 0}, shift, 1, 5, "wrap");
    // ---- random bins up to PF_CAP: uniform keys, keys that share the bucket bits, few keys many times ----------------------------------------
    std::mt19937_64 rng(20240613);
    for (int it = 0; it < 700; ++it) {
        const u32 shape = (u32)(rng() % 4);
        const u32 n = it < 8 ? PF_CAP - (u32)(it % 2) : 1 + (u32)(rng() % (it % 5 == 0 ? PF_CAP : 600));
        const int sh = 48 + (int)(rng() % 8);
        const u64 pre = (rng() >> sh) << sh;
        const u32 nkeys = shape == 2 ? 1 + (u32)(rng() % 40) : 0;
        std::vector<u64> pool(nkeys); for (auto &p : pool) p = pre | (rng() & ((1ull << sh) - 1));
        std::vector<u64> key(n); std::vector<u32> cnt(n);
        for (u32 i = 0; i < n; ++i) {
            if (shape == 0) key[i] = pre | (rng() & ((1ull << sh) - 1));                                    // about one per bucket
            else if (shape == 1) key[i] = pre | (0x155ull << (sh - PF_LOG2BKT)) | (rng() & 0xFFF);              // one bucket takes the whole bin
            else if (shape == 2) key[i] = pool[rng() % nkeys];                                              // long runs of equal keys
            else key[i] = pre | ((rng() % 3) << (sh - PF_LOG2BKT)) | (rng() % 64);                          // three crowded buckets, some repeats
            cnt[i] = rng() % 8 == 0 ? 1 + (u32)(rng() % 70000) : 1 + (u32)(rng() % 40);
        }
        std::vector<u32> ord = identity(n); std::shuffle(ord.begin(), ord.end(), rng);
        const u32 lo = 1 + (u32)(rng() % 3), hi = rng() % 3 == 0 ? 65535u : rng() % 2 ? 50u : 0x7FFFFFFFu;
        check_bin(key, cnt, ord, sh, lo, hi, shape == 0 ? "random uniform" : shape == 1 ? "random one bucket" : shape == 2 ? "random runs" : "random crowded");
    }
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK %ld bins\n", g_bins);
    return 0;
}
