// CPU exerciser of hysortk_amd/csrc/hsk_strandbits.h (the K bases of a read at a position, and their strand against an entry's canonical
// k-mer), built with -fsanitize=address,undefined by tests/test_strandbits.py.  Every packed buffer is a heap block of exactly the bytes
// the reads take, so a load that touches a byte behind the last read's last base is an AddressSanitizer report.  The loaded k-mer is held
// to one built base by base, the strand to a reverse complement taken on the strings.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../hysortk_amd/csrc/hsk_strandbits.h"

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }

static int code(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3; }
static std::string revcomp(const std::string &s)
{
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = "TGCA"[code(c)];
    return r;
}
static std::string random_read(size_t n) { std::string s(n, 'A'); for (char &c : s) c = "ACGT"[rnd() & 3]; return s; }

// the Mer layout, base by base
template <int NW> static void mer_of(const std::string &s, uint64_t (&w)[NW])
{
    for (int i = 0; i < NW; ++i) w[i] = 0;
    for (size_t i = 0; i < s.size(); ++i) w[i / 32] |= (uint64_t)code(s[i]) << (2 * (31 - i % 32));
}

// reads packed as hsk_count reads them, every read from a byte boundary, in a heap block of exactly their bytes
struct Packed {
    uint8_t *p = nullptr; uint64_t nbytes = 0; std::vector<uint64_t> off;
    explicit Packed(const std::vector<std::string> &reads)
    {
        for (const auto &r : reads) { off.push_back(nbytes); nbytes += (r.size() + 3) / 4; }
        p = (uint8_t *)std::malloc(nbytes ? nbytes : 1);
        std::memset(p, 0, nbytes);
        for (size_t k = 0; k < reads.size(); ++k)
            for (size_t i = 0; i < reads[k].size(); ++i) p[off[k] + i / 4] |= (uint8_t)(code(reads[k][i]) << (6 - 2 * (i % 4)));
    }
    ~Packed() { std::free(p); }
};

static uint64_t g_loads = 0, g_fwd = 0, g_rev = 0, g_pal = 0, g_mis = 0;

// every position of the LAST read of `reads`: the load, and the strand against the canonical k-mer, its twin's owner and a stranger
template <int NW> static void check_reads(const std::vector<std::string> &reads, int k)
{
    const Packed pk(reads);
    const std::string &rd = reads.back();
    const uint64_t base = pk.off.back();
    for (size_t pos = 0; pos + k <= rd.size(); ++pos) {
        const std::string s = rd.substr(pos, k), t = revcomp(s), canon = s < t ? s : t;
        uint64_t f[NW], want[NW], tw[NW], want_tw[NW], e[NW];
        hsk::strand_load<NW>(pk.p, pk.nbytes, 8 * base + 2 * pos, k, f);
        mer_of<NW>(s, want); mer_of<NW>(t, want_tw); mer_of<NW>(canon, e);
        bool same = true, same_tw = true;
        hsk::strand_twin<NW>(f, k, tw);
        for (int i = 0; i < NW; ++i) { same = same && f[i] == want[i]; same_tw = same_tw && tw[i] == want_tw[i]; }
        CHECK(same, "K %d pos %zu byte phase %llu: word 0 %016llx, expected %016llx", k, pos, (unsigned long long)(base & 3), (unsigned long long)f[0], (unsigned long long)want[0]);
        CHECK(same_tw, "K %d pos %zu: the twin differs from the string's reverse complement", k, pos);
        ++g_loads;
        const int got = hsk::strand_decide<NW>(f, e, k);
        const int exp = s == t ? hsk::STRAND_PALINDROME : s == canon ? hsk::STRAND_FORWARD : hsk::STRAND_REVERSE;
        CHECK(got == exp, "K %d pos %zu: strand %d, expected %d", k, pos, got, exp);
        g_fwd += exp == hsk::STRAND_FORWARD; g_rev += exp == hsk::STRAND_REVERSE; g_pal += exp == hsk::STRAND_PALINDROME;
        // a k-mer that is neither: one base of the canonical k-mer changed (and the change checked on the strings)
        std::string other = canon;
        const size_t at = rnd() % (size_t)k;
        other[at] = "ACGT"[(code(other[at]) + 1 + rnd() % 3) & 3];
        if (other != s && other != t) {
            mer_of<NW>(other, e);
            CHECK(hsk::strand_decide<NW>(f, e, k) == hsk::STRAND_MISMATCH, "K %d pos %zu: a stranger's k-mer was taken for the read's", k, pos);
            ++g_mis;
        }
    }
}

template <int NW> static void check_k(int k)
{
    // the read under test behind 0 .. 3 bytes of another read (every byte phase of its start against the aligned words), its length
    // such that its last base sits at every bit offset 0 / 2 / 4 / 6 of the buffer's last byte; every position has every bit offset
    for (int lead = 0; lead < 4; ++lead)
        for (int extra = 0; extra < 4; ++extra) {
            std::vector<std::string> reads;
            if (lead) reads.push_back(random_read(4 * lead - (rnd() % 4)));
            reads.push_back(random_read((size_t)k + 36 + extra));
            check_reads<NW>(reads, k);
        }
    { std::vector<std::string> one; one.push_back(random_read(k)); check_reads<NW>(one, k); }      // a read of exactly K bases, alone
    if (k % 2 == 0) {                                       // ACGT repeats: k-mers that are their own reverse complement
        for (int extra = 0; extra < 4; ++extra) {
            std::string s; while ((int)s.size() < k + 8 + extra) s += "ACGT";
            s.resize(k + 8 + extra);
            std::vector<std::string> reads; reads.push_back(random_read(5)); reads.push_back(s);
            check_reads<NW>(reads, k);
        }
    }
}

int main()
{
    const int ks[] = {3, 4, 21, 31, 33, 51, 63, 65, 77, 95, 22, 34, 62, 66, 94};
    for (int k : ks) {
        const uint64_t pal0 = g_pal;
        if (k <= 31) check_k<1>(k); else if (k <= 63) check_k<2>(k); else check_k<3>(k);
        if (k % 2 == 0) CHECK(g_pal > pal0, "K %d: no palindrome among the ACGT repeats", k);
    }
    CHECK(g_fwd > 1000 && g_rev > 1000 && g_pal > 10 && g_mis > 1000, "cases: %llu forward, %llu reverse, %llu palindromes, %llu strangers",
          (unsigned long long)g_fwd, (unsigned long long)g_rev, (unsigned long long)g_pal, (unsigned long long)g_mis);
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK %llu loads, %llu forward, %llu reverse, %llu palindromes, %llu strangers\n", (unsigned long long)g_loads, (unsigned long long)g_fwd,
                (unsigned long long)g_rev, (unsigned long long)g_pal, (unsigned long long)g_mis);
    return 0;
}
