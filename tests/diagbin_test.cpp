// CPU exerciser of hysortk_amd/csrc/hsk_diagbin.h (diagonal number, bin, sort word, the selection's comparator), built with
// -fsanitize=address,undefined by tests/test_pair_diagonals_cpu.py.  The arithmetic is held to its definition in 128-bit integers:
// D = pos_a - pos_b + 2^32 or pos_a + pos_b, bin = D / W -- at positions 0 and 2^32 - 1 in both orientations, for W in { 1, 7, 2^31 } --
// and the sort word to what the sort needs of it: never negative, the order and the equality of the bins inside a key, the way back.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../hysortk_amd/csrc/hsk_diagbin.h"

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

typedef __int128 i128;

static uint64_t want_bin(uint64_t o, uint32_t pa, uint32_t pb, uint64_t w)
{
    const i128 D = o ? (i128)pa + pb : (i128)pa - pb + ((i128)1 << 32);
    return (uint64_t)(D / (i128)w);
}

int main()
{
    const uint32_t TOP = 0xFFFFFFFFu;
    const uint64_t widths[] = {1, 7, 16, 64, 1ull << 31};
    const uint32_t edge[] = {0, 1, 2, 6, 7, 8, 100, 255, 256, 65535, 0x7FFFFFFFu, 0x80000000u, TOP - 7, TOP - 1, TOP};
    unsigned long long checked = 0;
    // ---- the definition, at the ends of the position range --------------------------------------------------------------------------------
    CHECK(hsk::diag_number(0, 0, 0) == (1ull << 32) && hsk::diag_number(0, 0, TOP) == 1 && hsk::diag_number(0, TOP, 0) == (1ull << 33) - 1, "same strand: D at the corners");
    CHECK(hsk::diag_number(1, 0, 0) == 0 && hsk::diag_number(1, TOP, TOP) == (1ull << 33) - 2 && hsk::diag_number(1, 0, TOP) == TOP, "opposite strands: D at the corners");
    CHECK(hsk::DIAG_MAX_WIDTH == (1ull << 31), "the largest width");
    for (uint64_t w : widths)
        for (uint64_t o = 0; o < 2; ++o)
            for (uint32_t pa : edge)
                for (uint32_t pb : edge) {
                    const uint64_t b = hsk::diag_bin_of(o, pa, pb, w);
                    CHECK(b == want_bin(o, pa, pb, w), "o %llu pa %u pb %u W %llu: bin %llu", (unsigned long long)o, pa, pb, (unsigned long long)w, (unsigned long long)b);
                    ++checked;
                }
    CHECK(hsk::diag_bin_of(0, 0, TOP, 1ull << 31) == 0 && hsk::diag_bin_of(0, TOP, 0, 1ull << 31) == 3 && hsk::diag_bin_of(1, TOP, TOP, 1ull << 31) == 3, "W = 2^31: four bins at most");

    // ---- the sort word: order-preserving inside a key, and back to the reported bin ----------------------------------------------------------
    for (uint64_t w : widths)
        for (uint32_t maxpos : {0u, 1u, 255u, 1000u, 0x7FFFFFFFu, TOP})
            for (uint64_t o = 0; o < 2; ++o) {
                std::vector<uint32_t> ps;
                for (uint32_t p : edge) if (p <= maxpos) ps.push_back(p);
                for (uint32_t d = 0; d < 40 && d <= maxpos; ++d) { ps.push_back(d); ps.push_back(maxpos - d); }
                const uint64_t lo = hsk::diag_bin_lo(o, maxpos, w);
                struct Rec { uint64_t bin, word; };
                std::vector<Rec> recs;
                for (uint32_t pa : ps)
                    for (uint32_t pb : ps) {
                        const uint64_t bin = hsk::diag_bin_of(o, pa, pb, w), word = hsk::diag_sort_word(o, pa, pb, maxpos, w);
                        CHECK(bin >= lo, "o %llu pa %u pb %u maxpos %u W %llu: bin %llu below bin_lo %llu", (unsigned long long)o, pa, pb, maxpos, (unsigned long long)w, (unsigned long long)bin, (unsigned long long)lo);
                        CHECK(word == bin - lo && hsk::diag_bin_of_sort_word(o, word, maxpos, w) == bin, "the sort word does not lead back to the bin");
                        CHECK(word <= 2 * (uint64_t)maxpos / w + 1, "sort word %llu beyond 2 maxpos / W + 1 (maxpos %u, W %llu)", (unsigned long long)word, maxpos, (unsigned long long)w);
                        recs.push_back({bin, word});
                        ++checked;
                    }
                for (size_t x = 0; x < recs.size(); x += 7)
                    for (size_t y = 0; y < recs.size(); y += 5) {
                        CHECK((recs[x].bin < recs[y].bin) == (recs[x].word < recs[y].word) && (recs[x].bin == recs[y].bin) == (recs[x].word == recs[y].word), "the sort word changes the order of two bins");
                    }
            }
    // positions below 256 and W = 16: fewer than 64 values, one digit of the sort
    for (uint64_t o = 0; o < 2; ++o)
        for (uint32_t pa = 0; pa < 256; ++pa)
            for (uint32_t pb = 0; pb < 256; ++pb) CHECK(hsk::diag_sort_word(o, pa, pb, 255, 16) < 64, "positions below 256, W = 16: the sort word has more than one digit");

    // ---- the comparator: larger support, then smaller bin ----------------------------------------------------------------------------------
    CHECK(hsk::diag_better(5, 9, 4, 1) && !hsk::diag_better(4, 1, 5, 9), "larger support wins whatever the bins");
    CHECK(hsk::diag_better(5, 3, 5, 9) && !hsk::diag_better(5, 9, 5, 3), "equal support: the smaller bin wins");
    CHECK(!hsk::diag_better(5, 3, 5, 3), "a bin does not beat itself");
    CHECK(hsk::diag_better(1, ~0ull - 1, 0, ~0ull) && hsk::diag_better(1, 0, 0, ~0ull), "any bin with support beats the empty choice");
    {   // the selection over a list in any order is the first row of the largest support in ascending bin order
        const uint64_t sup[] = {3, 7, 2, 7, 7, 1}, bin[] = {10, 11, 12, 13, 14, 15};
        for (int start = 0; start < 6; ++start) {
            uint64_t bs = 0, bb = ~0ull;
            for (int q = 0; q < 6; ++q) { const int i = (start + q) % 6; if (hsk::diag_better(sup[i], bin[i], bs, bb)) { bs = sup[i]; bb = bin[i]; } }
            CHECK(bs == 7 && bb == 11, "selection from row %d on: support %llu bin %llu", start, (unsigned long long)bs, (unsigned long long)bb);
        }
    }
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK %llu bins\n", checked);
    return 0;
}
