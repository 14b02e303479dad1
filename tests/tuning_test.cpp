// CPU exerciser of hysortk_amd/csrc/hsk_tuning.h (the table of tuning names and Tuning::parse), built with -fsanitize=address,undefined by
// tests/test_tuning.py.  The names and defaults are written out here once more, as data, independently of the header's table: a default
// that moves, a row that goes or a name parse() no longer knows fails here.  parse() is held to its grammar: items separated by ',', an
// item without '=' or without a name skipped, leading spaces (only spaces, only leading) dropped from a name, the value atoll of what
// follows '=', the first setting of a name kept, unknown names ignored.
#include <cstdio>
#include <cstring>
#include <string>

#include "../hysortk_amd/csrc/hsk_tuning.h"

using hsk::Tuning;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

struct Row { const char *name; long long dflt; long long Tuning::*value; bool Tuning::*set; };
#define ROW(name, dflt) {#name, dflt, &Tuning::name, &Tuning::name##_set}
static const Row ROWS[] = {
    ROW(expand_reserve, 1), ROW(unstable_first, 1), ROW(agg_adapt, 1), ROW(agg_large, 1), ROW(overlap, 1), ROW(xcd_batch, 1), ROW(fused_scatter, 1),
    ROW(fused_scatter_ext, 1), ROW(fused_scatter_wide, 1), ROW(xs2, 1), ROW(pair_cap, 1), ROW(early_d2h, 1), ROW(ingest_pipeline, 1), ROW(parse_fast, 1),
    ROW(combine, 1), ROW(combine_dedup, 1), ROW(plan_sample, 1), ROW(drop_certain, 1), ROW(zero_copy, 1), ROW(uniform_len, 1), ROW(derive_offsets, 1),
    ROW(widen_threads, 0), ROW(wide_lookback, 0), ROW(pair_cap_records, 0), ROW(scan_place, 0), ROW(bin_vmax, 0), ROW(parse_rec_cap, 0), ROW(scan_generic, 0),
    ROW(scatter_generic, 0), ROW(combine_prefix, 0), ROW(pool_redzone, 0), ROW(force_no_xcd, 0),
    ROW(lag, -1), ROW(place_bytes, -1),
    ROW(compact_d2h, 2), ROW(h2d_slabs, 16), ROW(combine_ratio, 16), ROW(bin_cap_pct, 125), ROW(combine_bucket, 12288), ROW(agg_maxrung, 13),
    ROW(plan_min_input, 32LL << 20), ROW(combine_min_bytes, 64LL << 20),
};
constexpr int NROWS = sizeof ROWS / sizeof ROWS[0];
static_assert(NROWS == 42, "42 names");
#define X(name, dflt) +1
static_assert(0 HSK_TUNING_TABLE(X) == NROWS, "the header's table has as many rows as this list");
#undef X

static int row_of(const char *name)
{
    for (int i = 0; i < NROWS; ++i) if (strcmp(ROWS[i].name, name) == 0) return i;
    return -1;
}

// every name but `except` (-1: every name) is at its default and not marked as set
static void check_defaults(const Tuning &t, int except, const char *what)
{
    for (int i = 0; i < NROWS; ++i) {
        if (i == except) continue;
        CHECK(t.*ROWS[i].value == ROWS[i].dflt, "%s: %s is %lld, default %lld", what, ROWS[i].name, t.*ROWS[i].value, ROWS[i].dflt);
        CHECK(!(t.*ROWS[i].set), "%s: %s is marked as set", what, ROWS[i].name);
    }
}

// `s` sets exactly the name `name` to `value` (name == nullptr: it sets nothing)
static void check_one(const char *s, const char *name, long long value)
{
    Tuning t; t.parse(s);
    const int r = name ? row_of(name) : -1;
    CHECK(!name || r >= 0, "%s is not in the test's list", name);
    check_defaults(t, r, s ? s : "(null)");
    if (r >= 0) {
        CHECK(t.*ROWS[r].value == value, "\"%s\": %s is %lld, expected %lld", s, name, t.*ROWS[r].value, value);
        CHECK(t.*ROWS[r].set, "\"%s\": %s is not marked as set", s, name);
    }
}

int main()
{
    { Tuning t; check_defaults(t, -1, "fresh"); }
    check_one(nullptr, nullptr, 0);
    check_one("", nullptr, 0);

    // every name set alone is read back (a value no default has: 7 + its row, and a negative one), the others stay; its upper-case spelling is unknown
    for (int i = 0; i < NROWS; ++i) {
        for (long long v : {7LL + i, -3LL - i, 0LL, 1LL << 40}) {
            const std::string s = std::string(ROWS[i].name) + "=" + std::to_string(v);
            check_one(s.c_str(), ROWS[i].name, v);
        }
        std::string up = ROWS[i].name; for (char &ch : up) if (ch >= 'a' && ch <= 'z') ch = (char)(ch - 'a' + 'A');
        check_one((up + "=5").c_str(), nullptr, 0);
        // a name that is a prefix of this one, or this one and more, is another name
        check_one((std::string(ROWS[i].name) + "x=5").c_str(), nullptr, 0);
        const std::string shorter(ROWS[i].name, strlen(ROWS[i].name) - 1);
        check_one((shorter + "=5").c_str(), row_of(shorter.c_str()) >= 0 ? shorter.c_str() : nullptr, 5);
    }

    // all of them in one string, each with a value of its own
    {
        std::string s;
        for (int i = 0; i < NROWS; ++i) s += std::string(i ? "," : "") + ROWS[i].name + "=" + std::to_string(1000 + i);
        Tuning t; t.parse(s.c_str());
        for (int i = 0; i < NROWS; ++i) CHECK(t.*ROWS[i].value == 1000 + i && t.*ROWS[i].set, "all names in one string: %s is %lld", ROWS[i].name, t.*ROWS[i].value);
    }

    // the first setting of a name wins: inside one string ...
    check_one("parse_fast=0,parse_fast=1", "parse_fast", 0);
    check_one("lag=1,lag=0,lag=-1", "lag", 1);
    check_one("h2d_slabs=16,h2d_slabs=4", "h2d_slabs", 16);                 // (set to its default: still set)
    // ... and from one parse() to the next (hsk_init: the client's string, then HSK_TUNING)
    {
        Tuning t; t.parse("parse_fast=0,combine_ratio=3"); t.parse("parse_fast=1,combine_ratio=9,xs2=0");
        CHECK(t.parse_fast == 0 && t.combine_ratio == 3 && t.xs2 == 0, "two calls: parse_fast %lld combine_ratio %lld xs2 %lld", t.parse_fast, t.combine_ratio, t.xs2);
        Tuning u; u.parse(nullptr); u.parse("xs2=0"); u.parse(""); u.parse("xs2=1");
        CHECK(u.xs2 == 0 && u.xs2_set, "two calls after NULL: xs2 %lld", u.xs2);
        Tuning w; w.parse("h2d_slabs=16"); w.parse("h2d_slabs=4");
        CHECK(w.h2d_slabs == 16, "a name set to its default stays: h2d_slabs %lld", w.h2d_slabs);
    }

    // the grammar's corners
    check_one(" parse_fast=0", "parse_fast", 0);                           // leading spaces go
    check_one("   parse_fast=0", "parse_fast", 0);
    { Tuning t; t.parse("xs2=0, parse_fast=0"); CHECK(t.xs2 == 0 && t.parse_fast == 0, "a space behind the comma: xs2 %lld parse_fast %lld", t.xs2, t.parse_fast); }
    check_one("parse_fast =0", nullptr, 0);                                // a trailing space belongs to the name: unknown
    check_one("\tparse_fast=0", nullptr, 0);                               // only spaces are dropped
    check_one("parse fast=0", nullptr, 0);
    check_one("=3", nullptr, 0);                                           // no name
    check_one(" =3", nullptr, 0);
    check_one("parse_fast", nullptr, 0);                                   // no '='
    check_one(",,", nullptr, 0);
    check_one(",", nullptr, 0);
    check_one("parse_fast=0,", "parse_fast", 0);
    check_one(",parse_fast=0", "parse_fast", 0);
    check_one(",,parse_fast=0,,", "parse_fast", 0);
    check_one("PARSE_FAST=0", nullptr, 0);
    check_one("Parse_fast=0", nullptr, 0);
    check_one("lag=-1", "lag", -1);                                        // negative values are kept (and -1, lag's default, marks it as set)
    check_one("lag=-7", "lag", -7);
    check_one("combine_min_bytes=0", "combine_min_bytes", 0);
    check_one("plan_min_input=64MB", "plan_min_input", 64);                // atoll: the digits in front
    check_one("parse_fast=x", "parse_fast", 0);                            // atoll: no digits, 0
    check_one("parse_fast=", "parse_fast", 0);
    check_one("parse_fast=,xs2", "parse_fast", 0);                         // (an empty value does not reach into the next item)
    check_one("parse_fast= 0", "parse_fast", 0);                           // atoll skips white space in front of the digits
    check_one("parse_fast=+0", "parse_fast", 0);
    check_one("parse_fast=0=1", "parse_fast", 0);                          // the first '=' ends the name
    check_one("widen_threads=3.9", "widen_threads", 3);
    check_one("x=1,parse_fast=0", "parse_fast", 0);                        // an unknown name in front changes nothing
    check_one("parse_fast=0,x=1", "parse_fast", 0);
    check_one("tune=1,get=2,v=3,parse=4,set=5", nullptr, 0);
    check_one("parse_fast_set=1", nullptr, 0);                             // the marks are no names

    // 4 KB of unknown names, with a known one at the very end
    {
        std::string s;
        while (s.size() < 4096) s += "no_such_name_" + std::to_string(s.size()) + "=" + std::to_string(s.size() % 7) + ",";
        check_one(s.c_str(), nullptr, 0);
        check_one((s + "bin_vmax=9").c_str(), "bin_vmax", 9);
        const std::string one(4096, 'q');                                   // one item of 4 KB without '=', and one with
        check_one(one.c_str(), nullptr, 0);
        check_one((one + "=1").c_str(), nullptr, 0);
    }

    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK %d names\n", NROWS);
    return 0;
}
