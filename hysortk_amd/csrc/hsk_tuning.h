// hsk_tuning.h -- the tuning names: hsk_config::tuning ("name=value,name=value", copied at hsk_init), behind it the environment's HSK_TUNING
// (ad-hoc diagnostics without touching the client).  Forced paths for the byte-identity tests and a handful of measured thresholds; never an
// algorithm a caller would choose (those are hsk_config fields and HSK_FLAG_*).  Held per CONTEXT (hsk_ctx::tune): two contexts of one
// process may differ.  The table below is the list -- one row per name: identifier, default, what it forces; INTEGRATION.md section 5 says
// more about each.  A read is a member access (c->tune.parse_fast): a name that is not in the table does not compile, and a default is
// written once, here.  A row nobody reads fails tests/test_host_logic.py.
//
// No HIP in here: parse() runs on the CPU under the sanitizers (tests/tuning_test.cpp).
#pragma once
#include <stdlib.h>
#include <string.h>

namespace hsk {

#define HSK_TUNING_TABLE(X)                                                                                                              \
    /* parse (hsk_host_parse.h, hsk_api.hip) */                                                                                          \
    X(parse_fast, 1)               /* 0: the general parse kernels */                                                                    \
    X(parse_rec_cap, 0)            /* record slots per tile instead of the window's (parse_rec_cap, hsk_parseplan.h); 0 = by window */  \
    X(scan_generic, 0)             /* 1: the generic scan_kernel instance for the default (k, m) too */                                  \
    X(scan_place, 0)               /* 1: the scan places the items of the combining extraction itself (chunked bins) */                  \
    X(bin_cap_pct, 125)            /* chunks of the scan-placed bins, per cent of the expectation (tests: a store that runs out) */      \
    X(bin_vmax, 0)                 /* > 0: chunks a bin's map holds (tests: a bin beyond its map) */                                     \
    X(place_bytes, -1)             /* 0 / 1: supermers as byte runs never / always; -1 = when they travel between ranks */              \
    X(drop_certain, 1)             /* 0: the scan keeps the homopolymer k-mers the sketch has found more than U copies of */            \
    /* ingest of hsk_count (hsk_api.hip, hsk_host_pipeline.h) */                                                                         \
    X(zero_copy, 1)                /* 0: pinned input is copied to the device, not read in place */                                      \
    X(uniform_len, 1)              /* 0: the read lengths are always copied, never generated from a sample */                            \
    X(derive_offsets, 1)           /* 0: the read offsets are always copied, never derived from the lengths */                           \
    X(h2d_slabs, 16)               /* pinned input: slabs copied ahead of the scan; 0 / 1: read in place over PCIe */                    \
    X(ingest_pipeline, 1)          /* 0: no ingest + scan + placement as one pipeline over the slabs (the two-step parse) */             \
    /* the plan of a call (hsk_api.hip, hsk_host_pipeline.h) */                                                                          \
    X(plan_sample, 1)              /* 0: no sketch of the input, the context's memory of earlier calls decides */                        \
    X(plan_min_input, 32LL << 20)  /* packed bytes below which no sketch is taken (MIN_INPUT of estimate_plan; tests lower it) */        \
    X(xcd_batch, 1)                /* 0: one task at a time instead of one per XCD */                                                    \
    X(force_no_xcd, 0)             /* 1: behave as on a partitioned device (hsk_init's census is overruled) */                           \
    X(overlap, 1)                  /* 0: one exchange up front instead of one per task group behind the counting */                      \
    X(lag, -1)                     /* 0 / 1: second stage of a batch's aggregation behind the next batch; -1 = when the result stays in HBM */ \
    X(early_d2h, 1)                /* 0: no result copies while later batches are counted */                                             \
    X(compact_d2h, 2)              /* 0 / 1: 16- / 10-byte entries over PCIe instead of 7 */                                             \
    X(widen_threads, 0)            /* host threads that widen compact entries (at most 64); 0 = half the cores, 2 .. 32 */               \
    /* expand, sort, scatter (hsk_host_expand.h, hsk_host_sort.h, hsk_host_scatter.h) */                                                 \
    X(expand_reserve, 1)           /* 0: expand_kernel's tiles get their output ranges from tile sums + a scan, not with an atomic */    \
    X(unstable_first, 1)           /* 0: the first scatter pass is stable like the others */                                             \
    X(wide_lookback, 0)            /* 1: 64-bit look-back words for every task size */                                                   \
    X(fused_scatter, 1)            /* 0: extraction and first scatter pass as two kernels */                                             \
    X(fused_scatter_ext, 1)        /* ... the same with EXTENSION */                                                                     \
    X(fused_scatter_wide, 1)       /* ... the same for two-word keys */                                                                  \
    X(xs2, 1)                      /* 0: expand_scatter_kernel (one sweep per flush) where expand_scatter2_kernel would run */           \
    X(scatter_generic, 0)          /* 1: the generic fused-scatter instance for the default k too */                                     \
    /* table finishes (hsk_host_finish.h) */                                                                                             \
    X(agg_adapt, 1)                /* 0: never leave the aggregation, 2: leave it after the first batch, 3: as 1 with tables on every rung */ \
    X(agg_large, 1)                /* 0: a prefix bin of 65536 records and more is counted by one workgroup, not in slices */            \
    X(agg_maxrung, 13)             /* last rung of the table ladder (AG_LOG2CAP_HUGE; tests stop it early: the long way) */              \
    /* combining extraction (hsk_host_combine.h, hsk_host_pipeline.h) */                                                                 \
    X(combine, 1)                  /* 0 = HSK_FLAG_NO_COMBINE */                                                                         \
    X(combine_dedup, 1)            /* 0: combine_kernel rolls every supermer item, equal ones too */                                     \
    X(combine_min_bytes, 64LL << 20) /* packed bytes from which the combining extraction is considered */                                \
    X(combine_bucket, 12288)       /* k-mers per minimizer bucket it aims at (at least 256) */                                           \
    X(combine_ratio, 16)           /* k-mers per pair below which it does not pay (at least 1) */                                        \
    X(combine_prefix, 0)           /* 9 .. 16: key bits of its finish's bins; 0 = following the pairs per task */                        \
    X(pair_cap, 1)                 /* 0: its pair stores hold a task's k-mers, not 4 x the sketch's promise */                           \
    X(pair_cap_records, 0)         /* > 0: ... hold that many records (tests: stores that run over) */                                   \
    /* checking (hsk_pool.h) */                                                                                                          \
    X(pool_redzone, 0)             /* bytes of red zone behind every device block (at most 2^20), compared when a call ends */

struct Tuning {
#define X(name, dflt) long long name = dflt;
    HSK_TUNING_TABLE(X)
#undef X
#define X(name, dflt) bool name##_set = false;
    HSK_TUNING_TABLE(X)
#undef X

    // "name=value,name=value": an item without '=' or without a name is skipped, leading spaces of a name are dropped, the value is atoll of
    // what follows '='; a name that is already set stays (within one string and from one call to the next), an unknown name is ignored
    void parse(const char *s)
    {
        while (s && *s) {
            const char *e = strchr(s, ',');
            const char *q = (const char *)memchr(s, '=', e ? (size_t)(e - s) : strlen(s));
            if (q && q > s) {
                const char *k = s; while (*k == ' ') ++k;
                set(k, (size_t)(q - k), atoll(q + 1));      // (atoll stops at the item's ',')
            }
            s = e ? e + 1 : nullptr;
        }
    }

private:
    void set(const char *k, size_t n, long long value)
    {
#define X(name, dflt) if (n == sizeof(#name) - 1 && memcmp(k, #name, n) == 0) { if (!name##_set) { name = value; name##_set = true; } return; }
        HSK_TUNING_TABLE(X)
#undef X
    }
};

} // namespace hsk
