"""Capacities at their edges, with red zones behind every device block (tuning pool_redzone, hsk_pool.h): a kernel that writes past the end of
a block fails the call with HSK_ERR_INTERNAL and names the block's allocation site, even where nothing reads the bytes it overwrote.

- The combining extraction's pair stores (kA / vA: rec_cap records per task) swept over caps around the task's pair count P: the low caps make
  the chunk store run over (error bit 512), the caps between hold more records than bit 512 can see (the host compares every task's pairs with
  rec_cap), P and P + 1 fit.  The sort buffers are requested with 64 bytes to spare: P - 8 and P - 9 sit on either side of that slack.
- Every plan the suite covers, once more with the red zones on: the same list as without them.
- The scan's record store and the scan-placed bin store at and around their default capacities."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import util
from tests import _combine_worker as W

pytestmark = pytest.mark.gpu
RZ = "pool_redzone=4096"
BASE = dict(K=31, M=17, L=2, U=200, ntasks=16, genome=1500000, read_len=150, nreads=400000, seed=77, calls=["device"])
CH = {31: 4096, 51: 2048}                                    # records per chunk of the pair store (one-word / two-word keys)


def run(spec, extra=None):
    """one context with the tuning string `extra` (a "name=value,..." string), one result dict per call"""
    return W.run_spec(dict(spec, tuning=extra))


def keys(r):
    return (r["digest"], r["entries"], r["total_kmers"])


# ---- the pair stores of the combining extraction: one task, so combine_pairs is its pair count P ----
SWEEPS = {
    # ~1.5 M pairs in one task: more chunks than bit 512 lets a store of one record have (a task of 10^6 pairs fits in 257 spare chunks)
    "k31": (dict(BASE, L=1, ntasks=1), "combine_min_bytes=0"),
    "k51": (dict(BASE, K=51, L=1, ntasks=1), "combine_min_bytes=0"),
    # ONE task in 512 bins of ~2900 pairs (test_weighted_long_way_on_one_gpu): the pairs are sorted by sort_task_device and summed
    "weighted": (dict(BASE, L=1, ntasks=1), "combine_min_bytes=0,combine_prefix=9"),
}


def sweep_caps(P, ch):
    """from stores that hold every pair down to one record: a store written a few records past its end fails on the first cap that shows it"""
    return sorted({max(1, x) for x in (1, P // 4, P - 64 * ch, P - ch, P - ch // 2, P - 9, P - 8, P - 1, P, P + 1)}, reverse=True)


@pytest.mark.parametrize("which", sorted(SWEEPS))
def test_pair_store_capacity_sweep(which, tmp_path):
    spec, extra = SWEEPS[which]
    ref = run(spec, "combine=0")[0]
    full = [run(spec, extra + ",pair_cap=0," + RZ)[0] for _ in range(2)]           # full-size stores (the sketch's cap off)
    P = full[0]["combine_pairs"]
    assert full[0]["combine_launches"] > 0 and 0 < P <= full[0]["combine_kmers"]
    assert full[1]["combine_pairs"] == P, "the pair count of this input is not reproducible: the sweep needs an input where it is"
    assert keys(full[0]) == keys(full[1]) == keys(ref)
    ch = CH[spec["K"]]
    for cap in sweep_caps(P, ch):
        sp = dict(spec, dump=str(tmp_path / "p.npz")) if cap == P - 1 and which != "weighted" else spec
        r = run(sp, "%s,%s,pair_cap_records=%d" % (extra, RZ, cap))[0]                # (HskError: a red zone was written)
        assert keys(r) == keys(ref), (which, P, cap)
        assert r["combine_launches"] > 0 and r["combine_pairs"] == P, (which, P, cap)   # (a store that ran over: the call again, full size, same plan)
        if which == "weighted":
            assert r["redone_tasks"] > 0, (which, P, cap)
        else:
            assert r["instance_extractions"] == 0, (which, P, cap)
        if cap == P - 1 and which != "weighted":
            from oracle import hsk_oracle as O
            z = np.load(sp["dump"])
            want = O.count(z["packed"], z["off"], z["lens"], k=spec["K"], m=spec["M"], L=spec["L"], U=spec["U"], ntasks=1, fast=True)
            assert np.array_equal(want.task_off, z["task_off"]) and np.array_equal(want.keys, z["kmers"]) and np.array_equal(want.cnt, z["cnt"]), (which, cap)


def test_pair_stores_that_run_over_start_again_full_size():
    """hsk_stats is restored when a call starts again, so only HSK_TIMING shows that it did: a fresh process whose stores hold one record per task
    (the chunk store runs over: error bit 512) and one whose stores hold P - CH / 2 records (too few spare chunks for bit 512 to fire: the host's
    comparison of the pairs with the store).  Both say why they started again, and both give the list of the instance path."""
    spec, extra = SWEEPS["k31"]
    ref = run(spec, "combine=0")[0]
    P = run(spec, extra + ",pair_cap=0")[0]["combine_pairs"]
    for cap, why in ((1, "the pair stores ran over (sized from the estimate)"), (P - CH[31] // 2, "the pair stores ran over (more pairs than records)")):
        env = dict(os.environ, HSK_TIMING="1")
        arg = json.dumps(dict(spec, tuning="%s,%s,pair_cap_records=%d" % (extra, RZ, cap)))
        p = subprocess.run([sys.executable, os.path.join(util.ROOT, "tests", "_combine_worker.py"), arg], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        r = json.loads(p.stdout.strip().splitlines()[-1])
        assert why in p.stderr, (cap, [l for l in p.stderr.splitlines() if "starts again" in l])
        assert keys(r) == keys(ref) and r["combine_launches"] > 0, cap


# ---- every plan the suite covers, with red zones behind every block ----
MANY = dict(BASE, genome=6000000, nreads=1500000)
POLY = dict(BASE, U=65535, L=2, poly_a_pct=5.0, calls=["pinned", "host"], ntasks=8)


@pytest.mark.parametrize("spec,extra,why", [
    (BASE, "combine=0", "the instance path"),
    (BASE, "combine_min_bytes=0", "the combining extraction, one-word keys"),
    (dict(BASE, K=51, L=1, U=65535), "combine_min_bytes=0", "the combining extraction, two-word keys"),
    (dict(BASE, K=77, M=17, L=1, U=65535), "", "three-word keys"),
    (dict(BASE, EXT=1, L=1, U=65535), "", "EXTENSION"),
    (dict(BASE, plan="full_sort"), "", "HSK_FLAG_FULL_SORT"),
    (dict(BASE, plan="no_aggregation"), "", "HSK_FLAG_NO_AGGREGATION"),
    (BASE, "combine_min_bytes=0,parse_rec_cap=200", "the scan's record store runs over: the general parse kernels"),
    (MANY, "combine_min_bytes=0,scan_place=1,bin_cap_pct=1", "the scan-placed bin store runs out: the call again on the instance path"),
    (MANY, "combine_min_bytes=0,scan_place=1,bin_vmax=1", "a bin of more chunks than its map has entries"),
    (POLY, "combine_min_bytes=0", "5 % all-A reads: the combining extraction counts the all-A bucket in CB_UNIT slices"),
    (POLY, "combine=0", "5 % all-A reads: the instance path counts the all-A bin in slices (agg_large)"),
    (dict(POLY, U=40), "plan_min_input=1", "5 % all-A reads: the sketch is certain the all-A k-mer goes, the scan drops it"),
    (dict(BASE, ntasks=16, genome=2000000, nreads=480000, L=1, U=65535, calls=["loopback:2"]), "combine_min_bytes=0", "two virtual ranks"),
    (dict(BASE, ntasks=72, genome=2000000, nreads=480000, L=1, U=65535, calls=["loopback:8"]), "combine_min_bytes=0", "eight virtual ranks"),
    (dict(BASE, calls=["host", "pinned"]), "combine_min_bytes=0", "hsk_count from pageable and from pinned memory"),
], ids=["instance", "combine", "combine_k51", "k77", "extension", "full_sort", "no_aggregation", "parse_rec_cap_200", "bin_cap_pct_1", "bin_vmax_1",
        "poly_a_combine", "poly_a_agg_large", "poly_a_certain_drops", "loopback_2", "loopback_8", "host_pinned"])
def test_every_plan_under_red_zones(spec, extra, why):
    a = run(spec, extra or None)
    b = run(spec, (extra + "," + RZ) if extra else RZ)                  # (HskError: a red zone was written)
    assert [keys(x) for x in b] == [keys(x) for x in a], why
    assert [(x["combine_launches"] > 0, x["dropped_kmers"], x["parse_fallbacks"]) for x in b] == \
        [(x["combine_launches"] > 0, x["dropped_kmers"], x["parse_fallbacks"]) for x in a], why
    if "plan_min_input" in extra:
        assert all(x["dropped_kmers"] > 0 for x in b), why


# ---- the scan's record store and the scan-placed bin store at their edges ----
@pytest.mark.parametrize("rec_cap,fallback", [(512, False), (256, None)])
def test_scan_record_store_at_its_default_capacity_and_half(rec_cap, fallback):
    """K = 31, M = 17: 512 records per 2048-position tile by default (parse_rec_cap, hsk_host_parse.h).  At the default the scan keeps its fast
    path; half of it still holds most tiles of these reads (parse_rec_cap=200 does not: test_every_plan_under_red_zones), so only the list is
    held there.  The same list either way."""
    ref = run(BASE, "combine=0")[0]
    for extra in ("combine=0", "combine_min_bytes=0"):
        r = run(BASE, "%s,%s,parse_rec_cap=%d" % (extra, RZ, rec_cap))[0]
        assert keys(r) == keys(ref), (extra, rec_cap)
        assert fallback is None or (r["parse_fallbacks"] > 0) == fallback, (extra, rec_cap, r["parse_fallbacks"])


@pytest.mark.parametrize("pct", [100, 101])
def test_scan_placed_bin_store_at_its_edge(pct):
    """bin_cap_pct: the scan-placed items' chunk store in per cent of the chunks expected; from 100 on it also keeps a first chunk and one opened
    ahead per bin (below: one per bin).  At 100 and 101 the same list as the instance path."""
    ref = run(BASE, "combine=0")[0]
    r = run(BASE, "combine_min_bytes=0,scan_place=1,bin_cap_pct=%d,%s" % (pct, RZ))[0]
    assert keys(r) == keys(ref), pct
    assert r["combine_launches"] > 0, pct
