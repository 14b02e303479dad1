"""place_items_kernel (hsk_parse.h) and bucket_scatter_kernel (hsk_combine.h) walk their input in steps and load the NEXT step's
records while the current one is written out.  The suite's base input (400 000 reads) is 29 tiles per placement workgroup: one
step, nothing prefetched is ever consumed.  Here: the smallest inputs that make two steps or more, and every other caller of the two
kernels, against the instance path (HSK_COMBINE=0) on the same input, and one list k-mer by k-mer against the oracle.

A placement step is 32 tiles of 2048 base positions; a workgroup owns tiles_per_block = ceil(tiles / 1024) consecutive tiles
(make_parse_args, hsk_host_parse.h).  A bucket-order step is 8192 items (CS_TILE) of a work item of at most 131072 (CS_ITEM); an item is
a supermer of 7.6 k-mers on average, a task has 16 virtual tasks."""
import numpy as np
import pytest

from tests import util
from tests import _combine_worker as W

pytestmark = pytest.mark.gpu
RL = 150
BASE = dict(K=31, M=17, L=2, U=200, ntasks=16, read_len=RL, seed=77, calls=["device"])
N33, N64, N65 = 450000, 880000, 890000          # reads that make 33 / 64 / 65 tiles per placement workgroup


def tiles_per_block(nreads, slabs=1):
    packed_bytes = nreads * ((RL + 3) // 4)
    ntiles = (packed_bytes * 4 + 2047) // 2048
    nblocks = min(ntiles, 1024)
    if slabs > 1:
        ntiles = (ntiles + slabs - 1) // slabs
    return (ntiles + nblocks - 1) // nblocks


def spec_of(nreads, **kw):
    return dict(BASE, nreads=nreads, genome=nreads * RL // 40, **kw)


def run(spec, env):
    return W.run_spec(dict(spec, tuning=util.tuning(env)))


_refs = {}


def instance_path(spec):
    """(digest, entries, total_kmers) of the input on the instance path: computed once per input"""
    key = repr(sorted((k, v) for k, v in spec.items() if k != "calls"))
    if key not in _refs:
        r = run(dict(spec, calls=["device"]), {"HSK_COMBINE": "0"})[0]
        assert r["combine_launches"] == 0 and r["instance_extractions"] > 0 and r["entries"] > 100000
        _refs[key] = (r["digest"], r["entries"], r["total_kmers"])
    return _refs[key]


def check(spec, env, why):
    want = instance_path(spec)
    for r in run(spec, dict(env, HSK_COMBINE_MIN_BYTES="0")):
        assert r["combine_launches"] > 0 and r["instance_extractions"] == 0, why
        assert (r["digest"], r["entries"], r["total_kmers"]) == want, why


@pytest.mark.parametrize("nreads,tiles,why", [
    (N33, 33, "a full step, then a step of one tile"),
    (N64, 64, "two full steps, nothing left"),
    (N65, 65, "two full steps and a tile"),
])
def test_placement_steps_per_block(nreads, tiles, why):
    assert tiles_per_block(nreads) == tiles
    check(spec_of(nreads), {}, why)


@pytest.mark.parametrize("nreads,ntasks,why", [
    (N65, 8, "128 virtual tasks of ~110 000 items: a work item makes 14 steps, the last one partial"),
    (N65 // 4, 40, "640 virtual tasks of ~5 500 items: less than one step, nothing prefetched"),
    (1200000, 8, "128 virtual tasks of ~150 000 items: beyond CS_ITEM, cut into two work items, the second one short"),
])
def test_bucket_scatter_steps_per_work_item(nreads, ntasks, why):
    check(spec_of(nreads, ntasks=ntasks), {}, why)


@pytest.mark.parametrize("kw,env,why", [
    (dict(K=51, L=1, U=65535), {}, "two-word keys: same placement, same bucket order"),
    (dict(K=21, M=11), {}, "the generic instance, a wide window"),
    (dict(), {"HSK_SCAN_PLACE": "1"}, "items placed by the scan: the bucket order reads chunk work items, some of them empty"),
    (dict(calls=["pinned"]), {}, "slab-pipelined placement: one launch per slab (place_one), sixteen slabs"),
    (dict(calls=["pinned"]), {"HSK_H2D_SLABS": "2"}, "... two slabs: 33 tiles per workgroup and launch, two steps in every launch"),
    (dict(calls=["loopback:2"], L=1, U=65535), {}, "two virtual ranks: the owner's items go through the bucket order"),
])
def test_other_callers_of_the_item_passes(kw, env, why):
    assert tiles_per_block(N65) == 65 and tiles_per_block(N65, 2) == 33
    spec = spec_of(N65, **kw)
    if spec["calls"] == ["loopback:2"]:
        ref = run(spec, {"HSK_COMBINE": "0"})[0]
        r = run(spec, {"HSK_COMBINE_MIN_BYTES": "0"})[0]
        assert ref["combine_launches"] == 0 and r["combine_launches"] > 0 and r["instance_extractions"] == 0, why
        assert (r["digest"], r["entries"], r["total_kmers"]) == (ref["digest"], ref["entries"], ref["total_kmers"]), why
    else:
        check(spec, env, why)


def test_two_step_placement_vs_oracle(tmp_path):
    """the list itself, k-mer by k-mer, against the CPU oracle at the 33-tile size"""
    from oracle import hsk_oracle as O
    assert tiles_per_block(N33) == 33
    dump = str(tmp_path / "p33.npz")
    r = run(spec_of(N33, ntasks=8, L=1, U=65535, dump=dump), {"HSK_COMBINE_MIN_BYTES": "0"})[0]
    assert r["combine_launches"] > 0 and r["instance_extractions"] == 0
    z = np.load(dump)
    want = O.count(z["packed"], z["off"], z["lens"], k=31, m=17, L=1, U=65535, ntasks=8, fast=True)
    assert np.array_equal(want.task_off, z["task_off"]) and np.array_equal(want.keys, z["kmers"]) and np.array_equal(want.cnt, z["cnt"])
