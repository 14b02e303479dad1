"""One scope per entry point (ApiCall, hysortk_amd/csrc/hsk_api.hip): a call that fails after it has allocated hands every device block back
(live bytes at its close = live bytes at its open, HSK_TIMING's line per call), and nothing of one call's state (CallState) reaches the next:
a count on the same context afterwards equals a fresh context's, and so do the stage entry points after a count that took the combining
extraction.  Nor does one context's tuning reach another's calls: two live contexts called in turn on one thread each take their own path."""
import json
import os
import re
import subprocess
import sys

import pytest

from tests import util

pytestmark = pytest.mark.gpu
INVALID_ARG = 1
LINE = re.compile(r"^\[hsk\] call (\w+): rc (-?\d+), pool live (\d+) -> (\d+) bytes, (\d+) blocks rolled back", re.M)


def run_worker(spec):
    env = dict(os.environ, HSK_TIMING="1")
    p = subprocess.run([sys.executable, os.path.join(util.ROOT, "tests", "_calls_worker.py"), json.dumps(spec)], env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1]), [(m[0], int(m[1]), int(m[2]), int(m[3]), int(m[4])) for m in LINE.findall(p.stderr)]


@pytest.mark.parametrize("tuning", [None, "pool_redzone=4096"], ids=["plain", "redzone"])
def test_failed_calls_hand_back_what_they_allocated(tuning):
    res, calls = run_worker(dict(mode="failures", tuning=tuning))
    failing = ["hsk_count_loopback", "hsk_stage_count_sorted", "hsk_stage_task_kmers", "hsk_format_entries"]
    assert [res[n] for n in failing] == [INVALID_ARG] * len(failing), res
    failed = [c for c in calls if c[1] != 0]
    assert [c[0] for c in failed] == failing, calls
    for name, rc, live_open, live_close, rolled in failed:
        assert rc == INVALID_ARG and live_close == live_open, (name, rc, live_open, live_close, rolled)
        if name != "hsk_count_loopback":                                   # (its check of the owner table comes after every block is back)
            assert rolled > 0, (name, rolled)
    assert res["same"] == res["fresh"]


def test_stage_calls_after_a_combining_count_equal_a_fresh_context():
    """hsk_count with the combining extraction leaves nothing of its plan behind (combine_now, item_mode_now: CallState): the stage entry points
    that parse afterwards on the same context give what they give on a fresh one."""
    res, _ = run_worker(dict(mode="stages", tuning="combine_min_bytes=0", ntasks=16, genome=1500000, nreads=400000, seed=77))
    assert res["combine_launches"] > 0, res
    assert res["same"] == res["fresh"]


_TWO_CTX = dict(K=31, M=17, L=2, U=60, ntasks=8)
_TWO_CTX_INPUT = []


def _two_ctx_input():
    """~4000 reads of 150 bases from a 20 kb random genome and the CPU oracle's list of them: made once, shared, never written to"""
    if not _TWO_CTX_INPUT:
        from hysortk_amd import synth
        from oracle import hsk_oracle as O
        dna = synth.packed_reads(20000, 150, 4000, 11)
        p = _TWO_CTX
        _TWO_CTX_INPUT.append((dna, O.count(*dna, k=p["K"], m=p["M"], L=p["L"], U=p["U"], ext=0, ntasks=p["ntasks"], rid_base=0, fast=True)))
    return _TWO_CTX_INPUT[0]


@pytest.mark.parametrize("b_first", [False, True], ids=["A-then-B", "B-then-A"])
def test_two_live_contexts_on_one_thread_each_keep_their_own_tuning(b_first):
    """The tuning table belongs to the context (hsk_ctx::tune), not to the thread or the process: context A ("parse_fast=0": the general parse
    kernels, no scan) and context B (no tuning: the fast scan) are alive together on one thread and are called in turn, A B A B -- whichever was
    created first.  Every call takes its own context's path (hsk_stats::scan_launches) and every list is the CPU oracle's."""
    import numpy as np
    import hysortk_amd as H
    dna, want = _two_ctx_input()
    assert len(want.cnt) > 10000                                            # (30x coverage: nearly every k-mer of the genome is in [L, U])
    kw = dict(profile=True, **_TWO_CTX)
    if b_first:
        b = H.Context(tuning=None, **kw); a = H.Context(tuning="parse_fast=0", **kw)
    else:
        a = H.Context(tuning="parse_fast=0", **kw); b = H.Context(tuning=None, **kw)
    try:
        for i, (c, scans) in enumerate([(a, False), (b, True), (a, False), (b, True)]):
            res = c.count(dna)
            st = c.stats(reset=True)
            print(i, "scan_launches", int(st["scan_launches"]), "entries", len(res.cnt))
            assert (st["scan_launches"] > 0) == scans, (i, st)
            assert np.array_equal(res.task_off, want.task_off) and np.array_equal(res.kmers, want.keys) and np.array_equal(res.cnt, want.cnt), i
    finally:
        a.close(); b.close()
