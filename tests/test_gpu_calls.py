"""One scope per entry point (ApiCall, hysortk_amd/csrc/hsk_api.hip): a call that fails after it has allocated hands every device block back
(live bytes at its close = live bytes at its open, HSK_TIMING's line per call), and nothing of one call's state (CallState) reaches the next:
a count on the same context afterwards equals a fresh context's, and so do the stage entry points after a count that took the combining
extraction."""
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
