"""Helper of tests/test_gpu_calls.py: `python _calls_worker.py <json>`, run under HSK_TIMING=1 (every entry point's scope prints one line when it
closes: name, status, device-pool bytes live when it opened and when it closed, blocks rolled back).  Prints one JSON line.

mode "failures": on one context, calls that fail after they have allocated (hsk_count_loopback with too small an owner table after a full
run, hsk_stage_count_sorted / hsk_stage_task_kmers with too small a capacity, hsk_format_entries with too small a text buffer), then hsk_count
on the same context and on a fresh one.
mode "stages": hsk_count on reads in HBM with the combining extraction, then hsk_stage_task_kmers for every task and hsk_stage_destinations on
the same context, and the same stages on a fresh context."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hysortk_amd as H  # noqa: E402
from hysortk_amd import _lib, synth  # noqa: E402
from hysortk_amd.api import _p  # noqa: E402


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def count_digest(r):
    return digest(r.kmers, r.cnt, r.task_off, r.histo)


def failures(spec):
    packed, off, lens = synth.packed_reads(20000, 150, 4000, 3)
    cfg = dict(K=31, M=17, L=2, U=40, ntasks=5, tuning=spec.get("tuning"))
    out = {}
    with H.Context(**cfg) as c:
        lib, h = c.lib, c.h
        half, nbr = len(lens) // 2, (150 + 3) // 4
        dnas = [(packed[:half * nbr], off[:half], lens[:half]), (packed[half * nbr:], off[:half], lens[half:])]
        c.count_loopback(dnas)                                              # a full run (its results are freed)
        pk = [np.ascontiguousarray(d[0]) for d in dnas]; of = [np.ascontiguousarray(d[1]) for d in dnas]; ln = [np.ascontiguousarray(d[2]) for d in dnas]
        PP = (C.c_void_p * 2)(*[x.ctypes.data for x in pk]); OP = (C.c_void_p * 2)(*[x.ctypes.data for x in of]); LP = (C.c_void_p * 2)(*[x.ctypes.data for x in ln])
        nb = np.array([x.size for x in pk], dtype=np.uint64); nr = np.array([x.size for x in ln], dtype=np.uint64)
        outs = (_lib.Result * 2)()
        owner = np.zeros(1, dtype=np.int32)
        out["hsk_count_loopback"] = lib.hsk_count_loopback(h, 2, PP, _p(nb), OP, LP, _p(nr), outs, _p(owner), 1)

        distinct = np.unique(np.random.default_rng(1).integers(0, 1 << 62, 5000, dtype=np.uint64))
        keys = np.ascontiguousarray(np.repeat(distinct, 3))                # three copies each: inside [L, U]
        ent = np.zeros((keys.size, 2), dtype=np.uint64)
        m = C.c_uint64(0)
        out["hsk_stage_count_sorted"] = lib.hsk_stage_count_sorted(h, _p(keys), keys.size, 1, _p(ent), 10, C.byref(m))

        kbuf = np.zeros((16, 1), dtype=np.uint64)
        n = C.c_uint64(0)
        out["hsk_stage_task_kmers"] = lib.hsk_stage_task_kmers(h, _p(packed), packed.size, _p(off), _p(lens), lens.size, 0, 0, _p(kbuf), None, None, 1, C.byref(n))

        e = np.zeros((100, 2), dtype=np.uint64); e[:, 0] = np.arange(100, dtype=np.uint64) * 977; e[:, 1] = 5
        text = np.zeros(8, dtype=np.uint8)
        need = C.c_uint64(0)
        out["hsk_format_entries"] = lib.hsk_format_entries(h, _p(e), 100, 1, 0, _p(text), text.size, C.byref(need))

        out["same"] = count_digest(c.count((packed, off, lens)))
    with H.Context(**cfg) as c:
        out["fresh"] = count_digest(c.count((packed, off, lens)))
    return out


def stages(spec):
    cfg = dict(K=31, M=17, L=1, U=200, ntasks=spec["ntasks"], profile=True, tuning=spec.get("tuning"))
    n = spec["nreads"]
    out = {}

    def run_stages(c, reads):
        d = [digest(np.sort(c.stage_task_kmers(reads, t)[0], axis=0)) for t in range(spec["ntasks"])]
        dest, doff = c.stage_destinations(reads)
        return d + [digest(dest, doff)]

    with H.Context(**cfg) as c:
        dp, nb, do, dl = c.synth_reads(spec["genome"], 150, n, spec["seed"])
        reads = (np.empty(nb, np.uint8), np.empty(n, np.uint64), np.empty(n, np.uint32))
        c.d2h_into(reads[0], dp, nb); c.d2h_into(reads[1], do, n * 8); c.d2h_into(reads[2], dl, n * 4)
        c.stats(reset=True)
        c.count_device(dp, nb, do, dl, n)
        out["combine_launches"] = int(c.stats(reset=True)["combine_launches"])
        c.synth_free(dp, do, dl)
        out["same"] = run_stages(c, reads)
    with H.Context(**cfg) as c:
        out["fresh"] = run_stages(c, reads)
    return out


if __name__ == "__main__":
    spec = json.loads(sys.argv[1])
    print(json.dumps({"failures": failures, "stages": stages}[spec["mode"]](spec)), flush=True)
