"""Timing of hsk_result_pairs (read pairs that share k-mers, from the resident EXTENSION list).

Workload: reads of a random genome generated in HBM (hsk_synth_reads): G = 8 Mbp, 150-bp reads, 20x, K = 31, L = 2, U = 50, EXTENSION,
KEEP_DEVICE.  Counted once; then hsk_result_pairs over all tasks, 2 warm-up calls and 5 timed ones (rows left on the device, so that the
numbers are the stage's; one more call with the rows copied to the host gives ms_d2h).  Per phase: the HIP-event timers of the call, the
algorithmic bytes (expansion: 16 B written per record; sort: 32 B per record and scatter pass plus 8 B per record for the histogram;
reducer: 16 B read per record) and the GB/s they make, against hsk_copy_peak measured in the same process.  For context, what a client
has to do without the stage before it can start pairing: DeviceResult.fetch of every task (wall clock).

usage: python tools/time_pairs.py [--gbp 0.008] [--coverage 20] [--out profiles/pairs_8mbp.json]"""
import argparse, json, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, REPS = 2, 5


def median(v):
    s = sorted(v)
    return s[len(s) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbp", type=float, default=0.008); ap.add_argument("--coverage", type=float, default=20.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs_8mbp.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import hysortk_amd as H
    RL = 150
    G = int(a.gbp * 1e9)
    n = int(G * a.coverage / RL)
    ctx = H.Context(K=31, M=17, L=2, U=50, EXT=1, ntasks=0, keep_device=True)
    peak = ctx.copy_peak(1 << 30, 3)
    dp, nb, do, dl = ctx.synth_reads(G, RL, n, 11)
    dna = H.DeviceDna(ctx, dp, nb, do, dl, n)
    t0 = time.perf_counter()
    dev = dna.count_resident_device()
    count_ms = (time.perf_counter() - t0) * 1e3
    runs = []
    for i in range(WARMUP + REPS):
        t0 = time.perf_counter()
        with dev.pairs(on_device=True) as rp:
            info = dict(rp.info, rows=rp.n, wall_ms=(time.perf_counter() - t0) * 1e3)
        if i >= WARMUP:
            runs.append(info)
    host = dev.pairs()
    last = runs[-1]
    rec, passes = last["records"], last["sort_passes"]
    nbytes = {"expand": 16 * rec, "sort": 32 * rec * passes + 8 * rec, "reduce": 16 * rec}
    phases = {}
    for ph in ("expand", "sort", "reduce"):
        ms = [r["ms_" + ph] for r in runs]
        m = median(ms)
        phases[ph] = {"ms": ms, "median_ms": m, "bytes": nbytes[ph], "gbs": nbytes[ph] / (m * 1e-3) / 1e9 if m > 0 else 0.0,
                      "of_copy_peak": nbytes[ph] / (m * 1e-3) / 1e9 / peak if m > 0 and peak > 0 else 0.0}
    # the parent commit's way to the payload: every task's CSR across PCIe
    t0 = time.perf_counter()
    fetched = 0
    for t in range(dev.ntasks):
        d = dev.fetch(t)
        fetched += d["n"] * (dev.nw + 1) * 8 + d["n"] * 8 + d["npay"] * 8
    fetch_ms = (time.perf_counter() - t0) * 1e3
    out = {"what": "tools/time_pairs.py: hsk_result_pairs over all tasks of a resident EXTENSION result",
           "workload": {"genome_bp": G, "read_len": RL, "reads": n, "K": 31, "M": 17, "L": 2, "U": 50, "ntasks": dev.ntasks, "entries": dev.n, "count_call_wall_ms": count_ms},
           "records": rec, "self_records": last["self_records"], "keys": last["keys"], "rows": last["rows"], "sort_passes": passes,
           "copy_peak_gbs": peak, "phases": phases,
           "ms_total": {"ms": [r["ms_total"] for r in runs], "median_ms": median([r["ms_total"] for r in runs])},
           "wall_ms": {"ms": [r["wall_ms"] for r in runs], "median_ms": median([r["wall_ms"] for r in runs])},
           "rows_to_host": {"ms_d2h": host.info["ms_d2h"], "ms_total": host.info["ms_total"], "bytes": len(host) * 32},
           "fetch_every_task": {"wall_ms": fetch_ms, "bytes": fetched}}
    dev.close()
    ctx.synth_free(dp, do, dl)
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
