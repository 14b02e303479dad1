"""Timing of the finishes on skewed input (hsk_agg.h: AggLarge), this build against another build of the library (the parent commit's, given
with --parent; each build runs in a process of its own that loads it through HSK_LIB).  Input: reads of a random genome at 30x, generated on
the GPU, with 5 % of the reads replaced by all-A reads ("polyA") or by (AC)n reads ("AC"), or left alone ("clean"); drop_certain=0, so the
repeat reaches the finish.  Per case and input both builds count the same reads in turn -- parent, new, parent, new, ... --, five timed calls
each after two warm-up calls, result left in HBM (keep_device: no result copy in the numbers).  One JSON to --out; a table to stdout.

usage: python tools/time_large_bins.py --parent /path/to/parent/libhsk.so [--gbp 5] [--out profiles/large_bins.json]
       (worker, started by the driver: --worker K EXT input gbp)"""
import argparse, json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(77, 0), (35, 0), (31, 1), (51, 1)]
INPUTS = ["polyA", "AC", "clean"]
WARMUP, REPS = 2, 5


def worker(K, EXT, kind, gbp):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import hysortk_amd as H
    RL = 150
    n = int(gbp * 1e9 / RL)
    ctx = H.Context(K=K, M=17, L=2, U=65535, EXT=EXT, ntasks=0, keep_device=True, tuning="drop_certain=0")
    dp, nb, do, dl = ctx.synth_reads(n * RL // 30, RL, n, 11)
    keep = None
    if kind != "clean":
        packed = ctx.d2h(dp, nb)
        view = packed.reshape(n, (RL + 3) // 4)
        rng = np.random.default_rng(12)
        view[rng.choice(n, n // 20, replace=False)] = 0x00 if kind == "polyA" else 0x11
        keep = torch.from_numpy(packed).cuda()
        torch.cuda.synchronize()
        dna = H.DeviceDna(ctx, keep.data_ptr(), nb, do, dl, n)
    else:
        dna = H.DeviceDna(ctx, dp, nb, do, dl, n)
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "run":
            break
        try:
            t = time.perf_counter()
            r = dna.count_resident_device()
            dt = (time.perf_counter() - t) * 1e3
            st = ctx.stats()
            print(json.dumps({"ms": dt, "entries": int(r.n), "agg_large_bins": int(st.get("agg_large_bins", 0)), "agg_large_slices": int(st.get("agg_large_slices", 0)),
                              "redone_tasks": int(st["redone_tasks"])}), flush=True)
            r.close()
        except Exception as e:                                   # (out of memory at this size, ...: reported, the driver goes on)
            print(json.dumps({"error": str(e)}), flush=True)
            break
    ctx.synth_free(dp, do, dl)
    ctx.close()


def start(lib, K, EXT, kind, gbp):
    env = dict(os.environ)
    if lib:
        env["HSK_LIB"] = lib
    else:
        env.pop("HSK_LIB", None)
    # (every worker under a time limit of its own; a worker that dies ends the whole run: nothing more is started on the GPU after a fault)
    p = subprocess.Popen(["timeout", "-k", "10", "900", sys.executable, os.path.abspath(__file__), "--worker", str(K), str(EXT), kind, str(gbp)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)
    return p if p.stdout.readline().strip() == "ready" else None


def one(p):
    p.stdin.write("run\n"); p.stdin.flush()
    line = p.stdout.readline()
    return json.loads(line) if line.strip() else {"error": "the worker ended"}


def median(v):
    s = sorted(v)
    return s[len(s) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent"); ap.add_argument("--gbp", type=float, default=5.0); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "large_bins.json"))
    ap.add_argument("--cases", default=",".join("%d:%d" % c for c in CASES)); ap.add_argument("--worker", nargs=4)
    a = ap.parse_args()
    if a.worker:
        return worker(int(a.worker[0]), int(a.worker[1]), a.worker[2], float(a.worker[3]))
    rows = []
    for K, EXT in [tuple(int(x) for x in c.split(":")) for c in a.cases.split(",")]:
        for kind in INPUTS:
            procs = {"parent": start(a.parent, K, EXT, kind, a.gbp), "new": start(None, K, EXT, kind, a.gbp)}
            row = {"K": K, "EXT": EXT, "input": kind, "gbp": a.gbp}
            ok = all(procs.values())
            runs = {b: [] for b in procs}
            for i in range(WARMUP + REPS if ok else 0):
                for b in ("parent", "new"):
                    r = one(procs[b])
                    if "error" in r:
                        row["error_" + b] = r["error"]; ok = False; break
                    if i >= WARMUP:
                        runs[b].append(r)
                if not ok:
                    break
            for b, p in procs.items():
                if p:
                    try:
                        p.stdin.write("quit\n"); p.stdin.flush()
                    except OSError:
                        pass
                    p.wait()
                if ok:
                    ms = [r["ms"] for r in runs[b]]
                    row[b] = {"ms": ms, "median_ms": median(ms), "spread_ms": max(ms) - min(ms), "entries": runs[b][-1]["entries"],
                              "agg_large_bins": runs[b][-1]["agg_large_bins"], "agg_large_slices": runs[b][-1]["agg_large_slices"], "redone_tasks": runs[b][-1]["redone_tasks"]}
            if not ok and "error_parent" not in row and "error_new" not in row:
                row["error"] = "a worker did not start"
            rows.append(row)
            print(json.dumps(row), flush=True)
            with open(a.out, "w") as f:
                json.dump({"what": "tools/time_large_bins.py: ms per call, parent build against this build, 5 % repeat reads against clean reads", "rows": rows}, f, indent=1)
            died = [b for b, p in procs.items() if p is None or p.returncode != 0]
            if died:
                print("worker(s) %s ended badly: stopping here" % died, flush=True)
                sys.exit(1)
    print("| K | EXT | input | parent ms (spread) | new ms (spread) | parent skewed/clean | new skewed/clean |")
    clean = {(r["K"], r["EXT"]): r for r in rows if r["input"] == "clean" and "new" in r}
    for r in rows:
        if "new" not in r:
            continue
        c = clean.get((r["K"], r["EXT"]))
        rat = lambda b: "%.2f" % (r[b]["median_ms"] / c[b]["median_ms"]) if c else "-"
        print("| %d | %d | %s | %.1f (%.1f) | %.1f (%.1f) | %s | %s |" % (r["K"], r["EXT"], r["input"], r["parent"]["median_ms"], r["parent"]["spread_ms"], r["new"]["median_ms"], r["new"]["spread_ms"], rat("parent"), rat("new")))


if __name__ == "__main__":
    main()
