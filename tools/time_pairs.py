"""Timing of hsk_result_pairs, hsk_result_pairs_sliced and hsk_pairs_merge (read pairs that share k-mers, from the resident EXTENSION list;
DESIGN sections 6.7 and 6.7b).

Workload: reads of a random genome generated in HBM (hsk_synth_reads): G = 8 Mbp, 150-bp reads, 20x, K = 31, L = 2, U = 50, EXTENSION,
KEEP_DEVICE.  Counted once; then hsk_result_pairs over all tasks, 2 warm-up calls and 5 timed ones (rows left on the device, so that the
numbers are the stage's; one more call with the rows copied to the host gives ms_d2h).  Per phase: the HIP-event timers of the call, the
algorithmic bytes (expansion: 16 B written per record; sort: 32 B per record and scatter pass plus 8 B per record for the histogram;
reducer: 16 B read per record) and the GB/s they make, against hsk_copy_peak measured in the same process.  For context, what a client
has to do without the stage before it can start pairing: DeviceResult.fetch of every task (wall clock).

--max-records N (repeatable; N a number of records, a fraction of the range's records such as 1/4, or 0 for the library's choice): the
same timing of hsk_result_pairs_sliced with that budget, its slices and merges, the ratio of its time to the unsliced call's, and its rows
compared with the unsliced rows.  Where the unsliced call does not fit the device its error is recorded and the sliced runs stand alone.
--merge-only: the lists of the two halves of the task range, left on the device, merged by hsk_pairs_merge: the merge kernels' time and
GB/s (32 B read per input row, 32 B written per output row) against hsk_copy_peak.

--oriented: hsk_result_strands (the strand of every payload slot, from the reads in HBM), then hsk_result_pairs and
hsk_result_pairs_oriented on the same resident result: the ms of each, the sort passes of both pair calls, the ratio of the oriented call
to the plain one, and the oriented rows folded and compared with the plain rows.  --strands-only (with --oriented): the strand pass alone --
with --gbp it shows how the pass scales with the size of the packed reads it gathers from (the entry lookup per payload slot is the same).

--diagonals [--diag-bin W]: on the input of --oriented, hsk_result_pairs_oriented (single pass) and hsk_result_pair_diagonals (best bin and
all bins, W diagonals per bin) on the same resident result, side by side: the ms of each call and phase, the sort passes, the ratio to the
oriented call, and the rows compared -- the selection of the all-bins list with the best-bin list, the all-bins list folded by key with the
oriented list.  The oriented call is the yardstick: per record and scatter pass the sort moves 48 bytes (two key words and the value) where
it moves 32.  Writes profiles/pairs_diagonals_8mbp.json unless --out says otherwise.
--diagonals --max-records N (repeatable, N as above): hsk_result_pair_diagonals_sliced with that budget against the single pass of the same
run -- best bin and all bins, the slices and merges, the merges' GB/s (48 B read per input row; the output rows are not counted: a lower
bound) against hsk_copy_peak, the rows compared with the single pass -- and the device join of the all-bins lists of the two halves of the
task range (hsk_pair_diags_merge, lists in HBM) against what it replaces: both lists copied to the host and PairDiagonals.combine there, with
and without the selection.  Where the single pass is refused (HSK_ERR_OOM: --gbp 0.096), its error is recorded and the sliced runs with a
budget that needs no record count (a number, or 0) stand alone, with what the device holds after them.  Writes
profiles/pairs_diagonals_sliced_8mbp.json unless --out says otherwise.

--extend [--error-rate R]: on the input of --diagonals, with reads generated with substitution errors (default 0.01) so that the extension
has something to stop at: hsk_result_pair_diagonals (best bin, rows left in HBM) and hsk_pair_diags_extend of those rows (reads and result in
HBM) side by side -- the ms of each and their ratio, columns, wave_rows, and the bytes of reads the overlaps cover (two bits per base and
read: columns / 2) per ms against hsk_copy_peak of the same run.  The host route it replaces, as a SAMPLE: the rows copied to the host, the
packed reads copied to the host, and tests/extend_ref.py (numpy, one column per step) on --sample rows, which are also compared with the
device's rows.  Then a wave_span sweep (1, 512, 4096, none) on a long-read input (--long-reads reads of --long-len bases).  Writes
profiles/pairs_extend_8mbp.json unless --out says otherwise.

--gapped [--band B ...] [--indel-rate R] [--error-rate R]: the gapped call beside the ungapped one.  The reads are made on the HOST -- fixed
spans of a random genome, both strands, substitutions (--error-rate, default 0.01) and indels (--indel-rate, default 0.005: half
insertions, half deletions), so their lengths differ; the device generator has substitutions only and stays as it is --, written as FASTA
and packed on the GPU (hsk_pack_fasta).  The diagonal rows come from the pipeline (count, strands, hsk_result_pair_diagonals, best bin, left
in HBM).  Timed in one run: hsk_result_pair_diagonals, hsk_pair_diags_extend, and hsk_pair_diags_extend_gapped for every --band (default 7,
15, 31; the library's group width), with ms, live cells and live cells per second; a sample of --gapped-sample rows of every band is
compared with tests/gapped_ref.py, and how many overlaps are longer than the ungapped ones is counted.  Writes
profiles/pairs_gapped_8mbp.json unless --out says otherwise.

--reduce [--band B] [--pile P] [--pile-lane-only]: the string graph (hsk_overlaps_reduce) of the overlap rows of the --gapped workload (band B,
default 15), rows and lengths in HBM.  Timed in one run: hsk_result_pair_diagonals, hsk_pair_diags_extend_gapped, the reduction with its
phases and counts (rows per class, arcs, largest degree, the kept rows' bytes against the input's), the copy of the input rows alone to the
host (what the host route pays before it starts), a wave_degree sweep (1, 64, 256, 1024, none), the rows kept at fuzz 0 / 10 / 100, and the
same sweep with a staggered pile of --pile reads (default 3000) of one length behind the reads, whose rows are fabricated
(tests/strgraph_ref.py: every pair of the pile is a dovetail, so its vertices have up to P - 1 out-arcs); `none` on the pile only with
--pile-lane-only (its deg^2 walk takes long).  Writes profiles/overlaps_reduce_8mbp.json unless --out says otherwise.

--unitigs [--band B] [--synthetic-reads N]: the unitigs (hsk_overlaps_unitigs) of the --reduce workload's string graph, everything resident:
gapped overlaps, hsk_overlaps_reduce with on_device, then the unitigs of that graph.  Timed in one run, --reps repetitions after the warm-up,
every time with its median, smallest and largest: the unitigs call and its phases, the reduce call and its phases, and the host route the
call replaces -- the kept rows and the contained bits over PCIe plus OverlapGraph.arcs (wall clock) --, with the walk a client would then
do timed once behind it (numpy and one Python step per link).  Then a synthetic line and a ring of N reads (default 10^6) on random strands:
one chain through every read, where a sequential walk is one chase of N steps.  Writes profiles/overlaps_unitigs_8mbp.json unless --out
says otherwise.

usage: python tools/time_pairs.py [--gbp 0.008] [--coverage 20] [--max-records N ...] [--merge-only] [--oriented [--strands-only]] [--diagonals [--diag-bin W] [--max-records N ...]] [--extend [--error-rate R]] [--gapped [--band B ...] [--indel-rate R]] [--out profiles/pairs_8mbp.json]"""
import argparse, json, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, REPS = 2, 5


def median(v):
    s = sorted(v)
    return s[len(s) // 2]


def timed(call, warmup=WARMUP, reps=REPS):
    """info dicts of `reps` calls after `warmup` calls; the rows stay on the device and go back after every call."""
    runs = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        with call() as rp:
            info = dict(rp.info, rows=rp.n, wall_ms=(time.perf_counter() - t0) * 1e3)
        if i >= warmup:
            runs.append(info)
    return runs


def summary(runs):
    """what the timed calls of one kind say: the counts of the last one, the medians of the call and of its phases"""
    last = runs[-1]
    s = {"records": last["records"], "self_records": last["self_records"], "keys": last["keys"], "rows": last["rows"], "sort_passes": last["sort_passes"],
         "ms_total": [r["ms_total"] for r in runs], "median_ms": median([r["ms_total"] for r in runs])}
    if "bins" in last:
        s["bins"] = last["bins"]
    for ph in ("expand", "sort", "reduce"):
        s["median_ms_" + ph] = median([r["ms_" + ph] for r in runs])
    return s


def budget(text, records):
    if "/" in text:
        p, q = text.split("/")
        return max(1, records * int(p) // int(q))
    return int(text)


def sliced_alone(H, ctx, dev, st, W, a):
    """hsk_result_pair_diagonals_sliced where the single pass is refused: every budget that needs no record count (numbers, 0), both lists,
    and what the device holds when the call is over (what the runtime reports used: the context's pool keeps its blocks, so this is the
    high-water mark of the process, the resident result and the reads included)."""
    res = []
    for text in a.max_records:
        if "/" in text:
            continue
        m, s = int(text), {"max_records": int(text), "asked": text}
        for name, all_bins in (("best_bin", False), ("all_bins", True)):
            runs = timed(lambda: dev.pair_diagonals(st, W, all_bins=all_bins, on_device=True, max_records=m), reps=a.reps)
            last = runs[-1]
            s[name] = {k: last[k] for k in ("records", "self_records", "rows", "keys", "bins", "slices", "peak_records", "merges", "merged_rows", "sort_passes")}
            s[name].update({"ms_total": [r["ms_total"] for r in runs], "median_ms": median([r["ms_total"] for r in runs]),
                            "ms_merge": [r["ms_merge"] for r in runs], "wall_ms": [r["wall_ms"] for r in runs]})
        try:                                             # the HIP runtime the library has initialised in this process
            import ctypes
            fr, tot = ctypes.c_size_t(), ctypes.c_size_t()
            rc = ctypes.CDLL("libamdhip64.so").hipMemGetInfo(ctypes.byref(fr), ctypes.byref(tot))
            s["device_bytes_used_after"], s["device_bytes_total"] = (int(tot.value - fr.value), int(tot.value)) if rc == 0 else (None, None)
        except OSError:
            s["device_bytes_used_after"] = None
        res.append(s)
    return res


def unpack_reads(np, packed, off, lens, ids):
    """(code matrix, lengths) of the reads `ids` of a packed buffer, as tests/extend_ref.code_matrix gives them for strings"""
    lens = lens[ids].astype(np.int64)
    m = np.zeros((ids.size, max(1, int(lens.max()) if ids.size else 1)), dtype=np.int64)
    for i, (o, n) in enumerate(zip(off[ids].tolist(), lens.tolist())):
        b = packed[o:o + (n + 3) // 4]
        m[i, :n] = np.stack([(b >> 6) & 3, (b >> 4) & 3, (b >> 2) & 3, b & 3], axis=1).reshape(-1)[:n]
    return m, lens


def extend_summary(runs, peak):
    last = runs[-1]
    ms = median([r["ms_extend"] for r in runs])
    gbs = last["columns"] / 2 / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
    return {"rows": last["rows"], "input_rows": last["input_rows"], "columns": last["columns"], "wave_rows": last["wave_rows"], "dropped": last["dropped"],
            "ms_extend": [r["ms_extend"] for r in runs], "median_ms_extend": ms, "ms_total": [r["ms_total"] for r in runs], "median_ms": median([r["ms_total"] for r in runs]),
            "wall_ms": [r["wall_ms"] for r in runs], "read_bytes_covered": last["columns"] // 2, "read_gbs": gbs, "read_of_copy_peak": gbs / peak if peak > 0 else 0.0}


def extend_sweep(H, a, peak):
    """the wave_span sweep on long reads, in a context of its own: (workload, {wave_span: summary}, rows equal over the sweep)"""
    import numpy as np
    G, RL, n = a.long_len * a.long_reads // 8, a.long_len, a.long_reads      # 8x
    ctx = H.Context(K=31, M=17, L=2, U=50, EXT=1, ntasks=0, keep_device=True)
    dp, nb, do, dl = ctx.synth_reads(G, RL, n, 13, error_rate=a.error_rate)
    dna = H.DeviceDna(ctx, dp, nb, do, dl, n)
    res, base, same = {}, None, True
    with dna.count_resident_device() as dev, dev.strands(dna) as st, dev.pair_diagonals(st, a.diag_bin, on_device=True) as pd:
        for span in (1, 512, 4096, 0xFFFFFFFF):
            res[str(span)] = extend_summary(timed(lambda: pd.extend(ctx, dna, wave_span=span, on_device=True), reps=a.reps), peak)
            rows = pd.extend(ctx, dna, wave_span=span).rows()
            same = same and (base is None or bool(np.array_equal(rows, base)))
            base = rows
        work = {"genome_bp": G, "read_len": RL, "reads": n, "error_rate": a.error_rate, "diagonal_rows": pd.n, "records": pd.info["records"]}
    ctx.synth_free(dp, do, dl)
    ctx.close()
    return work, res, same


def host_reads_fasta(np, path, G, RL, n, sub, indel, seed):
    """n reads as a FASTA file with its .fai: spans of RL bases of a random genome of G bases, half of them reverse-complemented, with
    substitutions and indels (an insertion in front of a base, or the base deleted).  One line per record."""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, G, dtype=np.uint8)
    lens = np.zeros(n, np.int64)
    parts = []
    for lo in range(0, n, 1 << 17):                      # in blocks: the per-base random numbers of all reads at once are large
        m = min(1 << 17, n - lo)
        start = rng.integers(0, G - RL, m)
        base = genome[start[:, None] + np.arange(RL)[None, :]]
        rev = rng.integers(0, 2, m).astype(bool)
        base[rev] = 3 - base[rev][:, ::-1]
        u = rng.random((m, RL))
        hit = (u >= indel) & (u < indel + sub)
        base[hit] = (base[hit] + rng.integers(1, 4, int(hit.sum()), dtype=np.uint8)) & 3
        emit = np.stack([rng.integers(0, 4, (m, RL), dtype=np.uint8), base], axis=2)                # (an inserted base, the base)
        valid = np.stack([(u >= indel / 2) & (u < indel), u >= indel / 2], axis=2)
        parts.append(emit[valid])                        # row-major: every read's bases in order
        lens[lo:lo + m] = valid.sum(axis=(1, 2))
    codes = np.concatenate(parts)
    rec = np.concatenate([[0], np.cumsum(lens + 4)])     # ">r\n" + bases + "\n"
    text = np.full(int(rec[-1]), 10, np.uint8)
    text[rec[:-1]], text[rec[:-1] + 1] = ord(">"), ord("r")
    flat = np.concatenate([[0], np.cumsum(lens)])
    text[np.repeat(rec[:-1] + 3 - flat[:-1], lens) + np.arange(codes.size)] = np.frombuffer(b"ACGT", np.uint8)[codes]
    text.tofile(path)
    with open(path + ".fai", "w") as f:
        f.write("".join("r\t%d\t%d\t%d\t%d\n" % (L, o + 3, L, L + 1) for L, o in zip(lens.tolist(), rec[:-1].tolist())))
    return lens


def gapped_run(H, a):
    """--gapped: see the module's text"""
    import shutil, tempfile
    import numpy as np
    from tests import gapped_ref as GR
    RL, G = 150, int(a.gbp * 1e9)
    n = int(G * a.coverage / RL)
    bands = a.band or [7, 15, 31]
    ctx = H.Context(K=31, M=17, L=2, U=50, EXT=1, ntasks=0, keep_device=True)
    peak = ctx.copy_peak(1 << 30, 3)
    tmp = tempfile.mkdtemp()
    try:
        t0 = time.perf_counter()
        lens = host_reads_fasta(np, os.path.join(tmp, "reads.fa"), G, RL, n, a.error_rate, a.indel_rate, 11)
        make_ms = (time.perf_counter() - t0) * 1e3
        dna = H.read_dna_buffer_device(ctx, os.path.join(tmp, "reads.fa"))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    dev = dna.count_resident_device()
    out = {"what": "tools/time_pairs.py --gapped: hsk_result_pair_diagonals (best bin), hsk_pair_diags_extend and hsk_pair_diags_extend_gapped of its rows, rows and reads in HBM; one run on one card",
           "workload": {"genome_bp": G, "read_span": RL, "reads": n, "read_len_min": int(lens.min()), "read_len_max": int(lens.max()), "bases": int(lens.sum()), "error_rate": a.error_rate,
                        "indel_rate": a.indel_rate, "K": 31, "M": 17, "L": 2, "U": 50, "ntasks": dev.ntasks, "entries": dev.n, "host_reads_wall_ms": make_ms},
           "scores": {"match": 1, "mismatch": 1, "gap": 1, "xdrop": 7}, "diag_bin": a.diag_bin, "copy_peak_gbs": peak, "reps": a.reps}
    with dev.strands(dna) as st:
        diag = summary(timed(lambda: dev.pair_diagonals(st, a.diag_bin, on_device=True), reps=a.reps))
        with dev.pair_diagonals(st, a.diag_bin, on_device=True) as pd:
            ung = extend_summary(timed(lambda: pd.extend(ctx, dna, on_device=True), reps=a.reps), peak)
            hrows = ctx.d2h(pd.rows_dev, pd.n * 48).view(np.uint64).reshape(pd.n, 6)
            packed, off = dna.packed(), ctx.d2h(dna.do, n * 8).view(np.uint64)
            pick = np.sort(np.random.default_rng(1).choice(pd.n, min(a.gapped_sample, pd.n), replace=False))
            srows = hrows[pick].copy()
            ids = np.concatenate([(srows[:, 0] >> np.uint64(32)) & np.uint64(0x7FFFFFFF), srows[:, 0] & np.uint64(0xFFFFFFFF)]).astype(np.int64)
            uniq, inv = np.unique(ids, return_inverse=True)
            srows[:, 0] = (srows[:, 0] & (np.uint64(1) << np.uint64(63))) | (inv[:pick.size].astype(np.uint64) << np.uint64(32)) | inv[pick.size:].astype(np.uint64)
            mat = unpack_reads(np, packed, off.astype(np.int64), lens.astype(np.uint32), uniq)
            urows = pd.extend(ctx, dna).rows()
            lo = np.uint64(0xFFFFFFFF)
            ulen = (urows[:, 2] & lo) - (urows[:, 2] >> np.uint64(32))
            by_band = {}
            for b in bands:
                runs = timed(lambda: pd.extend_gapped(ctx, dna, band=b, on_device=True), reps=a.reps)
                s = extend_summary(runs, peak)
                s["cells"] = runs[-1]["cells"]
                s["cells_per_s"] = s["cells"] / (s["median_ms_extend"] * 1e-3) if s["median_ms_extend"] > 0 else 0.0
                s["group"] = 8 if b < 8 else 16 if b < 16 else 32 if b < 32 else 64
                grows = pd.extend_gapped(ctx, dna, band=b).rows()
                glen, gblen = (grows[:, 2] & lo) - (grows[:, 2] >> np.uint64(32)), (grows[:, 3] & lo) - (grows[:, 3] >> np.uint64(32))
                s["rows_longer_than_ungapped"], s["rows_shorter_than_ungapped"], s["rows_whose_spans_differ"] = int((glen > ulen).sum()), int((glen < ulen).sum()), int((glen != gblen).sum())
                s["edits"] = int((grows[:, 4] >> np.uint64(32)).sum())
                t0 = time.perf_counter()
                want, _, _ = GR.extend_rows_bulk(srows, mat, 31, band=b)
                s["sample"] = {"rows": int(pick.size), "reference_wall_ms": (time.perf_counter() - t0) * 1e3,
                               "device_rows_equal_reference": bool(np.array_equal(grows[pick][:, 1:], want[:, 1:]) and np.array_equal(grows[pick][:, 0], hrows[pick, 0]))}
                s["over_ungapped"] = s["median_ms_extend"] / ung["median_ms_extend"] if ung["median_ms_extend"] > 0 else None
                s["over_pair_diagonals"] = s["median_ms"] / diag["median_ms"] if diag["median_ms"] > 0 else None
                by_band[str(b)] = s
                print("%-40s %10.3f ms (kernels %.3f), %d cells, %.3g cells/s, %d of %d rows longer than ungapped, sample equal: %s" % (
                    "hsk_pair_diags_extend_gapped band %d" % b, s["median_ms"], s["median_ms_extend"], s["cells"], s["cells_per_s"], s["rows_longer_than_ungapped"], pd.n, s["sample"]["device_rows_equal_reference"]))
    out["pair_diagonals"], out["extend"], out["extend_gapped"] = diag, ung, by_band
    print("%-40s %10.3f ms, %d rows" % ("hsk_result_pair_diagonals", diag["median_ms"], diag["rows"]))
    print("%-40s %10.3f ms (kernels %.3f), %d columns" % ("hsk_pair_diags_extend", ung["median_ms"], ung["median_ms_extend"], ung["columns"]))
    dev.close()
    dna.free()
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


def reduce_run(H, a):
    """--reduce: see the module's text"""
    import shutil, tempfile
    import numpy as np
    from tests import strgraph_ref as SR
    RL, G, NONE = 150, int(a.gbp * 1e9), 0xFFFFFFFF
    n = int(G * a.coverage / RL)
    band = (a.band or [15])[0]
    ctx = H.Context(K=31, M=17, L=2, U=50, EXT=1, ntasks=0, keep_device=True)
    peak = ctx.copy_peak(1 << 30, 3)
    tmp = tempfile.mkdtemp()
    try:
        lens = host_reads_fasta(np, os.path.join(tmp, "reads.fa"), G, RL, n, a.error_rate, a.indel_rate, 11)
        dna = H.read_dna_buffer_device(ctx, os.path.join(tmp, "reads.fa"))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    dev = dna.count_resident_device()
    out = {"what": "tools/time_pairs.py --reduce: hsk_overlaps_reduce of the rows of hsk_pair_diags_extend_gapped (band %d), rows and lengths in HBM, beside the calls that make the rows; one run on one card" % band,
           "workload": {"genome_bp": G, "read_span": RL, "reads": n, "read_len_min": int(lens.min()), "read_len_max": int(lens.max()), "error_rate": a.error_rate, "indel_rate": a.indel_rate,
                        "K": 31, "M": 17, "L": 2, "U": 50, "band": band}, "copy_peak_gbs": peak, "reps": a.reps}
    phases = ("ms_total", "ms_classify", "ms_sort", "ms_reduce", "ms_d2h")

    def run(src, reads, **kw):
        """the counts of the last of `reps` calls after the warm-up, and the median of every phase"""
        infos = []
        for i in range(WARMUP + a.reps):
            with src.reduce(ctx, reads, on_device=True, **kw) as g:
                infos.append(dict(g.info, rows=len(g)))
        s = {k: v for k, v in infos[-1].items() if not k.startswith("ms_")}
        s.update({"median_" + ph: median([r[ph] for r in infos[WARMUP:]]) for ph in phases})
        s["median_ms_kernels"] = median([r["ms_classify"] + r["ms_sort"] + r["ms_reduce"] for r in infos[WARMUP:]])
        return s

    with dev.strands(dna) as st:
        diag = summary(timed(lambda: dev.pair_diagonals(st, a.diag_bin, on_device=True), reps=a.reps))
        with dev.pair_diagonals(st, a.diag_bin, on_device=True) as pd:
            gap = extend_summary(timed(lambda: pd.extend_gapped(ctx, dna, band=band, on_device=True), reps=a.reps), peak)
            with pd.extend_gapped(ctx, dna, band=band, on_device=True) as ov:
                walls = []
                for i in range(WARMUP + a.reps):          # what the host route pays before it starts: the rows over PCIe
                    t0 = time.perf_counter()
                    hrows = ctx.d2h(ov.rows_dev, ov.n * 48)
                    walls.append((time.perf_counter() - t0) * 1e3)
                hrows = hrows.view(np.uint64).reshape(ov.n, 6)
                out["input_rows_d2h"] = {"bytes": ov.n * 48, "median_wall_ms": median(walls[WARMUP:]), "note": "into pageable host memory"}
                red = run(ov, dna)
                red["kept_bytes"], red["input_bytes"] = red["rows"] * 48, ov.n * 48
                out["sweep_wave_degree"] = {str(wd): run(ov, dna, wave_degree=wd) for wd in (1, 64, 256, 1024, NONE)}
                out["kept_by_fuzz"] = {str(f): run(ov, dna, fuzz=f)["kept"] for f in (0, 10, 100)}
        # a staggered pile of reads of one length behind the reads -- what a tandem repeat shorter than the reads does: every pair of the
        # pile is a dovetail, its vertices have up to pile - 1 out-arcs.  The rows are fabricated (no bases are read) and uploaded per call.
        P = a.pile
        pile = SR.layout_rows(np.arange(P), np.full(P, P + RL), np.random.default_rng(5).integers(0, 2, P), 31, rid_base=n)
        both = H.Overlaps.from_rows(np.concatenate([hrows, pile]))
        lens2 = np.concatenate([lens, np.full(P, P + RL)]).astype(np.uint32)
        out["sweep_wave_degree_with_pile"] = {"pile_reads": P, "pile_rows": int(pile.shape[0]), "note": "host rows, uploaded by every call: compare median_ms_kernels",
                                              "runs": {str(wd): run(both, lens2, wave_degree=wd) for wd in (1, 64, 256, 1024, NONE)[:None if a.pile_lane_only else -1]}}
    out["pair_diagonals"], out["extend_gapped"], out["overlaps_reduce"] = diag, gap, red
    print("%-40s %10.3f ms, %d rows" % ("hsk_result_pair_diagonals", diag["median_ms"], diag["rows"]))
    print("%-40s %10.3f ms (kernels %.3f)" % ("hsk_pair_diags_extend_gapped", gap["median_ms"], gap["median_ms_extend"]))
    print("%-40s %10.3f ms (classify %.3f, sort %.3f, reduce %.3f), %d of %d rows kept, %d arcs, max degree %d; the rows alone to the host: %.3f ms" % (
        "hsk_overlaps_reduce", red["median_ms_total"], red["median_ms_classify"], red["median_ms_sort"], red["median_ms_reduce"], red["rows"], red["input_rows"], red["arcs"], red["max_degree"],
        out["input_rows_d2h"]["median_wall_ms"]))
    for name in ("sweep_wave_degree", "sweep_wave_degree_with_pile"):
        runs = out[name].get("runs", out[name])
        print(name + ": " + ", ".join("%s: %.3f ms" % (wd, s["median_ms_kernels"]) for wd, s in runs.items()))
    dev.close()
    dna.free()
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


def spread(v):
    """the median, the smallest and the largest of the timed repetitions"""
    return {"median": median(v), "min": min(v), "max": max(v), "all": list(v)}


def host_walk(np, v, w, nv):
    """what a client does with OverlapGraph.arcs: degrees, links, and one pointer chase per chain (numpy, then a Python loop per link);
    returns (chains, the longest chain's vertices)"""
    pair = np.unique(v.astype(np.int64) << 32 | w.astype(np.int64))
    pv, pw = pair >> 32, pair & 0xFFFFFFFF
    deg = np.bincount(pv, minlength=nv)
    link = (deg[pv] == 1) & (deg[pw ^ 1] == 1)
    succ = np.full(nv, -1, np.int64)
    succ[pv[link]] = pw[link]
    has_pred = np.zeros(nv, bool)
    has_pred[pw[link]] = True
    succ_l, seen = succ.tolist(), np.zeros(nv, bool)
    chains = longest = 0
    for h in np.flatnonzero(~has_pred).tolist() + np.flatnonzero(has_pred).tolist():      # the paths from their heads, then what is left: the cycles
        if seen[h]:
            continue
        x, k = h, 0
        while x >= 0 and not seen[x]:
            seen[x] = True
            x, k = succ_l[x], k + 1
        chains, longest = chains + 1, max(longest, k)
    return chains, longest


def unitigs_run(H, a):
    """--unitigs: see the module's text"""
    import shutil, tempfile
    import numpy as np
    from tests import strgraph_ref as SR
    RL, G = 150, int(a.gbp * 1e9)
    n = int(G * a.coverage / RL)
    band = (a.band or [15])[0]
    ctx = H.Context(K=31, M=17, L=2, U=50, EXT=1, ntasks=0, keep_device=True)
    tmp = tempfile.mkdtemp()
    try:
        lens = host_reads_fasta(np, os.path.join(tmp, "reads.fa"), G, RL, n, a.error_rate, a.indel_rate, 11)
        dna = H.read_dna_buffer_device(ctx, os.path.join(tmp, "reads.fa"))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    dev = dna.count_resident_device()
    out = {"what": "tools/time_pairs.py --unitigs: hsk_overlaps_unitigs on the resident graph of hsk_overlaps_reduce (rows of hsk_pair_diags_extend_gapped, band %d), beside the reduce call and the host route "
                   "it replaces, and on a synthetic line and ring; %d repetitions after %d warm-up calls, one run on one card" % (band, a.reps, WARMUP),
           "workload": {"genome_bp": G, "read_span": RL, "reads": n, "error_rate": a.error_rate, "indel_rate": a.indel_rate, "K": 31, "M": 17, "L": 2, "U": 50, "band": band}, "reps": a.reps}
    UPH = ("ms_total", "ms_arcs", "ms_sort", "ms_rank", "ms_emit", "ms_d2h")

    def unitigs_of(g, reads):
        infos = []
        for i in range(WARMUP + a.reps):
            with g.unitigs(ctx, reads, on_device=True) as ut:
                infos.append(dict(ut.info))
        s = {k: v for k, v in infos[-1].items() if not k.startswith("ms_")}
        s.update({ph: spread([r[ph] for r in infos[WARMUP:]]) for ph in UPH})
        return s

    with dev.strands(dna) as st, dev.pair_diagonals(st, a.diag_bin, on_device=True) as pd, pd.extend_gapped(ctx, dna, band=band, on_device=True) as ov:
        infos = []
        for i in range(WARMUP + a.reps):
            with ov.reduce(ctx, dna, on_device=True) as g:
                infos.append(dict(g.info, rows=len(g)))
        red = {k: v for k, v in infos[-1].items() if not k.startswith("ms_")}
        red.update({ph: spread([r[ph] for r in infos[WARMUP:]]) for ph in ("ms_total", "ms_classify", "ms_sort", "ms_reduce", "ms_d2h")})
        with ov.reduce(ctx, dna, on_device=True) as g:
            uni = unitigs_of(g, dna)
            # the host route the call replaces: the kept rows and the bits over PCIe, then OverlapGraph.arcs -- and only then the walk
            walls, walks = [], []
            for i in range(WARMUP + a.reps):
                t0 = time.perf_counter()
                kept = ctx.d2h(g.edges.rows_dev, len(g) * 48).view(np.uint64).reshape(len(g), 6)
                contained = g.host_copy()[1]
                av, aw, al, ar = H.OverlapGraph(H.Overlaps.from_rows(kept), None, contained, {}, g.rid_base, g.nreads).arcs(lens)
                walls.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            chains, longest = host_walk(np, av, aw, 2 * g.nreads)
            out["host_route"] = {"bytes": len(g) * 48 + 4 * ((g.nreads + 31) // 32), "wall_ms_rows_bits_arcs": spread(walls[WARMUP:]), "wall_ms_walk_once": (time.perf_counter() - t0) * 1e3,
                                 "chains_of_both_orientations": chains, "longest": longest, "note": "pageable host memory; the walk is numpy and one Python step per link, timed once, not repeated"}
            with g.unitigs(ctx, dna) as ut:               # every live read once, and the walk's chains are the unitigs and their complements
                out["checks"] = {"every_live_read_once": bool(np.array_equal(np.sort(ut.rid.astype(np.int64) - g.rid_base), np.flatnonzero(~contained))),
                                 "chains_are_twice_the_unitigs": chains - int(contained.sum()) * 2 == 2 * len(ut), "longest_equal": longest == ut.info["longest"]}
    out["overlaps_reduce"], out["overlaps_unitigs"] = red, uni
    # a line and a ring of a million reads on random strands: one chain through every read, where a walk is one chase of a million steps
    N = a.synthetic_reads
    strands = np.random.default_rng(9).integers(0, 2, N)
    slens = np.full(N, 100, np.uint32)
    line = SR.layout_rows(np.arange(N) * 40, slens, strands, 41)
    back = SR.layout_rows([40, 0], [100, 100], [strands[0], strands[N - 1]], 1)[0].copy()
    back[0] = np.uint64((int(back[0]) >> 63) << 63 | (N - 1))
    for name, rows, want in (("line", line, [0, N, 40 * (N - 1) + 100, 0]), ("ring", np.concatenate([line, back[None, :]]), [0, N, 40 * N, 1])):
        with H.Overlaps.from_rows(rows).reduce(ctx, slens, fuzz=0, on_device=True) as g:
            s = unitigs_of(g, slens)
            with g.unitigs(ctx, slens) as ut:
                s["one_unitig_as_expected"] = bool(len(g) == rows.shape[0] and ut.table().tolist() == [want])
                t0 = time.perf_counter()
                kept = ctx.d2h(g.edges.rows_dev, len(g) * 48).view(np.uint64).reshape(len(g), 6)
                av, aw, al, ar = H.OverlapGraph(H.Overlaps.from_rows(kept), None, np.zeros(N, bool), {}, 0, N).arcs(slens)
                s["host_wall_ms_rows_arcs_once"] = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                s["host_walk"] = host_walk(np, av, aw, 2 * N)
                s["host_wall_ms_walk_once"] = (time.perf_counter() - t0) * 1e3
        out["synthetic_" + name] = s
    for name in ("overlaps_unitigs", "synthetic_line", "synthetic_ring"):
        s = out[name]
        print("%-40s %10.3f ms [%.3f, %.3f] (arcs %.3f, sort %.3f, rank %.3f, emit %.3f), %d rows, %d unitigs, longest %d, %d rounds" % (
            "hsk_overlaps_unitigs " + name, s["ms_total"]["median"], s["ms_total"]["min"], s["ms_total"]["max"], s["ms_arcs"]["median"], s["ms_sort"]["median"], s["ms_rank"]["median"], s["ms_emit"]["median"],
            s["input_rows"], s["unitigs"], s["longest"], s["rounds"]))
    print("%-40s %10.3f ms [%.3f, %.3f] (classify %.3f, sort %.3f, reduce %.3f), %d of %d rows kept" % (
        "hsk_overlaps_reduce", red["ms_total"]["median"], red["ms_total"]["min"], red["ms_total"]["max"], red["ms_classify"]["median"], red["ms_sort"]["median"], red["ms_reduce"]["median"], red["rows"], red["input_rows"]))
    print("%-40s %10.3f ms [%.3f, %.3f] rows, bits and arcs on the host; the walk behind it once: %.3f ms" % (
        "the host route", out["host_route"]["wall_ms_rows_bits_arcs"]["median"], out["host_route"]["wall_ms_rows_bits_arcs"]["min"], out["host_route"]["wall_ms_rows_bits_arcs"]["max"], out["host_route"]["wall_ms_walk_once"]))
    dev.close()
    dna.free()
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--unitigs", action="store_true"); ap.add_argument("--synthetic-reads", type=int, default=1000000)
    ap.add_argument("--reduce", action="store_true"); ap.add_argument("--pile", type=int, default=3000); ap.add_argument("--pile-lane-only", action="store_true")
    ap.add_argument("--gapped", action="store_true"); ap.add_argument("--band", type=int, action="append", default=[]); ap.add_argument("--indel-rate", type=float, default=0.005)
    ap.add_argument("--gapped-sample", type=int, default=2000)
    ap.add_argument("--extend", action="store_true"); ap.add_argument("--error-rate", type=float, default=0.01); ap.add_argument("--sample", type=int, default=20000)
    ap.add_argument("--long-reads", type=int, default=2000); ap.add_argument("--long-len", type=int, default=12000)
    ap.add_argument("--gbp", type=float, default=0.008); ap.add_argument("--coverage", type=float, default=20.0)
    ap.add_argument("--max-records", action="append", default=[]); ap.add_argument("--merge-only", action="store_true")
    ap.add_argument("--oriented", action="store_true"); ap.add_argument("--strands-only", action="store_true")
    ap.add_argument("--diagonals", action="store_true"); ap.add_argument("--diag-bin", type=int, default=64)
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None and a.unitigs:
        a.out = os.path.join(ROOT, "profiles", "overlaps_unitigs_8mbp.json")
    if a.out is None and a.reduce:
        a.out = os.path.join(ROOT, "profiles", "overlaps_reduce_8mbp.json")
    if a.out is None and a.gapped:
        a.out = os.path.join(ROOT, "profiles", "pairs_gapped_8mbp.json")
    if a.out is None and a.extend:
        a.out = os.path.join(ROOT, "profiles", "pairs_extend_8mbp.json")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", ("pairs_diagonals_sliced_8mbp.json" if a.max_records else "pairs_diagonals_8mbp.json") if a.diagonals else "pairs_8mbp.json")
    sys.path.insert(0, ROOT)
    import numpy as np
    import hysortk_amd as H
    if a.unitigs:
        return unitigs_run(H, a)
    if a.reduce:
        return reduce_run(H, a)
    if a.gapped:
        return gapped_run(H, a)
    RL = 150
    G = int(a.gbp * 1e9)
    n = int(G * a.coverage / RL)
    ctx = H.Context(K=31, M=17, L=2, U=50, EXT=1, ntasks=0, keep_device=True)
    peak = ctx.copy_peak(1 << 30, 3)
    dp, nb, do, dl = ctx.synth_reads(G, RL, n, 11, error_rate=a.error_rate if a.extend else 0.0)
    dna = H.DeviceDna(ctx, dp, nb, do, dl, n)
    t0 = time.perf_counter()
    dev = dna.count_resident_device()
    count_ms = (time.perf_counter() - t0) * 1e3
    out = {"what": "tools/time_pairs.py: hsk_result_pairs over all tasks of a resident EXTENSION result",
           "workload": {"genome_bp": G, "read_len": RL, "reads": n, "K": 31, "M": 17, "L": 2, "U": 50, "ntasks": dev.ntasks, "entries": dev.n, "count_call_wall_ms": count_ms},
           "copy_peak_gbs": peak}

    def finish(out):
        dev.close()
        ctx.synth_free(dp, do, dl)
        ctx.close()
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out))

    if a.extend:
        # the diagonal call (unchanged code: the yardstick) and the extension of its rows, both with rows and reads in HBM
        from tests import extend_ref as X
        W = a.diag_bin
        with dev.strands(dna) as st:
            diag = summary(timed(lambda: dev.pair_diagonals(st, W, on_device=True), reps=a.reps))
            with dev.pair_diagonals(st, W, on_device=True) as pd:
                ext = extend_summary(timed(lambda: pd.extend(ctx, dna, on_device=True), reps=a.reps), peak)
                lane = extend_summary(timed(lambda: pd.extend(ctx, dna, wave_span=0xFFFFFFFF, on_device=True), reps=a.reps), peak)
                t0 = time.perf_counter()
                hrows = ctx.d2h(pd.rows_dev, pd.n * 48).view(np.uint64).reshape(pd.n, 6)
                t1 = time.perf_counter()
                packed, off, lens = dna.packed(), ctx.d2h(do, n * 8).view(np.uint64), ctx.d2h(dl, n * 4).view(np.uint32)
                t2 = time.perf_counter()
                pick = np.sort(np.random.default_rng(1).choice(pd.n, min(a.sample, pd.n), replace=False))
                srows = hrows[pick].copy()
                ids = np.concatenate([(srows[:, 0] >> np.uint64(32)) & np.uint64(0x7FFFFFFF), srows[:, 0] & np.uint64(0xFFFFFFFF)]).astype(np.int64)
                uniq, inv = np.unique(ids, return_inverse=True)
                top = srows[:, 0] & (np.uint64(1) << np.uint64(63))
                srows[:, 0] = top | (inv[:pick.size].astype(np.uint64) << np.uint64(32)) | inv[pick.size:].astype(np.uint64)      # the sample's reads renumbered
                mat = unpack_reads(np, packed, off.astype(np.int64), lens, uniq)
                t3 = time.perf_counter()
                want, _ = X.extend_rows_bulk(srows, mat, 31)
                t4 = time.perf_counter()
                got = pd.extend(ctx, dna).rows()[pick]
                ext["host_route_sample"] = {"note": "a sample: the rows and the packed reads copied to the host (all of them), then the numpy reference on `rows` rows only",
                                            "rows_d2h_bytes": pd.n * 48, "rows_d2h_wall_ms": (t1 - t0) * 1e3, "reads_d2h_bytes": int(packed.size) + n * 12, "reads_d2h_wall_ms": (t2 - t1) * 1e3,
                                            "rows": int(pick.size), "unpack_wall_ms": (t3 - t2) * 1e3, "reference_wall_ms": (t4 - t3) * 1e3,
                                            "reference_us_per_row": (t4 - t3) * 1e6 / max(1, pick.size),
                                            "device_rows_equal_reference": bool(np.array_equal(got[:, 1:], want[:, 1:]) and np.array_equal(got[:, 0], hrows[pick, 0]))}
        out["what"] = "tools/time_pairs.py --extend: hsk_result_pair_diagonals (best bin) and hsk_pair_diags_extend of its rows, rows and reads in HBM"
        out["workload"]["error_rate"] = a.error_rate
        out["diag_bin"] = W
        out["pair_diagonals"], out["extend"], out["extend_lane_path_only"] = diag, ext, lane
        out["extend_over_pair_diagonals"] = ext["median_ms"] / diag["median_ms"] if diag["median_ms"] > 0 else None
        print("%-32s %10.3f ms, %d rows" % ("hsk_result_pair_diagonals", diag["median_ms"], diag["rows"]))
        print("%-32s %10.3f ms (kernels %.3f), %d columns, %d wave rows, %.1f GB/s of reads covered (%.3f of the copy peak), x %.3f of the diagonal call" % (
            "hsk_pair_diags_extend", ext["median_ms"], ext["median_ms_extend"], ext["columns"], ext["wave_rows"], ext["read_gbs"], ext["read_of_copy_peak"], out["extend_over_pair_diagonals"] or 0.0))
        dev.close()
        ctx.synth_free(dp, do, dl)
        ctx.close()
        work, sweep, same = extend_sweep(H, a, peak)
        out["wave_span_sweep"] = {"workload": work, "default_wave_span": 512, "by_wave_span": sweep, "rows_equal_over_the_sweep": same}
        for span, s in sweep.items():
            print("long reads, wave_span %-10s %10.3f ms (kernels %.3f), %d wave rows of %d, %d columns" % (span, s["median_ms"], s["median_ms_extend"], s["wave_rows"], s["input_rows"], s["columns"]))
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out))
        return
    if a.diagonals:
        # the oriented single pass and the diagonal call on the same resident result and strands: what the second key word and the second reducer cost
        W = a.diag_bin
        st = dev.strands(dna)
        try:
            ori = summary(timed(lambda: dev.pairs(on_device=True, strands=st), reps=a.reps))
            best = summary(timed(lambda: dev.pair_diagonals(st, W, on_device=True), reps=a.reps))
            allb = summary(timed(lambda: dev.pair_diagonals(st, W, all_bins=True, on_device=True), reps=a.reps))
        except H.HskError as e:                          # the single pass does not fit the device: the sliced runs stand alone
            if not a.max_records:
                raise
            out["what"] = "tools/time_pairs.py --diagonals --max-records: hsk_result_pair_diagonals_sliced where the single pass is refused"
            out["diag_bin"] = W
            out["single_pass"] = {"status": e.status, "error": str(e)}
            out["sliced"] = sliced_alone(H, ctx, dev, st, W, a)
            st.close()
            finish(out)
            return
        with st:
            hb, ha, ho = dev.pair_diagonals(st, W), dev.pair_diagonals(st, W, all_bins=True), dev.pairs(strands=st)
            best["equals_selection_of_all_bins"] = bool(np.array_equal(ha.select().rows(), hb.rows()))
            k = ha.rows()
            start = np.flatnonzero(np.concatenate([[True], k[1:, 0] != k[:-1, 0]])) if k.shape[0] else np.zeros(0, np.int64)
            folded = np.stack([k[start, 0], np.add.reduceat(k[:, 3], start), np.minimum.reduceat(k[:, 4], start), np.maximum.reduceat(k[:, 5], start)], axis=1) if k.shape[0] else np.zeros((0, 4), np.uint64)
            allb["folded_by_key_equals_oriented"] = bool(np.array_equal(folded, ho.rows()))
            best["rows_to_host"] = {"ms_d2h": hb.info["ms_d2h"], "ms_total": hb.info["ms_total"], "bytes": len(hb) * 48}
            sliced = []
            for text in a.max_records:
                m = budget(text, best["records"])
                s = {"max_records": m, "asked": text}
                for name, all_bins, base, rows in (("best_bin", False, best, hb.rows()), ("all_bins", True, allb, ha.rows())):
                    runs = timed(lambda: dev.pair_diagonals(st, W, all_bins=all_bins, on_device=True, max_records=m), reps=a.reps)
                    last = runs[-1]
                    tot, mrg = median([r["ms_total"] for r in runs]), median([r["ms_merge"] for r in runs])
                    got = dev.pair_diagonals(st, W, all_bins=all_bins, max_records=m)
                    s[name] = {"records": last["records"], "rows": last["rows"], "keys": last["keys"], "bins": last["bins"], "slices": last["slices"], "peak_records": last["peak_records"],
                               "merges": last["merges"], "merged_rows": last["merged_rows"], "sort_passes": last["sort_passes"],
                               "ms_total": [r["ms_total"] for r in runs], "median_ms": tot, "ms_merge": [r["ms_merge"] for r in runs], "median_ms_merge": mrg,
                               "median_ms_expand": median([r["ms_expand"] for r in runs]), "median_ms_sort": median([r["ms_sort"] for r in runs]),
                               "median_ms_reduce": median([r["ms_reduce"] for r in runs]),
                               "merge_read_gbs": 48 * last["merged_rows"] / (mrg * 1e-3) / 1e9 if mrg > 0 else 0.0,
                               "merge_read_of_copy_peak": 48 * last["merged_rows"] / (mrg * 1e-3) / 1e9 / peak if mrg > 0 and peak > 0 else 0.0,
                               "ratio_to_single_pass": tot / base["median_ms"] if base["median_ms"] > 0 else None,
                               "rows_equal_single_pass": bool(np.array_equal(got.rows(), rows)),
                               "counts_equal_single_pass": all(got.info[k] == base[k] for k in ("records", "self_records", "keys", "bins"))}
                    del got
                sliced.append(s)
            if sliced:
                out["sliced"] = sliced
                # the device join of two task-range lists against the host join and the copies it replaces
                half = dev.ntasks // 2
                join = {}
                with dev.pair_diagonals(st, W, 0, half, all_bins=True, on_device=True) as pa, dev.pair_diagonals(st, W, half, dev.ntasks, all_bins=True, on_device=True) as pb:
                    for name, all_bins in (("all_bins", True), ("best_bin", False)):
                        runs = timed(lambda: H.PairDiagonals.combine([pa, pb], ctx=ctx, all_bins=all_bins, on_device=True), reps=a.reps)
                        no = runs[-1]["rows"]
                        nbytes = 48 * (pa.n + pb.n) + (48 * no if all_bins else 0)
                        mm = median([r["ms_reduce"] for r in runs])
                        join[name] = {"rows_a": pa.n, "rows_b": pb.n, "rows_out": no, "keys": runs[-1]["keys"], "bins": runs[-1]["bins"], "merge_bytes": nbytes,
                                      "ms_reduce": [r["ms_reduce"] for r in runs], "median_ms_reduce": mm, "ms_total": [r["ms_total"] for r in runs],
                                      "median_ms": median([r["ms_total"] for r in runs]), "wall_ms": [r["wall_ms"] for r in runs]}
                        if all_bins:                     # (with the selection ms_reduce holds more than the merge: no GB/s for it)
                            join[name]["gbs"] = nbytes / (mm * 1e-3) / 1e9 if mm > 0 else 0.0
                            join[name]["of_copy_peak"] = nbytes / (mm * 1e-3) / 1e9 / peak if mm > 0 and peak > 0 else 0.0
                    host_runs = []
                    for i in range(WARMUP + a.reps):
                        t0 = time.perf_counter()
                        parts = [H.PairDiagonals.from_rows(ctx.d2h(p.rows_dev, p.n * 48).view(np.uint64).reshape(p.n, 6) if p.n else np.zeros((0, 6), np.uint64), diag_bin=W, all_bins=True, info=p.info) for p in (pa, pb)]
                        t1 = time.perf_counter()
                        comb = H.PairDiagonals.combine(parts)
                        t2 = time.perf_counter()
                        sel = comb.select()
                        t3 = time.perf_counter()
                        if i >= WARMUP:
                            host_runs.append({"d2h_wall_ms": (t1 - t0) * 1e3, "combine_wall_ms": (t2 - t1) * 1e3, "select_wall_ms": (t3 - t2) * 1e3})
                    join["host"] = {"d2h_bytes": 48 * (pa.n + pb.n), "runs": host_runs,
                                    "median_wall_ms_all_bins": median([r["d2h_wall_ms"] + r["combine_wall_ms"] for r in host_runs]),
                                    "median_wall_ms_best_bin": median([r["d2h_wall_ms"] + r["combine_wall_ms"] + r["select_wall_ms"] for r in host_runs])}
                    dj, dsel = H.PairDiagonals.combine([pa, pb], ctx=ctx), H.PairDiagonals.combine([pa, pb], ctx=ctx, all_bins=False)
                    join["device_rows_equal_host_join"] = bool(np.array_equal(dj.rows(), comb.rows()) and np.array_equal(dsel.rows(), sel.rows()))
                    join["device_rows_equal_whole_range"] = bool(np.array_equal(dj.rows(), ha.rows()) and np.array_equal(dsel.rows(), hb.rows()))
                    del dj, dsel, comb, sel, parts
                out["join_two_task_ranges"] = join
            del hb, ha, ho
        out["what"] = "tools/time_pairs.py --diagonals: hsk_result_pairs_oriented (single pass) and hsk_result_pair_diagonals on the same resident EXTENSION result and strands"
        out["diag_bin"] = W
        out["pairs_oriented"], out["pair_diagonals"], out["pair_diagonals_all_bins"] = ori, best, allb
        for name, s in (("pair_diagonals", best), ("pair_diagonals_all_bins", allb)):
            s["over_oriented"] = s["median_ms"] / ori["median_ms"] if ori["median_ms"] > 0 else None
            # sort traffic per record and scatter pass: 32 bytes (key + value, read and written) for the oriented call, 48 for the two-word key
            s["sort_bytes_over_oriented"] = (48.0 * s["sort_passes"]) / (32.0 * ori["sort_passes"]) if ori["sort_passes"] > 0 and s["sort_passes"] > 0 else None
        print("%-28s %10s %10s %10s %10s %6s %10s" % ("call (median ms)", "total", "expand", "sort", "reduce", "passes", "rows"))
        for name, s in (("hsk_result_pairs_oriented", ori), ("hsk_result_pair_diagonals", best), ("  ... all_bins", allb)):
            print("%-28s %10.3f %10.3f %10.3f %10.3f %6d %10d" % (name, s["median_ms"], s["median_ms_expand"], s["median_ms_sort"], s["median_ms_reduce"], s["sort_passes"], s["rows"]))
        for s in out.get("sliced", []):
            for name in ("best_bin", "all_bins"):
                print("max_records %-12d %-8s %10.3f ms, %d slices, %d merges in %.3f ms (%.1f GB/s read), x %.2f of the single pass" % (
                    s["max_records"], name, s[name]["median_ms"], s[name]["slices"], s[name]["merges"], s[name]["median_ms_merge"], s[name]["merge_read_gbs"], s[name]["ratio_to_single_pass"] or 0.0))
    elif a.oriented:
        # the strand pass, then both pair calls on the same resident result: what the strand bit costs the sort (its top digit is no longer trivial)
        sruns = []
        for i in range(WARMUP + a.reps):
            t0 = time.perf_counter()
            with dev.strands(dna) as st:
                info = dict(st.info, wall_ms=(time.perf_counter() - t0) * 1e3)
            if i >= WARMUP:
                sruns.append(info)
        sms = median([r["ms_total"] for r in sruns])
        npay = sum(dev.task(t)["npay"] for t in range(dev.ntasks))
        out["what"] = "tools/time_pairs.py --oriented: hsk_result_strands, hsk_result_pairs and hsk_result_pairs_oriented on the same resident EXTENSION result"
        out["strands"] = {"payloads": sruns[-1]["payloads"], "reverse": sruns[-1]["reverse"], "palindromes": sruns[-1]["palindromes"], "payload_slots": npay,
                          "packed_read_bytes": nb, "ms_total": [r["ms_total"] for r in sruns], "median_ms": sms, "wall_ms": [r["wall_ms"] for r in sruns],
                          "payloads_per_us": sruns[-1]["payloads"] / (sms * 1e3) if sms > 0 else 0.0}
        if not a.strands_only:
            with dev.strands(dna) as st:
                plain = summary(timed(lambda: dev.pairs(on_device=True), reps=a.reps))
                ori = summary(timed(lambda: dev.pairs(on_device=True, strands=st), reps=a.reps))
                folded = dev.pairs(strands=st).fold()
                ori["folded_rows_equal_plain"] = bool(np.array_equal(folded.rows(), dev.pairs().rows()))
                del folded
            out["pairs"] = plain
            out["pairs_oriented"] = ori
            out["oriented_over_plain"] = ori["median_ms"] / plain["median_ms"] if plain["median_ms"] > 0 else None
            out["strands_plus_oriented_over_plain"] = (sms + ori["median_ms"]) / plain["median_ms"] if plain["median_ms"] > 0 else None
    elif a.merge_only:
        half = dev.ntasks // 2
        with dev.pairs(0, half, on_device=True) as pa, dev.pairs(half, dev.ntasks, on_device=True) as pb:
            runs = timed(lambda: H.ReadPairs.combine([pa, pb], ctx=ctx, on_device=True), reps=a.reps)
            na, nbr, no = pa.n, pb.n, runs[-1]["rows"]
        nbytes = 32 * (na + nbr) + 32 * no
        m = median([r["ms_reduce"] for r in runs])
        out["what"] = "tools/time_pairs.py --merge-only: hsk_pairs_merge of the row lists of the two halves of the task range, all three lists in HBM"
        out["merge"] = {"rows_a": na, "rows_b": nbr, "rows_out": no, "keys": runs[-1]["keys"], "bytes": nbytes,
                        "ms_merge": [r["ms_reduce"] for r in runs], "median_ms": m, "gbs": nbytes / (m * 1e-3) / 1e9 if m > 0 else 0.0,
                        "of_copy_peak": nbytes / (m * 1e-3) / 1e9 / peak if m > 0 and peak > 0 else 0.0,
                        "ms_total": [r["ms_total"] for r in runs], "wall_ms": [r["wall_ms"] for r in runs]}
    else:
        base_rows, base_ms, records = None, None, None
        try:
            runs = timed(lambda: dev.pairs(on_device=True), reps=a.reps)
            host = dev.pairs()
            base_rows = host.rows() if a.max_records else None
            last = runs[-1]
            records = rec = last["records"]; passes = last["sort_passes"]
            nbytes = {"expand": 16 * rec, "sort": 32 * rec * passes + 8 * rec, "reduce": 16 * rec}
            phases = {}
            for ph in ("expand", "sort", "reduce"):
                ms = [r["ms_" + ph] for r in runs]
                m = median(ms)
                phases[ph] = {"ms": ms, "median_ms": m, "bytes": nbytes[ph], "gbs": nbytes[ph] / (m * 1e-3) / 1e9 if m > 0 else 0.0,
                              "of_copy_peak": nbytes[ph] / (m * 1e-3) / 1e9 / peak if m > 0 and peak > 0 else 0.0}
            base_ms = median([r["ms_total"] for r in runs])
            out.update({"records": rec, "self_records": last["self_records"], "keys": last["keys"], "rows": last["rows"], "sort_passes": passes, "phases": phases,
                        "ms_total": {"ms": [r["ms_total"] for r in runs], "median_ms": base_ms},
                        "wall_ms": {"ms": [r["wall_ms"] for r in runs], "median_ms": median([r["wall_ms"] for r in runs])},
                        "rows_to_host": {"ms_d2h": host.info["ms_d2h"], "ms_total": host.info["ms_total"], "bytes": len(host) * 32}})
            del host
        except H.HskError as e:
            out["unsliced"] = {"status": e.status, "error": str(e)}
        if not a.max_records:
            # the parent commit's way to the payload: every task's CSR across PCIe
            t0 = time.perf_counter()
            fetched = 0
            for t in range(dev.ntasks):
                d = dev.fetch(t)
                fetched += d["n"] * (dev.nw + 1) * 8 + d["n"] * 8 + d["npay"] * 8
            out["fetch_every_task"] = {"wall_ms": (time.perf_counter() - t0) * 1e3, "bytes": fetched}
        sliced = []
        for text in a.max_records:
            if records is None:                          # the unsliced call did not fit: the record count comes from a sliced call of 2^29 records at a time
                with dev.pairs(on_device=True, max_records=1 << 29) as rp:
                    records = rp.info["records"]
            m = budget(text, records)
            runs = timed(lambda: dev.pairs(on_device=True, max_records=m), reps=a.reps)
            last = runs[-1]
            tot, mrg = median([r["ms_total"] for r in runs]), median([r["ms_merge"] for r in runs])
            s = {"max_records": m, "asked": text, "records": last["records"], "rows": last["rows"], "keys": last["keys"], "slices": last["slices"],
                 "peak_records": last["peak_records"], "merges": last["merges"], "merged_rows": last["merged_rows"], "sort_passes": last["sort_passes"],
                 "ms_total": [r["ms_total"] for r in runs], "median_ms": tot, "ms_merge": [r["ms_merge"] for r in runs], "median_ms_merge": mrg,
                 "median_ms_expand": median([r["ms_expand"] for r in runs]), "median_ms_sort": median([r["ms_sort"] for r in runs]),
                 "median_ms_reduce": median([r["ms_reduce"] for r in runs]),
                 # the merges read 32 B per input row; their output rows (at most as many) are not counted here: a lower bound of the kernels' GB/s
                 "merge_read_gbs": 32 * last["merged_rows"] / (mrg * 1e-3) / 1e9 if mrg > 0 else 0.0,
                 "ratio_to_unsliced": tot / base_ms if base_ms else None}
            if base_rows is not None:
                got = dev.pairs(max_records=m)
                s["rows_equal_unsliced"] = bool(np.array_equal(got.rows(), base_rows))
                del got
            sliced.append(s)
        if sliced:
            out["sliced"] = sliced
    finish(out)


if __name__ == "__main__":
    main()
