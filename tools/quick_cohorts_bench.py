#!/usr/bin/env python
"""Time of quickDriver for many cohorts on one MI355X: the element context kernel alone, and the route files -> frames for C = 37,
each beside the parent's path, on synthetic inputs -- a genome of 22 chromosomes (6 Mb each by default) with a few runs of N, a
10-kb grid of C maps, and two element shapes:

    short   10^5 elements of 1 to 3 blocks of 200 to 3 000 bp on both strands (the element shape of SURVEY.md 8d cfg 1)
    long    one 5 Mb single-block element (a --region_str)
    floor   one 200-bp single-block element: what a call costs before any base is read (two memsets, two launches)

Kernel: dig_element_context_counts on device-resident tables, device events around the call, the median of --reps calls behind one
untimed call; its bytes are 2 bits per covered base + 16 B per block + 13 B and a 256 B row per element, given as a fraction of the
8 TB/s HBM peak.  The parent's path for the same L: ONE engine.count_contexts launch over the blocks, then the host sum of
onthefly_tools._onthefly -- the block rows into a 192-column float frame keyed by 'chr{}:{}-{}', rows without a repeated key,
L_contexts.loc[keys], np.add.at -- timed in two parts (the launch with its copy to the host, the host sum).
Route: cohort_batch.run_quick_cohorts over the short elements for C cohorts with given scale factors, wall clock, beside
onthefly_tools.DIG_onthefly of the first --serial-cohorts cohorts (the parent runs one process per cohort: the figure is per cohort).

The inputs are written once; every figure is taken in a FRESH process (--processes, default 5: DESIGN.md section 8.1's method) and
the medians over the processes are printed as one JSON line.

    python tools/quick_cohorts_bench.py
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOW = 10_000
HBM_PEAK = 8.0e12


def write_inputs(tmp, args):
    from digdriver_amd.io import mapfile
    rng = np.random.default_rng(args.seed)
    n_chrom, clen = 22, args.chrom_mb * 1_000_000
    with open(os.path.join(tmp, "genome.fa"), "wb") as f:
        for c in range(1, n_chrom + 1):
            s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, clen)]
            for a in rng.integers(0, clen - 5000, 6):                    # a few runs of N, one of them long
                s[a:a + int(rng.integers(1, 40))] = ord("N")
            s[:10_000] = ord("N")
            f.write(b">chr%d\n" % c)
            for i in range(0, clen, 10_000):
                f.write(s[i:i + 10_000].tobytes() + b"\n")
    # short elements: bed12, 1 to 3 blocks of 200 to 3 000 bp
    E = args.elements
    chrom = rng.integers(1, n_chrom + 1, E)
    start = rng.integers(10_000, clen - 20_000, E)
    nb = rng.integers(1, 4, E)
    with open(os.path.join(tmp, "short.bed"), "w") as f:
        for e in range(E):
            sizes = rng.integers(200, 3001, nb[e])
            gaps = rng.integers(10, 2000, nb[e])
            offs = np.concatenate([[0], np.cumsum(sizes[:-1] + gaps[:-1])])
            end = start[e] + offs[-1] + sizes[-1]
            f.write("%d\t%d\t%d\tE%06d\t0\t%s\t%d\t%d\t.\t%d\t%s,\t%s,\n" % (chrom[e], start[e], end, e, "+-"[e & 1], start[e], start[e], nb[e],
                                                                        ",".join(map(str, sizes)), ",".join(map(str, offs))))
    with open(os.path.join(tmp, "long.bed"), "w") as f:
        f.write("3\t500000\t5500000\tUserELT\t0\t+\t0\t0\t.\t1\t5000000,\t0,\n")
    with open(os.path.join(tmp, "floor.bed"), "w") as f:
        f.write("3\t500000\t500200\tUserELT\t0\t+\t0\t0\t.\t1\t200,\t0,\n")
    # C maps on one 10-kb grid, one mutation file each
    bins = [(c, s, s + WINDOW) for c in range(1, n_chrom + 1) for s in range(0, clen, WINDOW)]
    grid = pd.DataFrame(bins, columns=["CHROM", "START", "END"])
    ctx = ["".join(t) for t in __import__("itertools").product("ACGT", repeat=3)]
    seq_rows = [(c[1] + ">" + a, c) for c in ctx for a in "ACGT" if a != c[1]]
    for c in range(args.cohorts):
        rp = grid.copy()
        rp["Y_PRED"] = rng.gamma(9.0, 3.0, len(rp))
        rp["STD"] = rng.gamma(4.0, 1.0, len(rp))
        rp["Y_TRUE"] = rng.poisson(rp.Y_PRED.values)
        rp["FLAG"] = rng.uniform(size=len(rp)) < 0.1
        rp.index = ["chr{}:{}-{}".format(*b) for b in bins]
        pre = os.path.join(tmp, "map%02d.map" % c)
        mapfile.write_frame(pre, "region_params", rp)
        mapfile.write_frame(pre, "sequence_model_192", pd.DataFrame({"MUT_TYPE": [m for m, _ in seq_rows], "CONTEXT": [x for _, x in seq_rows],
                                                                    "FREQ": rng.dirichlet(np.ones(192)) * 1e-3}))
        mapfile.write_array(pre, "idx", grid.values.astype(np.int32))
        n = args.mut_rows
        m_chrom, m_start = rng.integers(1, n_chrom + 1, n), rng.integers(10_000, clen - 1, n)
        indel = rng.uniform(size=n) < 0.05
        rows = pd.DataFrame({0: m_chrom, 1: m_start, 2: m_start + np.where(indel, 3, 1), 3: np.where(indel, "ACG", "A"), 4: np.where(indel, "A", "T"),
                             5: np.char.add("S", rng.integers(0, 200, n).astype(str)), 6: ".", 7: np.where(indel, "INDEL", "Noncoding")})
        rows.sort_values([0, 1], kind="stable").to_csv(os.path.join(tmp, "cohort%02d.tsv" % c), sep="\t", header=False, index=False)


def element_tables(f_bed):
    from digdriver_amd.driver_model import cohort_batch
    return cohort_batch._quick_elements(f_bed)[:6]


def kernel_times(genome, f_bed, reps):
    """ms of dig_element_context_counts (median of reps) and of the parent's path for the same L, with the bytes the kernel reads."""
    import torch
    from digdriver_amd import _lib, engine
    names, chrom, minus, ptr, start, end = element_tables(f_bed)
    E, nb = len(names), len(start)
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    ci = genome.chrom_index(["chr%d" % c for c in chrom])
    tens = [d(ci), d(minus), d(ptr), d(start), d(end)]
    out = torch.empty((E, 64), dtype=torch.int32, device="cuda")
    n_ws = int(_lib.load().dig_element_context_counts_workspace(nb))
    ws = torch.empty(n_ws, dtype=torch.uint8, device="cuda")
    head = genome.genome2_args(torch.device("cuda"))
    p = _lib.dev_ptr
    call = lambda: _lib.call("dig_element_context_counts", *head, *[p(t) for t in tens], E, nb, p(out), p(ws), n_ws, _lib.stream_ptr())
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    lens = np.minimum(end, genome.lengths[ci][np.repeat(np.arange(E), np.diff(ptr))]) - np.maximum(start, 1)
    covered = int(np.maximum(lens, 0).sum())
    nbytes = covered / 4 + 16 * nb + 13 * E + 256 * E
    k_ms = float(np.median(ms))
    # the parent's path (onthefly_tools._onthefly: precount_region_contexts_parallel + the host sum)
    from digdriver_amd.sequence_model import sequence_tools
    owner = np.repeat(np.arange(E), np.diff(ptr))
    regions = list(zip(chrom[owner].astype(str), start, end, np.where(minus[owner] != 0, "-", "+")))
    trans_idx = sequence_tools.mk_trans_idx(n_up=1, n_down=1, collapse=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    frame = sequence_tools.nonc_elt_context_count(regions, trans_idx, genome)
    frame = frame.loc[~frame.index.duplicated()]
    t1 = time.perf_counter()
    keys = ['chr{}:{}-{}'.format(c, s, e) for c, s, e in zip(chrom[owner], start, end)]
    Lb = frame.loc[keys].values
    L = np.zeros((E, 192))
    np.add.at(L, owner, Lb)
    L = np.rint(L).astype(np.int32)
    t2 = time.perf_counter()
    _, cols = sequence_tools._context_columns(trans_idx)
    same = bool(np.array_equal(out.cpu().numpy()[:, cols], L))
    return {"elements": E, "blocks": nb, "covered_bases": covered, "kernel_ms": round(k_ms, 4), "kernel_ms_min": round(min(ms), 4),
            "kernel_bytes": int(nbytes), "kernel_TBps": round(nbytes / (k_ms * 1e-3) / 1e12, 4), "kernel_hbm_fraction": round(nbytes / (k_ms * 1e-3) / HBM_PEAK, 4),
            "parent_count_frame_ms": round((t1 - t0) * 1e3, 2), "parent_host_sum_ms": round((t2 - t1) * 1e3, 2), "same_L": same}


def child(tmp, args):
    import torch
    from digdriver_amd import _lib
    from digdriver_amd.driver_model import cohort_batch, onthefly_tools
    from digdriver_amd.sequence_model import sequence_tools
    _lib.require_device()
    assert torch.cuda.is_available()
    fa = os.path.join(tmp, "genome.fa")
    t0 = time.perf_counter()
    genome = sequence_tools.load_genome(fa)
    genome.on_device2(torch.device("cuda"))
    out = {"load_genome_s": round(time.perf_counter() - t0, 3)}
    out["short"] = kernel_times(genome, os.path.join(tmp, "short.bed"), args.reps)
    out["long"] = kernel_times(genome, os.path.join(tmp, "long.bed"), args.reps)
    out["floor"] = kernel_times(genome, os.path.join(tmp, "floor.bed"), args.reps)
    C = args.cohorts
    muts = [os.path.join(tmp, "cohort%02d.tsv" % c) for c in range(C)]
    maps = [os.path.join(tmp, "map%02d.map" % c) for c in range(C)]
    cj, cji = np.full(C, 0.004), np.full(C, 0.0007)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    frames = cohort_batch.run_quick_cohorts(muts, maps, fa, f_elts_bed=os.path.join(tmp, "short.bed"), scale_factors=(cj, cji),
                                            scale_by_expectation=False)
    out["route_s"] = round(time.perf_counter() - t0, 3)
    serial = []
    for c in range(min(C, args.serial_cohorts)):
        t0 = time.perf_counter()
        want = onthefly_tools.DIG_onthefly(maps[c], muts[c], fa, f_elts_bed=os.path.join(tmp, "short.bed"), scale_factor=cj[c],
                                           scale_factor_indel=cji[c], scale_by_expectation=False)
        serial.append(time.perf_counter() - t0)
        out["frames_close"] = bool(np.array_equal(want.OBS_SNV.values, frames[c].OBS_SNV.values) and
                                   np.allclose(want.PVAL_MUT_BURDEN.values, frames[c].PVAL_MUT_BURDEN.values, rtol=1e-9, atol=0, equal_nan=True))
    out["serial_per_cohort_s"] = round(float(np.median(serial)), 3) if serial else None
    print("__RESULT__" + json.dumps(out), flush=True)


def median_of(results, path):
    vals = []
    for r in results:
        for k in path:
            r = r[k]
        vals.append(r)
    return float(np.median(vals))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cohorts", type=int, default=37)
    ap.add_argument("--elements", type=int, default=100_000)
    ap.add_argument("--mut-rows", type=int, default=100_000, help="rows of a cohort's mutation file")
    ap.add_argument("--chrom-mb", type=int, default=6, help="length of each of the 22 chromosomes in Mb (at least 6: the long element)")
    ap.add_argument("--serial-cohorts", type=int, default=1, help="DIG_onthefly calls timed per process")
    ap.add_argument("--processes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--child", type=str, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args)
    with tempfile.TemporaryDirectory() as tmp:
        write_inputs(tmp, args)
        print("inputs written", file=sys.stderr, flush=True)
        results = []
        for _ in range(args.processes):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", tmp] + [x for k in ("cohorts", "serial_cohorts", "reps")
                                                                                 for x in ("--" + k.replace("_", "-"), str(getattr(args, k)))]
            text = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
            results.append(json.loads([ln for ln in text.splitlines() if ln.startswith("__RESULT__")][-1][len("__RESULT__"):]))
            print("process %d of %d: route %.2f s" % (len(results), args.processes, results[-1]["route_s"]), file=sys.stderr, flush=True)
    out = {"cohorts": args.cohorts, "processes": len(results), "first_process": results[0]}
    for shape in ("short", "long", "floor"):
        out[shape] = {k: median_of(results, (shape, k)) for k in ("kernel_ms", "kernel_TBps", "kernel_hbm_fraction", "parent_count_frame_ms",
                                                                  "parent_host_sum_ms")}
        out[shape]["same_L"] = all(r[shape]["same_L"] for r in results)
    out["long_over_short_per_byte"] = round(out["short"]["kernel_TBps"] / out["long"]["kernel_TBps"], 3)
    out["long_minus_floor_ms"] = round(out["long"]["kernel_ms"] - out["floor"]["kernel_ms"], 4)
    out["route_s"] = median_of(results, ("route_s",))
    out["serial_per_cohort_s"] = median_of(results, ("serial_per_cohort_s",))
    out["frames_close"] = all(r.get("frames_close", True) for r in results)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
