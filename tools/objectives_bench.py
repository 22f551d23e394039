#!/usr/bin/env python
"""Wall time of the training labels for many cohorts: data_tools.objectives.window_objectives on the device beside the same call
through the `_host` twins, on synthetic inputs of the training container's size -- C = 37 cohorts x 300 000 rows against 288 000
windows of 10 kb on 22 chromosomes.  The cohorts are encoded once (encode_objective_rows' arrays, made here without files: parsing
is the same host work on both routes and is reported apart, for one file); a timed pass is the interval join, the keys, the sort,
the two counting kernels and the sample thresholds.  The two routes take turns (device, host, device, ...) behind one untimed pass
of each; the median and the range of each go to one JSON line.

    python tools/objectives_bench.py --rounds 5
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_windows(n, width=10_000):
    per = -(-n // 22)
    idx = np.stack([np.repeat(np.arange(1, 23), per)[:n], (np.tile(np.arange(per), 22)[:n]) * width,
                    (np.tile(np.arange(per), 22)[:n] + 1) * width], 1)
    return idx.astype(np.int32)


def make_cohort(rng, n, idx, samples, width=10_000):
    """rows as encode_objective_rows gives them: 13 % indels of 4 bases, 2 % of the rows repeated, a hypermutated sample"""
    w = idx[rng.integers(0, len(idx), n)]
    start = w[:, 1].astype(np.int64) + rng.integers(0, width, n)
    indel = rng.uniform(size=n) < 0.13
    sample = np.minimum(rng.geometric(4.0 / samples, n) - 1, samples - 1).astype(np.int32)
    rep = rng.integers(0, n, n // 50)
    to = rng.integers(0, n, n // 50)
    start[to], indel[to], sample[to] = start[rep], indel[rep], sample[rep]
    chrom = w[:, 0].astype(np.int64)
    chrom[to] = chrom[rep]
    _, uid = np.unique(np.stack([chrom, start, indel.astype(np.int64)], 1), axis=0, return_inverse=True)
    uid = np.asarray(uid).reshape(-1)
    return dict(chrom=chrom, start=start, end=start + np.where(indel, 4, 1), sample=sample, uid=uid.astype(np.int32),
                indel=indel.astype(np.uint8), n_uid=int(uid.max()) + 1, sample_names=["S%d" % i for i in range(samples)])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cohorts", type=int, default=37)
    ap.add_argument("--mut-rows", type=int, default=300_000)
    ap.add_argument("--windows", type=int, default=288_000)
    ap.add_argument("--samples", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    args = ap.parse_args()
    from digdriver_amd.data_tools import objectives
    idx = make_windows(args.windows)
    cohorts = [make_cohort(np.random.default_rng([args.seed, c]), args.mut_rows, idx, args.samples) for c in range(args.cohorts)]
    kw = dict(max_muts_per_sample=5000, sample_filter_stdev=3.0)

    # the host work in front of both routes, for one cohort: a file written and parsed
    with tempfile.TemporaryDirectory() as tmp:
        c = cohorts[0]
        f = os.path.join(tmp, "cohort.annot.txt")
        import pandas as pd
        pd.DataFrame({0: c["chrom"], 1: c["start"], 2: c["end"], 3: np.where(c["indel"] > 0, "ACGT", "A"), 4: np.where(c["indel"] > 0, "A", "T"),
                      5: np.char.add("S", c["sample"].astype(str)), 6: ".", 7: np.where(c["indel"] > 0, "INDEL", "Noncoding")}).to_csv(
                          f, sep="\t", header=False, index=False)
        t0 = time.perf_counter()
        objectives.encode_objective_rows(f, {str(i): i for i in range(1, 23)})
        encode_s = time.perf_counter() - t0

    def device():
        import torch
        out = objectives.window_objectives(idx, cohorts, on_device=True, **kw)[1]
        torch.cuda.synchronize()
        return out

    def host():
        return objectives.window_objectives(idx, cohorts, on_device=False, **kw)[1]

    times = {"device": [], "host": []}
    a, b = device(), host()                                          # untimed: code objects, allocator
    for _ in range(args.rounds):
        for name, fn in (("device", device), ("host", host)):
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    out = {"cohorts": args.cohorts, "mut_rows": args.mut_rows, "windows": args.windows, "samples_per_cohort": args.samples,
           "labels_equal": bool(np.array_equal(a, b)), "label_sum": float(a.sum()), "encode_one_file_s": round(encode_s, 4)}
    for name, ts in times.items():
        out[name + "_s"] = {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4), "n": len(ts)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
