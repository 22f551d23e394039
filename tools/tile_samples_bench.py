#!/usr/bin/env python
"""Device time of the per-base route's counts by sample -- dig_tile_sample_keys, the key sort, dig_tile_sample_counts -- beside the
row count it stands in for, dig_tile_mut_counts, on the same (mutation, region) pairs, at the per-base shape of bench.py's
aux_rooflines (read from bench.py's source: regions, cohorts, bin width, tile width, chromosomes, mutation rows), with seeded rows.
Two inputs: `uniform` (rows, cohorts and samples drawn uniformly) and `adversarial` (half of the rows moved into ONE (tile, sample):
one run of M / 2 equal keys).  The interval join is made once per input and is not timed (both paths share it).  Per input: the
outputs are compared first (without a cap the capped plane is the row count), then 3 untimed launches and the median of 20 timed by
device events, for the row count, the chain, and the chain's three steps.  One JSON line.

    python tools/tile_samples_bench.py
"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bench_shape():
    """The per-base shape of bench.py's aux_rooflines, from its source."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    m = re.search(r"^\s*Rr, Cr, Wr, Br = ([\d_]+), ([\d_]+), ([\d_]+), ([\d_]+)\s*$", src, flags=re.M)
    n_chrom = re.search(r"^\s*n_chrom = (\d+)\s*$", src[m.end():], flags=re.M)
    rows = re.search(r"^\s*M = ([\d_]+)\b", src[m.end():], flags=re.M)
    R, C, W, B = (int(g.replace("_", "")) for g in m.groups())
    return dict(R=R, C=C, W=W, B=B, n_chrom=int(n_chrom.group(1)), M=int(rows.group(1).replace("_", "")))


def card():
    import torch
    name = torch.cuda.get_device_name(0)
    try:
        said = subprocess.run(["rocm-smi", "--showserial", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        serial = re.search(r"Serial Number:\s*(\S+)", said)
        return {"name": name, "serial": serial.group(1) if serial else None}
    except (OSError, subprocess.SubprocessError):
        return {"name": name, "serial": None}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples-per-cohort", type=int, default=100)
    ap.add_argument("--cap", type=int, default=2)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--rows", type=int, default=None, help="mutation rows (default: bench.py's)")
    args = ap.parse_args()
    import torch
    from digdriver_amd import _lib, engine
    from digdriver_amd._marshal import device_backend
    _lib.require_device()
    dev = torch.device("cuda:0")
    be = device_backend(dev)
    sh = bench_shape()
    R, C, W, B, n_chrom = sh["R"], sh["C"], sh["W"], sh["B"], sh["n_chrom"]
    M = args.rows or sh["M"]
    T, per, spc = W // B, R // n_chrom, args.samples_per_cohort
    S = C * spc
    reg_chrom, reg_start = np.repeat(np.arange(n_chrom), per), np.tile(np.arange(per, dtype=np.int64) * W, n_chrom)
    order, start_key, runmax_key, blk_end = engine.join_blocks(reg_chrom, reg_start, reg_start + W)
    first_pos, n_valid = be.arr(reg_start, "i64"), be.arr(np.full(R, T), "i32")
    p, s = _lib.dev_ptr, _lib.stream_ptr

    def inputs(adversarial):
        rng = np.random.default_rng(args.seed)
        chrom, start = rng.integers(0, n_chrom, M), rng.integers(0, per * W, M).astype(np.int64)
        cohort = rng.integers(0, C, M).astype(np.int32)
        sample = (cohort * spc + rng.integers(0, spc, M)).astype(np.int32)
        if adversarial:
            half = rng.permutation(M)[:M // 2]
            chrom[half], start[half], cohort[half], sample[half] = chrom[0], start[0], cohort[0], sample[0]
        mc, ms = be.arr(chrom, "i64"), be.arr(start, "i64")
        pm, pb = engine.overlap_join(be, start_key, runmax_key, blk_end, mc, ms, ms + 1)
        pr = be.arr(order, "i32")[pb.long()]
        return dict(pm=pm, pr=pr, ms=ms, co=be.arr(cohort, "i32"), sa=be.arr(sample, "i32"), n=int(pm.shape[0]))

    def timed(fn):
        for _ in range(args.warmups):
            fn()
        ts = []
        for _ in range(args.launches):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}

    out = {"shape": dict(sh, M=M, T=T, samples=S, cap=args.cap), "card": card(), "launches": args.launches, "warmups": args.warmups}
    for name in ("uniform", "adversarial"):
        d = inputs(name == "adversarial")
        n = d["n"]
        k, k_cap, k_samples = (be.empty((C, R, T), "i32") for _ in range(3))
        keys = be.empty(n, "i64")
        state = {"sorted": keys}

        def row_count():
            _lib.call("dig_tile_mut_counts", p(d["pm"]), p(d["pr"]), n, p(d["ms"]), p(d["co"]), p(first_pos), p(n_valid), B, T, R, C, p(k), s())

        def make_keys():
            _lib.call("dig_tile_sample_keys", p(d["pm"]), p(d["pr"]), n, p(d["ms"]), M, p(d["co"]), p(d["sa"]), None, p(first_pos), p(n_valid),
                      B, T, R, C, S, p(keys), s())

        def sort_keys():
            state["sorted"] = keys.sort()[0]

        def count_keys(cap=args.cap):
            _lib.call("dig_tile_sample_counts", p(state["sorted"]), n, C, R, T, S, cap, p(k_cap), p(k_samples), s())

        def chain():
            make_keys(), sort_keys(), count_keys()

        row_count(), make_keys(), sort_keys(), count_keys(0)
        same = bool(torch.equal(k, k_cap))                          # without a cap the capped plane is the row count
        count_keys()
        res = {"pairs": n, "uncapped_equals_row_count": same, "largest_run": int(k.max()), "k_cap_sum": int(k_cap.sum()),
               "k_samples_sum": int(k_samples.sum())}
        for what, fn in (("tile_mut_counts", row_count), ("keys_sort_counts", chain), ("keys", make_keys), ("sort", sort_keys),
                         ("counts", count_keys)):
            res[what + "_ms"] = timed(fn)
        out[name] = res
        del d, k, k_cap, k_samples, keys, state
        torch.cuda.empty_cache()
    for what in ("tile_mut_counts", "keys_sort_counts"):
        out["adversarial_over_uniform_" + what] = round(out["adversarial"][what + "_ms"]["median"] / out["uniform"][what + "_ms"]["median"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
