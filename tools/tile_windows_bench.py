#!/usr/bin/env python
"""Device time of the sliding-window test of the per-base route, dig_tile_window_test, beside dig_tiled_nb_test on the same planes, at
the per-base shape of bench.py's aux_rooflines (read from bench.py's source: regions, cohorts, bin width, tile width, chromosomes,
mutation rows), with seeded rows; widths 2 and 10.  The base planes come from the route's own front half (engine.base_tile_probs,
engine.tile_mut_counts) on bench.py's synthetic genome.  Per width the outputs are checked first: pval_w and exp_w must be
dig_tiled_nb_test of the returned pt_w, k_w bit for bit, and width 1 must give dig_tiled_nb_test's planes; then 3 untimed launches
and the median and range of 20 timed by device events.  Fractions of the HBM peak by the algorithmic bytes: 40 per (tile, cohort)
for the window kernel (12 read, 28 written), 28 for dig_tiled_nb_test (12 read, 16 written).
The whole route, timed the same way (5 runs; the interval join and its host round trips included): the front half once and
the two widths, against two runs of the existing route (engine.tiled_nb_model) at the bin width and at ten times it.  One JSON line.

    python tools/tile_windows_bench.py
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

WIDTHS = (2, 10)
WINDOW_BYTES, TILED_BYTES = 40.0, 28.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--route-runs", type=int, default=5)
    ap.add_argument("--regions", type=int, default=None, help="regions (default: bench.py's)")
    ap.add_argument("--seed", type=int, default=4)
    args = ap.parse_args()
    import re
    import torch
    from tile_samples_bench import bench_shape, card
    from digdriver_amd import _lib, engine
    from digdriver_amd.data_tools.genome import PackedGenome
    _lib.require_device()
    sh = bench_shape()
    hbm_peak = float(re.search(r"^HBM_PEAK = ([\d.e]+)", open(os.path.join(ROOT, "bench.py")).read(), flags=re.M).group(1))
    R, C, W, B, n_chrom, M = args.regions or sh["R"], sh["C"], sh["W"], sh["B"], sh["n_chrom"], sh["M"]
    T, per = W // B, R // n_chrom
    rng = np.random.default_rng(args.seed)
    words = rng.integers(0, 2 ** 32, (per * W * n_chrom) // 8 + 2, dtype=np.uint64).astype(np.uint32) & np.uint32(0x33333333)
    words[0] = words[-1] = 0x44444444
    names = ["chr%d" % (i + 1) for i in range(n_chrom)]
    genome = PackedGenome(names, np.arange(n_chrom, dtype=np.int64) * per * W, np.full(n_chrom, per * W, np.int64), words)
    chroms, starts = np.repeat(names, per), np.tile(np.arange(per, dtype=np.int64) * W, n_chrom)
    mu, sigma = rng.uniform(5, 45, (C, R)), rng.uniform(1, 7, (C, R))
    mc, ms, co = np.array(names)[rng.integers(0, n_chrom, M)], rng.integers(0, per * W, M).astype(np.int64), rng.integers(0, C, M).astype(np.int32)
    s_prob = rng.uniform(0, 1e-2, (C, 64))
    up = lambda x: torch.as_tensor(x, device="cuda:0")
    mu_d, sigma_d, ms_d, co_d = up(mu), up(sigma), up(ms), up(co)

    def front(binsize):
        pt, first, nval = engine.base_tile_probs(genome, chroms, starts, starts + W, s_prob, binsize)
        k = engine.tile_mut_counts(genome, chroms, starts, starts + W, first, nval, mc, ms_d, ms_d + 1, co_d, C, binsize, pt.shape[2])
        return pt, k, nval

    def timed(fn, launches, warmups):
        for _ in range(warmups):
            fn()
        ts = []
        for _ in range(launches):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}

    pt, k, nval = front(B)
    n = float(C) * R * T
    out = {"shape": dict(sh, R=R, T=T, rows_counted=int(k.sum())), "card": card(), "launches": args.launches, "warmups": args.warmups,
           "hbm_peak_GBps": hbm_peak / 1e9}
    p, s = _lib.dev_ptr, _lib.stream_ptr
    pval, ex = torch.empty_like(pt), torch.empty_like(pt)
    planes = engine.tile_window_test(pt, k, mu_d, sigma_d, nval, 1)
    tiled = lambda a, b, o1, o2: _lib.call("dig_tiled_nb_test", p(a), 1, p(b), p(mu_d), p(sigma_d), p(o1), p(o2), C, R, T, s())
    same = lambda x, y: bool(torch.equal(x.view(torch.int64), y.view(torch.int64)))
    tiled(pt, k, pval, ex)
    out["width_1_equals_tiled_nb_test"] = same(planes["pval"], pval) and same(planes["exp"], ex) and same(planes["pt"], pt) and bool(torch.equal(planes["k"], k))
    for m in WIDTHS:
        engine.tile_window_test(pt, k, mu_d, sigma_d, nval, m, out=planes)
        tiled(planes["pt"], planes["k"], pval, ex)
        ok = same(planes["pval"], pval) and same(planes["exp"], ex)
        window = lambda: _lib.call("dig_tile_window_test", p(pt), p(k), p(mu_d), p(sigma_d), p(nval), C, R, T, m, p(planes["pt"]), p(planes["k"]),
                                   p(planes["exp"]), p(planes["pval"]), p(planes["n_windows"]), s())
        t = timed(window, args.launches, args.warmups)
        out["width_%d" % m] = {"composition_bit_equal": ok, "ms": t, "windows_with_rows": int((planes["k"] > 0).sum()),
                               "hbm_frac": round(WINDOW_BYTES * n / (t["median"] * 1e-3) / hbm_peak, 4)}
    t = timed(lambda: tiled(pt, k, pval, ex), args.launches, args.warmups)
    out["tiled_nb_test"] = {"ms": t, "hbm_frac": round(TILED_BYTES * n / (t["median"] * 1e-3) / hbm_peak, 4)}
    del pval, ex, planes, pt, k
    torch.cuda.empty_cache()

    def window_route():
        a, b, v = front(B)
        pl = None
        for m in WIDTHS:
            pl = engine.tile_window_test(a, b, mu_d, sigma_d, v, m, out=pl)

    def existing_route():
        for binsize in (B, 10 * B):
            engine.tiled_nb_model(genome, chroms, starts, starts + W, s_prob, mu_d, sigma_d, mc, ms_d, ms_d + 1, co_d, binsize=binsize)

    out["route_front_half_and_two_widths_ms"] = timed(window_route, args.route_runs, 1)
    torch.cuda.empty_cache()
    out["route_existing_at_two_bin_widths_ms"] = timed(existing_route, args.route_runs, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
