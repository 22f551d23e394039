#!/usr/bin/env python
"""Time and peak device memory of the sliding-window scan's two routes at the engine level, on the seeded genomes and rows of
tools/sparse_tiles_bench.py:
  dense   engine.base_tile_probs + engine.tile_mut_counts + engine.tile_window_test (the base planes and the window planes, 56 bytes
          per (tile, cohort)) + engine.tile_select at pval_max -- nb_model_window_hits' engine steps at one width
  sparse  engine.tile_census + engine.tile_window_census + the zero-window floor (nb_model.zero_tile_floor at binsize * width) +
          engine.sparse_window_test (join, keys, sort; count + scan; the test in chunks) + the cut on the mutated windows
Shape `both` (2 000 regions of 10 kb, 37 cohorts, binsize 1, 500 000 rows) at the widths 10 and 100: the outputs are compared first (the
dense hits with OBS >= 1 are the sparse hits: cohort, region, window, OBS equal, PVAL to 1e-6), then 3 untimed calls and the median of
20 timed ones with min and max, each ended by a device synchronise.  Shape `sparse-only` (200 000 regions of 2 kb, 5 000 000 rows) at
width 10: the sparse route alone.  torch.cuda.max_memory_allocated is taken per route, with the genome resident (`resident_bytes`).
The sparse route's steps are also timed one at a time.  One JSON line per shape and width.

    python tools/sparse_windows_bench.py [--shape both|sparse-only|all] [--widths 10 100]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))
from sparse_tiles_bench import make_genome  # noqa: E402
from tile_samples_bench import card  # noqa: E402


def run_shape(name, R, length, widths, C, binsize, M, n_chrom, pval_max, with_dense, launches, warmups, seed, chunk_windows):
    import torch
    from digdriver_amd import engine
    from digdriver_amd.sequence_model import nb_model
    dev = torch.device("cuda:0")
    per = R // n_chrom
    assert per * n_chrom == R
    g = make_genome(n_chrom, per * length, seed)
    rng = np.random.default_rng(seed + 1)
    chroms = [str(i + 1) for i in np.repeat(np.arange(n_chrom), per)]
    starts = np.tile(np.arange(per, dtype=np.int64) * length, n_chrom)
    ends = starts + length
    s_prob = rng.uniform(0.5, 1.5, (C, 64)) * 1e-3
    mu = rng.uniform(0.7, 1.3, (C, R)) * max(M / R / C, 0.05)
    sigma = 0.25 * mu
    m_chrom = torch.as_tensor(rng.integers(0, n_chrom, M), device=dev)
    m_start = torch.as_tensor(rng.integers(0, per * length, M), device=dev)
    m_cohort = torch.as_tensor(rng.integers(0, C, M).astype(np.int32), device=dev)
    rows = (m_chrom, m_start, m_start + 1, m_cohort)
    a = (g, chroms, starts, ends, s_prob)
    T = -(-length // binsize)
    g.on_device(dev)
    torch.cuda.synchronize()
    resident = torch.cuda.memory_allocated()
    smax, smin = s_prob.max(axis=1), s_prob.min(axis=1)

    def dense(m):
        pt, first, nval = engine.base_tile_probs(*a, binsize)
        k = engine.tile_mut_counts(g, chroms, starts, ends, first, nval, *rows, C, binsize, T)
        win = engine.tile_window_test(pt, k, mu, sigma, nval, m)
        return engine.tile_select(win["pval"], win["n_windows"], pval_max, k=win["k"])

    def cut(scan, m):
        kept = []
        for ch in scan.chunks(m, chunk_windows):
            hit = ch["pval"] <= pval_max
            kept.append({k: v[hit] for k, v in ch.items()})
        return {k: torch.cat([c[k] for c in kept]) for k in engine.SparseWindows.NAMES} if kept else None

    def sparse(m):
        first, nval, denom, npos = engine.tile_census(*a, binsize)
        nwin, npw = engine.tile_window_census(*a, binsize, m, n_tiles=T, n_positive=npos)
        floor, _ = nb_model.zero_tile_floor(denom, smax, smin, mu, sigma, binsize * m, npos)
        scan = engine.sparse_window_test(*a, binsize, T, first, nval, denom, mu, sigma, *rows)
        return cut(scan, m), floor

    def timed(fn):
        for _ in range(warmups):
            fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ts = []
        for _ in range(launches):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3),
                "max_memory_allocated": int(torch.cuda.max_memory_allocated())}

    def step(fn):
        """One step alone, ended by a synchronise: the median of 5 after one untimed call."""
        ts = []
        for _ in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return res, round(float(np.median(ts[1:])), 3)

    for m in widths:
        out = {"shape": dict(name=name, R=R, length=length, C=C, binsize=binsize, rows=M, width=m, tiles=R * T * C,
                             dense_plane_bytes=R * T * C * 56, pval_max=pval_max, chunk_windows=chunk_windows),
               "card": card(), "launches": launches, "warmups": warmups, "resident_bytes": int(resident)}
        got, floor = sparse(m)
        out["sparse_hits"] = int(got["k"].shape[0]) if got else 0
        out["zero_floor_min"], out["certified"] = float(floor.min()), bool((floor * (1 - nb_model.ZERO_FLOOR_MARGIN) > pval_max).all())
        if with_dense:
            want = dense(m)
            mutated = want["k"] >= 1
            cohort = torch.as_tensor(np.repeat(np.arange(C), np.diff(want["cohort_ptr"])), device=dev)[mutated]
            same = got is not None and (torch.equal(cohort, got["cohort"].long()) and torch.equal(want["region"][mutated], got["region"]) and
                                        torch.equal(want["tile"][mutated], got["window"]) and torch.equal(want["k"][mutated], got["k"]))
            rel = ((want["score"][mutated] - got["pval"]).abs() / want["score"][mutated].clamp_min(1e-300)).max().item() if same and len(cohort) else 0.0
            out["dense_hits"], out["dense_hits_without_a_row"] = int(want["k"].shape[0]), int((~mutated).sum())
            out["outputs_equal"], out["pval_max_rel_diff"] = bool(same and rel <= 1e-6), rel
            del want
            torch.cuda.empty_cache()
            out["dense"] = timed(lambda: dense(m))
            torch.cuda.empty_cache()
        del got
        out["sparse"] = timed(lambda: sparse(m))
        (first, nval, denom, npos), t_census = step(lambda: engine.tile_census(*a, binsize))
        _, t_wcensus = step(lambda: engine.tile_window_census(*a, binsize, m, n_tiles=T, n_positive=npos))
        _, t_walk = step(lambda: engine.tile_window_census(*a, binsize, m, n_tiles=T))
        scan, t_keys = step(lambda: engine.sparse_window_test(*a, binsize, T, first, nval, denom, mu, sigma, *rows))
        (_, total), t_count = step(lambda: scan.offsets(m))
        _, t_test = step(lambda: cut(scan, m))
        out["candidate_windows"] = int(total)
        out["sparse_steps_ms"] = {"census": t_census, "window_census": t_wcensus, "window_census_walking": t_walk, "join_keys_sort": t_keys,
                                  "count_scan": t_count, "test_and_cut": round(t_test - t_count, 3)}
        if with_dense:
            out["dense_over_sparse_time"] = round(out["dense"]["median_ms"] / out["sparse"]["median_ms"], 2)
            out["dense_over_sparse_memory"] = round((out["dense"]["max_memory_allocated"] - resident) /
                                                    max(out["sparse"]["max_memory_allocated"] - resident, 1), 1)
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", choices=["both", "sparse-only", "all"], default="all")
    ap.add_argument("--widths", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--cohorts", type=int, default=37)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--chunk-windows", type=int, default=1 << 24)
    args = ap.parse_args()
    from digdriver_amd import _lib
    _lib.require_device()
    common = dict(C=args.cohorts, binsize=1, pval_max=1e-4, launches=args.launches, warmups=args.warmups, seed=args.seed,
                  chunk_windows=args.chunk_windows)
    if args.shape in ("both", "all"):
        run_shape("both", R=2000, length=10000, widths=args.widths, M=500_000, n_chrom=4, with_dense=True, **common)
    if args.shape in ("sparse-only", "all"):
        run_shape("sparse-only", R=200_000, length=2000, widths=args.widths[:1], M=5_000_000, n_chrom=8, with_dense=False, **common)


if __name__ == "__main__":
    main()
