#!/usr/bin/env python
"""Time and peak device memory of the per-base scan's two routes at the engine level, on a seeded genome with seeded rows:
  dense   engine.tiled_nb_model (four [C, R, T] planes) + engine.tile_select at pval_max
  sparse  engine.tile_census + the zero-tile floor (nb_model.zero_tile_floor) + engine.sparse_tile_test + the cut on the mutated tiles
Shape `both` (default 2 000 regions of 10 kb, 37 cohorts, binsize 1, 500 000 rows; the dense planes take about 21 GB): the outputs are
compared first (the dense hits with OBS >= 1 are the sparse hits: region, tile, OBS equal, PVAL to 1e-6), then 3 untimed calls and the
median of 20 timed ones, each ended by a device synchronise.  Shape `sparse-only` (default 200 000 regions of 2 kb, 5 000 000 rows:
the dense planes would take about 410 GB): the sparse route alone.  torch.cuda.max_memory_allocated is taken per route, with the
genome resident (reported as `resident_bytes`).  One JSON line per shape.

    python tools/sparse_tiles_bench.py [--shape both|sparse-only|all]
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
from tile_samples_bench import card  # noqa: E402


def make_genome(n_chrom, chrom_len, seed):
    """A random ACGT genome in the packed 4-bit layout, written as words (a string of this size would take minutes to pack)."""
    from digdriver_amd.data_tools.genome import PackedGenome
    assert chrom_len % 8 == 0
    rng = np.random.default_rng(seed)
    words = rng.integers(0, 1 << 32, n_chrom * chrom_len // 8 + 2, dtype=np.uint64).astype(np.uint32) & np.uint32(0x33333333)
    words[0] = words[-1] = 0x44444444                     # the pad words: letters other than ACGT
    return PackedGenome([str(i + 1) for i in range(n_chrom)], np.arange(n_chrom, dtype=np.int64) * chrom_len,
                        np.full(n_chrom, chrom_len, np.int64), words)


def run_shape(name, R, width, C, binsize, M, n_chrom, pval_max, with_dense, launches, warmups, seed):
    import torch
    from digdriver_amd import engine
    from digdriver_amd.sequence_model import nb_model
    dev = torch.device("cuda:0")
    per = R // n_chrom
    assert per * n_chrom == R
    g = make_genome(n_chrom, per * width, seed)
    rng = np.random.default_rng(seed + 1)
    chroms = [str(i + 1) for i in np.repeat(np.arange(n_chrom), per)]
    starts = np.tile(np.arange(per, dtype=np.int64) * width, n_chrom)
    ends = starts + width
    s_prob = rng.uniform(0.5, 1.5, (C, 64)) * 1e-3
    rows_per_region = M / R
    mu = rng.uniform(0.7, 1.3, (C, R)) * max(rows_per_region / C, 0.05)
    sigma = 0.25 * mu
    m_chrom = torch.as_tensor(rng.integers(0, n_chrom, M), device=dev)
    m_start = torch.as_tensor(rng.integers(0, per * width, M), device=dev)
    m_cohort = torch.as_tensor(rng.integers(0, C, M).astype(np.int32), device=dev)
    rows = (m_chrom, m_start, m_start + 1, m_cohort)
    T = -(-width // binsize)
    g.on_device(dev)
    torch.cuda.synchronize()
    resident = torch.cuda.memory_allocated()
    smax, smin = s_prob.max(axis=1), s_prob.min(axis=1)

    def dense():
        res = engine.tiled_nb_model(g, chroms, starts, ends, s_prob, mu, sigma, *rows, binsize=binsize)
        return engine.tile_select(res["pval"], res["n_valid"], pval_max, k=res["k"])

    def sparse():
        first, nval, denom, npos = engine.tile_census(g, chroms, starts, ends, s_prob, binsize)
        floor, _ = nb_model.zero_tile_floor(denom, smax, smin, mu, sigma, binsize, npos)
        tiles = engine.sparse_tile_test(g, chroms, starts, ends, s_prob, binsize, T, first, nval, denom, mu, sigma, *rows)
        hit = tiles["pval"] <= pval_max
        return {k: v[hit] for k, v in tiles.items()}, floor, int(tiles["k"].shape[0])

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

    out = {"shape": dict(name=name, R=R, width=width, C=C, binsize=binsize, rows=M, tiles=R * T * C, dense_plane_bytes=R * T * C * 28,
                         pval_max=pval_max), "card": card(), "launches": launches, "warmups": warmups, "resident_bytes": int(resident)}
    got, floor, n_mutated = sparse()
    out["mutated_tiles"], out["sparse_hits"] = n_mutated, int(got["k"].shape[0])
    out["zero_floor_min"], out["certified"] = float(floor.min()), bool((floor * (1 - nb_model.ZERO_FLOOR_MARGIN) > pval_max).all())
    if with_dense:
        want = dense()
        mutated = want["k"] >= 1
        ptr = want["cohort_ptr"]
        cohort = torch.as_tensor(np.repeat(np.arange(C), np.diff(ptr)), device=dev)[mutated]
        same = (torch.equal(cohort, got["cohort"].long()) and torch.equal(want["region"][mutated], got["region"]) and
                torch.equal(want["tile"][mutated], got["tile"]) and torch.equal(want["k"][mutated], got["k"]))
        rel = ((want["score"][mutated] - got["pval"]).abs() / want["score"][mutated].clamp_min(1e-300)).max().item() if same and len(cohort) else 0.0
        out["dense_hits"], out["dense_hits_without_a_row"] = int(want["k"].shape[0]), int((~mutated).sum())
        out["outputs_equal"], out["pval_max_rel_diff"] = bool(same and rel <= 1e-6), rel
        del want
        torch.cuda.empty_cache()
        out["dense"] = timed(dense)
        torch.cuda.empty_cache()
    del got
    out["sparse"] = timed(sparse)

    # where the sparse route's time goes: its steps one at a time, each ended by a synchronise (median of 5 after one untimed call)
    def step(fn):
        ts = []
        for i in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return res, round(float(np.median(ts[1:])), 3)

    from digdriver_amd._marshal import device_backend
    be = device_backend(dev)
    (first, nval, denom, npos), t_census = step(lambda: engine.tile_census(g, chroms, starts, ends, s_prob, binsize))
    _, t_floor = step(lambda: nb_model.zero_tile_floor(denom, smax, smin, mu, sigma, binsize, npos))
    _, t_join = step(lambda: engine._tile_pairs(be, g, chroms, starts, ends, *rows[:3]))
    _, t_test = step(lambda: engine.sparse_tile_test(g, chroms, starts, ends, s_prob, binsize, T, first, nval, denom, mu, sigma, *rows))
    out["sparse_steps_ms"] = {"census": t_census, "floor": t_floor, "join": t_join, "keys_sort_test": round(t_test - t_join, 3)}
    if with_dense:
        out["dense_over_sparse_time"] = round(out["dense"]["median_ms"] / out["sparse"]["median_ms"], 2)
        out["dense_over_sparse_memory"] = round((out["dense"]["max_memory_allocated"] - resident) /
                                                max(out["sparse"]["max_memory_allocated"] - resident, 1), 1)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", choices=["both", "sparse-only", "all"], default="all")
    ap.add_argument("--cohorts", type=int, default=37)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--seed", type=int, default=4)
    args = ap.parse_args()
    from digdriver_amd import _lib
    _lib.require_device()
    common = dict(C=args.cohorts, binsize=1, pval_max=1e-4, launches=args.launches, warmups=args.warmups, seed=args.seed)
    if args.shape in ("both", "all"):
        run_shape("both", R=2000, width=10000, M=500_000, n_chrom=4, with_dense=True, **common)
    if args.shape in ("sparse-only", "all"):
        run_shape("sparse-only", R=200_000, width=2000, M=5_000_000, n_chrom=8, with_dense=False, **common)


if __name__ == "__main__":
    main()
