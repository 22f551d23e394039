#!/usr/bin/env python
"""Device time of the three kernels behind the calls of the element route -- dig_row_select_count, dig_row_select_fill,
dig_row_scatter -- on a seeded plane of the flagship size: rows = 4 p-value columns x 37 cohorts, n = 120 091 elements, uniform
p-values with about 1 % NaN, at cut = +inf (every number selected: the Benjamini-Hochberg pass) and at a cut that about 0.1 % of the
values pass (calls).  Beside them, on the same values viewed as [rows, 1, n], dig_tile_select_count / dig_tile_select_fill: what the
per-base route's selection would take for this plane (a wave per row in its fill).  The outputs of the two selections are compared
first.  Then, per repetition and cut, every call runs once in a fixed order between device events:

    row_count, row_fill, row_scatter, tile_count, tile_fill          x (cut = +inf, cut = --rate quantile)  x --reps

so that a kernel trace of the process (rocprofv3 --kernel-trace --stats -- python tools/row_select_bench.py) lists, per kernel name,
its dispatches in that order: the LAST 2 x reps dispatches of a kernel are the timed ones, dispatch i of them belonging to repetition
i // 2 and cut i % 2 (in front of them: the set-up's counts and the untimed pass).  One JSON line: the event times, and the bytes each call moves by its algorithm (count: the plane; fill:
the plane + 12 B per selected element; scatter: the plane read, the plane written + 8 B per selected element) over them.

    python tools/row_select_bench.py --reps 5
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12                                                      # bytes / s


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=4 * 37)
    ap.add_argument("--n", type=int, default=120_091)
    ap.add_argument("--nan", type=float, default=0.01)
    ap.add_argument("--rate", type=float, default=0.001)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    args = ap.parse_args()
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    dev = torch.device("cuda:0")
    rows, n = args.rows, args.n
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    score = torch.rand((rows, n), generator=gen, device=dev, dtype=torch.float64)
    score[torch.rand((rows, n), generator=gen, device=dev) < args.nan] = float("nan")
    p, s = _lib.dev_ptr, _lib.stream_ptr
    slots = int(_lib.load().dig_row_select_counts_size(rows, n))
    n_valid = torch.full((1,), n, dtype=torch.int32, device=dev)
    plane = 8 * rows * n

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def setup(cut_value):
        """Everything a timed call needs, formed beforehand: counts, offsets and output buffers of both selections."""
        cut = torch.full((rows,), cut_value, dtype=torch.float64, device=dev)
        counts, t_counts = torch.empty(slots, dtype=torch.int32, device=dev), torch.empty(rows, dtype=torch.int32, device=dev)
        _lib.call("dig_row_select_count", p(score), p(cut), rows, n, p(counts), s())
        _lib.call("dig_tile_select_count", p(score), p(n_valid), p(cut), rows, 1, n, p(t_counts), s())
        incl, t_incl = torch.cumsum(counts, 0, dtype=torch.int64), torch.cumsum(t_counts, 0, dtype=torch.int64)
        total = int(incl[-1])
        assert total == int(t_incl[-1])
        c = dict(cut=cut, counts=counts, t_counts=t_counts, offsets=incl - counts, t_offsets=t_incl - t_counts, total=total,
                 index=torch.empty(total, dtype=torch.int32, device=dev), hit=torch.empty(total, dtype=torch.float64, device=dev),
                 region=torch.empty(total, dtype=torch.int32, device=dev), tile=torch.empty(total, dtype=torch.int32, device=dev),
                 t_hit=torch.empty(total, dtype=torch.float64, device=dev), out=torch.empty((rows, n), dtype=torch.float64, device=dev))
        c["calls"] = {
            "row_count": lambda: _lib.call("dig_row_select_count", p(score), p(cut), rows, n, p(counts), s()),
            "row_fill": lambda: _lib.call("dig_row_select_fill", p(score), p(cut), rows, n, p(c["offsets"]), total, p(c["index"]), p(c["hit"]), s()),
            "row_scatter": lambda: _lib.call("dig_row_scatter", p(score), p(cut), rows, n, p(c["offsets"]), total, p(c["hit"]), float("nan"),
                                             p(c["out"]), s()),
            "tile_count": lambda: _lib.call("dig_tile_select_count", p(score), p(n_valid), p(cut), rows, 1, n, p(t_counts), s()),
            "tile_fill": lambda: _lib.call("dig_tile_select_fill", p(score), p(n_valid), p(cut), rows, 1, n, p(c["t_offsets"]), total, None, None,
                                           None, p(c["region"]), p(c["tile"]), p(c["t_hit"]), None, None, None, s())}
        c["bytes"] = {"row_count": plane, "row_fill": plane + 12 * total, "row_scatter": 2 * plane + 8 * total, "tile_count": plane,
                      "tile_fill": plane + 16 * total}
        return c

    numbers = score[~torch.isnan(score)]
    small = float(torch.quantile(numbers[:4_000_000], args.rate))
    cases = {"inf": setup(float("inf")), "rate": setup(small)}
    same = True
    for c in cases.values():                                           # the untimed pass of every call, and the comparison
        for fn in c["calls"].values():
            fn()
        torch.cuda.synchronize()
        back = torch.where(torch.isnan(c["out"]), torch.zeros_like(score), c["out"])
        sel = score <= c["cut"][:, None]
        same = same and torch.equal(c["index"], c["tile"]) and torch.equal(c["hit"], c["t_hit"]) and \
            torch.equal(back, torch.where(sel, score, torch.zeros_like(score))) and bool(torch.isnan(c["out"]).eq(~sel).all())
    times = {k: {name: [] for name in c["calls"]} for k, c in cases.items()}
    for _ in range(args.reps):
        for k, c in cases.items():
            for name, fn in c["calls"].items():
                times[k][name].append(timed(fn))
    out = {"rows": rows, "n": n, "chunk": int(_lib.load().dig_row_select_chunk()), "nan_fraction": args.nan, "reps": args.reps,
           "outputs_equal": same, "device": torch.cuda.get_device_name(0), "cuts": {}}
    for k, c in cases.items():
        rec = {"cut": float(c["cut"][0]), "selected": c["total"], "selected_fraction": round(c["total"] / (rows * n), 6), "calls": {}}
        for name, ts in times[k].items():
            med = float(np.median(ts))
            rec["calls"][name] = {"event_ms": {"median": round(med, 4), "min": round(min(ts), 4), "max": round(max(ts), 4)},
                                  "bytes": c["bytes"][name], "of_hbm_peak_by_event_time": round(c["bytes"][name] / (med * 1e-3) / HBM_PEAK, 3)}
        out["cuts"][k] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
