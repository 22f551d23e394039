#!/usr/bin/env python
"""Device time of one pass of the copy-number training labels, dig_cnv_segment_deltas and dig_cnv_window_means, at the workload's
size: 288 000 windows of 10 kb on 22 chromosomes, 37 cohorts, 300 000 synthetic segments per cohort with seeded log-uniform lengths from
10 kb to 50 Mb and uniform starts, cp_num from {0, 1, 2, 3, 4, 8}.  The labels of 24 windows (the first and last of a chromosome, the
windows on either side of a boundary between two chunks of the scan, and seeded ones) are first checked against a per-base-equivalent
closed-form sum in numpy, exactly; then 3 untimed launches and the median and range of 20 timed by device events, per entry point.
Fractions of the HBM peak by the algorithmic bytes:
    segment deltas   33 bytes read per segment (three i64, class, weight, cohort) + the difference array zeroed once, 8 bytes per
                     element; the binary searches (into 2.3 MB of window starts, cache-resident) and the atomics are not counted
    window means     the difference array read twice (chunk sums, then the scan) and the labels written: 24 bytes per (cohort, class, window)
The whole engine call (np.unique of the windows, uploads of the window tables, both entry points, the gather back to the windows' own
order) is timed the same way, 5 runs.  One JSON line.

    python tools/cnv_windows_bench.py
"""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SEGMENT_BYTES, SCAN_BYTES = 33.0, 24.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", type=int, default=288_000)
    ap.add_argument("--cohorts", type=int, default=37)
    ap.add_argument("--segments", type=int, default=300_000, help="per cohort")
    ap.add_argument("--width", type=int, default=10_000)
    ap.add_argument("--chromosomes", type=int, default=22)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--route-runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    import torch
    from tile_samples_bench import card
    from digdriver_amd import _lib, engine
    _lib.require_device()
    lib = _lib.load()
    hbm_peak = float(re.search(r"^HBM_PEAK = ([\d.e]+)", open(os.path.join(ROOT, "bench.py")).read(), flags=re.M).group(1))
    N, C, W, n_chrom = args.windows, args.cohorts, args.width, args.chromosomes
    per = -(-N // n_chrom)
    rng = np.random.default_rng(args.seed)
    win_chrom = np.repeat(np.arange(1, n_chrom + 1, dtype=np.int64), per)[:N]
    win_start = (np.tile(np.arange(per, dtype=np.int64), n_chrom) * W)[:N]
    n = C * args.segments
    chrom = rng.integers(1, n_chrom + 1, n).astype(np.int64)
    length = np.exp(rng.uniform(np.log(10_000), np.log(50_000_000), n)).astype(np.int64)
    start = rng.integers(0, per * W, n).astype(np.int64)
    end = start + length
    cp = rng.choice([0, 1, 2, 3, 4, 8], n)
    klass = np.where(cp == 2, 1, np.where(cp < 2, 2, 0)).astype(np.uint8)
    weight = np.where(cp == 2, 1, np.abs(cp - 2)).astype(np.int32)
    cohort = np.repeat(np.arange(C, dtype=np.int32), args.segments)
    up = lambda x: torch.as_tensor(x, device="cuda:0")
    segs = [up(x) for x in (chrom, start, end, klass, weight, cohort)]

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

    labels = engine.window_cnv_means(win_chrom, win_start, W, *segs, C).cpu().numpy()             # [N, 3, C]
    chunk = _lib.DIG_CNV_SCAN_CHUNK
    probe = sorted({0, per - 1, per, N - 1, chunk - 1, chunk, (N // chunk) * chunk - 1, min((N // chunk) * chunk, N - 1)} |
                   set(rng.integers(0, N, 16).tolist()))
    exact = True
    for i in probe:
        s = int(win_start[i])
        hit = np.flatnonzero((chrom == win_chrom[i]) & (start < s + W) & (end > s))
        cover = (np.minimum(end[hit], s + W) - np.maximum(start[hit], s)) * weight[hit].astype(np.int64)
        want = np.zeros((3, C), np.int64)
        np.add.at(want, (klass[hit], cohort[hit]), cover)
        exact = exact and bool(np.array_equal(labels[i], want / float(W)))
    out = {"shape": dict(windows=N, cohorts=C, segments_per_cohort=args.segments, width=W, chromosomes=n_chrom, segments=n,
                         mean_windows_per_segment=round(float(length.mean()) / W, 1)),
           "card": card(), "launches": args.launches, "warmups": args.warmups, "hbm_peak_GBps": hbm_peak / 1e9,
           "probed_windows": len(probe), "probed_windows_exact": exact, "labels_nonzero_fraction": round(float((labels > 0).mean()), 4)}
    del labels

    uniq = np.unique(np.stack([win_chrom, win_start], axis=1), axis=0)
    chrom_id, first = np.unique(uniq[:, 0], return_index=True)
    starts, ids, off = up(uniq[:, 1].copy()), up(chrom_id), up(np.concatenate([first, [N]]).astype(np.int64))
    delta_bytes, carry_bytes = int(lib.dig_cnv_segment_deltas_size(C, N)), int(lib.dig_cnv_window_means_size(C, N))
    deltas = torch.empty(delta_bytes // 8, dtype=torch.int64, device="cuda:0")
    carries = torch.empty(carry_bytes // 8, dtype=torch.int64, device="cuda:0")
    res = torch.empty((C, N, 3), dtype=torch.float64, device="cuda:0")
    p, s = _lib.dev_ptr, _lib.stream_ptr
    seg_call = lambda: _lib.call("dig_cnv_segment_deltas", p(starts), p(ids), p(off), len(chrom_id), N, W, *[p(x) for x in segs], n, C, p(deltas), s())
    scan_call = lambda: _lib.call("dig_cnv_window_means", p(deltas), N, C, W, p(res), p(carries), s())
    t = timed(seg_call, args.launches, args.warmups)
    b = SEGMENT_BYTES * n + delta_bytes
    out["segment_deltas"] = {"ms": t, "bytes": b, "hbm_frac": round(b / (t["median"] * 1e-3) / hbm_peak, 4),
                             "segments_per_us": round(n / (t["median"] * 1e3), 1)}
    t = timed(scan_call, args.launches, args.warmups)
    b = SCAN_BYTES * 3 * C * N
    out["window_means"] = {"ms": t, "bytes": b, "hbm_frac": round(b / (t["median"] * 1e-3) / hbm_peak, 4)}
    out["engine_call_ms"] = timed(lambda: engine.window_cnv_means(win_chrom, win_start, W, *segs, C), args.route_runs, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
