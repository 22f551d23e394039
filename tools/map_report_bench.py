#!/usr/bin/env python
"""Device time of the map report's two entry points at the size of a whole-genome run: N = 288 000 bins, C = 37 cohorts, synthetic
cohort-major tables in the style of BASELINE cfg3 (Y_PRED ~ Gamma(9, 3), STD ~ Gamma(4, 1), Y_TRUE ~ Poisson(Y_PRED), FLAG on a tenth
of the bins), 24 chromosomes of equal length, scales 1 / 5 / 10 / 100 bins.  Per scale dig_map_windows and dig_map_scores are timed
between device events, --reps times after an untimed pass, in a fixed order; beside the scale-1 launch one dig_nb_midp_upper launch
over the same M C (k, alpha, p) triples (formed from the scale-1 planes), in the same process: the same tests without the merge, the
five output planes and the input stream.

The algorithmic bytes of a dig_map_windows launch are C N (8 + 8 + 4 [+ 1 with --drop-flagged]) read + 8 (M + 1) of run_ptr + C M 36
written; `hbm_share` is their time at the measured streaming peak of the card (6.29 TB/s by a float4 copy) over the event time.

--reference-seconds: no GPU; times the reference's gp_tools.merge_windows on the CPU on grids of --reference-bins bins at scale 10
(M windows, three masks of N rows each: O(M N) per cohort) and prints the extrapolation to 288 000 bins x 37 cohorts as an
extrapolation.  Needs the reference tree (DIG_REFERENCE) and pandas.

    python tools/map_report_bench.py --reps 20
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 6.29e12                                        # bytes / s, measured float4 copy
W = 10_000


def make_tables(N, C, seed, n_chrom=24):
    rng = np.random.default_rng(seed)
    per = -(-N // n_chrom)
    chrom = np.minimum(np.arange(N) // per, n_chrom - 1).astype(np.int32) + 1
    start = (np.arange(N) - (chrom - 1).astype(np.int64) * per) * W
    mu = rng.gamma(9.0, 3.0, (C, N))
    sd = rng.gamma(4.0, 1.0, (C, N))
    y = rng.poisson(mu).astype(np.int32)
    flag = (rng.uniform(size=(1, N)) < 0.1).repeat(C, axis=0).astype(np.uint8)
    return chrom, start, mu, sd, y, flag


def reference_seconds(sizes, scale, seed):
    import types
    import pandas as pd
    for name in ["h5py", "seaborn"]:
        sys.modules.setdefault(name, types.ModuleType(name))
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, os.environ.get("DIG_REFERENCE", "/root/reference"))
    from DIGDriver.sequence_model import gp_tools
    from digdriver_amd.region_model import map_report
    runs = []
    for n_bins in sizes:
        chrom, start, mu, sd, y, _ = make_tables(n_bins, 1, seed, n_chrom=1)
        df = pd.DataFrame(dict(CHROM=chrom, START=start, END=start + W, Y_TRUE=y[0], Y_PRED=mu[0], STD=sd[0]))
        ptr, c, s, e = map_report.merged_runs(chrom, start, scale * W)
        t0 = time.perf_counter()
        gp_tools.merge_windows(df, np.column_stack([c, s, e]))
        runs.append({"bins": n_bins, "windows": len(ptr) - 1, "cpu_seconds_measured": round(time.perf_counter() - t0, 4)})
    # per merged window: a fixed cost a (three pandas selections) + b per row of the frame (three boolean masks): t = M (a + b N)
    (n1, m1, t1), (n2, m2, t2) = [(r["bins"], r["windows"], r["cpu_seconds_measured"]) for r in (runs[0], runs[-1])]
    b = (t2 / m2 - t1 / m1) / (n2 - n1)
    a = t1 / m1 - b * n1
    N, M = 288_000, 288_000 // scale
    full = M * (a + b * N)
    return {"reference_merge_windows": {"scale": scale, "runs": runs, "fit_seconds_per_window": {"fixed": a, "per_row": b},
                                        "extrapolated_seconds_one_cohort_288000_bins": round(full, 1),
                                        "extrapolated_seconds_37_cohorts": round(37 * full, 1),
                                        "note": "extrapolation by t = M (a + b N) fitted to the first and last run, not a measurement"}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bins", type=int, default=288_000)
    ap.add_argument("--cohorts", type=int, default=37)
    ap.add_argument("--scales", type=int, nargs="+", default=[1, 5, 10, 100])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--drop-flagged", action="store_true")
    ap.add_argument("--reference-seconds", action="store_true")
    ap.add_argument("--reference-bins", type=int, nargs="+", default=[599, 6000, 30000])
    args = ap.parse_args()
    if args.reference_seconds:
        print(json.dumps(reference_seconds(args.reference_bins, 10, args.seed)))
        return
    import torch
    from digdriver_amd import _lib, engine
    from digdriver_amd.region_model import map_report
    from digdriver_amd.sequence_model import nb_model
    _lib.require_device()
    dev = torch.device("cuda:0")
    N, C = args.bins, args.cohorts
    chrom, start, mu, sd, y, flag = make_tables(N, C, args.seed)
    on = lambda x: torch.as_tensor(x, device=dev)
    mu, sd, y, flag = on(mu), on(sd), on(y), on(flag) if args.drop_flagged else None

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    calls, info = {}, {}
    for s in args.scales:
        ptr = on(map_report.merged_runs(chrom, start, s * W)[0])
        M = int(ptr.shape[0]) - 1
        planes = engine.map_windows(mu, sd, y, flag, ptr, drop_flagged=args.drop_flagged)
        calls["map_windows_s%d" % s] = lambda ptr=ptr: engine.map_windows(mu, sd, y, flag, ptr, drop_flagged=args.drop_flagged)
        calls["map_scores_s%d" % s] = lambda P=planes: engine.map_scores(P["n_bins"], P["y_true"], P["y_pred"], P["pval"])
        info[s] = {"M": M, "bytes": C * N * (20 + bool(args.drop_flagged)) + 8 * (M + 1) + C * M * 36}
        if s == 1:
            alpha, theta = nb_model.normal_params_to_gamma(planes["y_pred"], planes["std"])
            k, p1, out = planes["y_true"].double().contiguous(), (1.0 / (theta + 1.0)).contiguous(), torch.empty_like(theta)
            alpha = alpha.contiguous()
            calls["nb_midp_upper_same_triples"] = lambda n=C * M: _lib.call("dig_nb_midp_upper", _lib.dev_ptr(k), _lib.dev_ptr(alpha), _lib.dev_ptr(p1),
                                                                            _lib.dev_ptr(out), n, _lib.stream_ptr())
    for fn in calls.values():                             # the untimed pass of every call
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for _ in range(args.reps):
        for name, fn in calls.items():
            times[name].append(timed(fn))
    res = {"N": N, "C": C, "reps": args.reps, "drop_flagged": bool(args.drop_flagged), "device": torch.cuda.get_device_name(0), "event_ms": {}}
    for name, ts in times.items():
        res["event_ms"][name] = {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}
    for s in args.scales:
        e = res["event_ms"]["map_windows_s%d" % s]
        e["M"], e["algorithmic_bytes"] = info[s]["M"], info[s]["bytes"]
        e["hbm_share"] = round(info[s]["bytes"] / HBM_PEAK / (e["median"] * 1e-3), 4)
    if 1 in args.scales:
        res["scale_1_over_elementwise"] = round(res["event_ms"]["map_windows_s1"]["median"] / res["event_ms"]["nb_midp_upper_same_triples"]["median"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
