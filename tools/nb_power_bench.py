#!/usr/bin/env python
"""Device time of dig_nb_power -- the critical counts of the element route's SNV burden test and the power at them -- on the planes of
the flagship problem: bench.make_workload's 120 091 elements x 37 cohorts through engine.element_pipeline, then ALPHA, THETA, P0 and
PVAL_SNV_BURDEN as [37, 120 091] planes, CJ as the scale.  Two level vectors: the `fdr` rule of cohort_batch.power_levels at 0.1 and
a flat 1e-6; three folds (2, 5, 10).  Beside them, as the yardstick, dig_nb_midp_upper over the same 4.4 M pairs at k = OBS_SNV: the
p-value evaluations that one critical count plus three powers cost.  Per repetition every call runs once in a fixed order between
device events:

    nb_power at the fdr levels, nb_power at 1e-6, nb_midp_upper at OBS_SNV            x --reps

so that a kernel trace of the process (rocprofv3 --kernel-trace --stats -- python tools/nb_power_bench.py --reps 5) lists the dispatches
of nb_power_kernel and nb3_kernel: the LAST 2 x --reps and --reps of them are the timed ones (--trace-csv FILE reads them from the
trace's kernel CSV in a second step).  One JSON line: the event times, the levels and what the counts look like.

    python tools/nb_power_bench.py --reps 5
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def from_trace(path, reps):
    """The timed dispatches of a rocprofv3 kernel-trace CSV (in start order, the last ones of each kernel): ms per call."""
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    ms = lambda name: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6 for r in rows if name in r["Kernel_Name"]]
    power, yard = ms("nb_power_kernel")[-2 * reps:], ms("nb3_kernel")[-reps:]
    stat = lambda ts: {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4), "n": len(ts)}
    return {"nb_power_fdr": stat(power[0::2]), "nb_power_flat": stat(power[1::2]), "nb_midp_upper": stat(yard)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--elements", type=int, default=120_091)
    ap.add_argument("--cohorts", type=int, default=37)
    ap.add_argument("--bins", type=int, default=288_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--trace-csv", default=None, help="no GPU run: summarise the kernel CSV of a trace of this tool run with the same --reps")
    args = ap.parse_args()
    if args.trace_csv:
        print(json.dumps({"kernel_trace_ms": from_trace(args.trace_csv, args.reps)}))
        return
    import torch
    from bench import make_workload
    from digdriver_amd import _lib, engine
    from digdriver_amd.driver_model import cohort_batch
    from digdriver_amd.sequence_model import nb_model
    _lib.require_device()
    dev = torch.device("cuda:0")
    w = make_workload(n_bins=args.bins, n_elements=args.elements, n_cohorts=args.cohorts, seed=args.seed)
    td = {k: torch.as_tensor(v, device=dev) for k, v in w.items() if isinstance(v, np.ndarray)}
    acc, st = engine.element_pipeline(td["bin_mu"], td["bin_std"], td["bin_y"], td["bin_flag"], td["bin_ctx"], td["ov_ptr"], td["ov_idx"],
                                      td["L"], td["strand_minus"], td["d_pr"], td["obs_snv"], td["obs_samples"], td["obs_indel"],
                                      td["cj"], td["cj_indel"])
    by_cohort = lambda x: x.transpose(0, 1).contiguous()
    alpha, theta = (by_cohort(x) for x in nb_model.normal_params_to_gamma(acc["MU"], acc["SIGMA"]))
    pi, pval, obs, cj = by_cohort(acc["P"][:, 0, :]), by_cohort(st[1]), by_cohort(td["obs_snv"]).double(), td["cj"].double()
    C, E = alpha.shape
    levels = {"fdr": cohort_batch.power_levels(pval, fdr=0.1), "flat": (np.full(C, 1e-6), None, None)}
    folds = torch.tensor([2.0, 5.0, 10.0], dtype=torch.float64, device=dev)
    k_crit, power = torch.empty((C, E), dtype=torch.int32, device=dev), torch.empty((3, C, E), dtype=torch.float64, device=dev)
    p1 = 1.0 / ((theta * cj[:, None]) * pi + 1.0)
    out = torch.empty_like(p1)
    p, s = _lib.dev_ptr, _lib.stream_ptr
    calls, shape = {}, {}
    for name, (level, _, _) in levels.items():
        lv = torch.as_tensor(level, device=dev)
        calls["nb_power_" + name] = lambda lv=lv: _lib.call("dig_nb_power", p(alpha), p(theta), p(pi), p(cj), p(lv), C, E, p(folds), 3,
                                                            1 << 20, p(k_crit), p(power), s())
    calls["nb_midp_upper"] = lambda: _lib.call("dig_nb_midp_upper", p(obs), p(alpha), p(p1), p(out), C * E, s())

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for name, fn in calls.items():                                   # the untimed pass of every call, and what the counts look like
        fn()
        torch.cuda.synchronize()
        if name.startswith("nb_power"):
            K = k_crit[k_crit >= 0].double()
            q = torch.quantile(K[:: max(1, K.numel() // 1_000_000)], torch.tensor([0.5, 0.99], dtype=torch.float64, device=dev))
            top = power[2]
            shape[name] = {"k_crit_median": float(q[0]), "k_crit_p99": float(q[1]), "k_crit_max": int(K.max()),
                           "undefined_or_out_of_reach": int((k_crit < 0).sum()),
                           "share_powered_at_fold_10_power_0.8": round(float((top >= 0.8).double().mean()), 4)}
    times = {name: [] for name in calls}
    for _ in range(args.reps):
        for name, fn in calls.items():
            times[name].append(timed(fn))
    res = {"C": C, "E": E, "pairs": C * E, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "levels_fdr_0.1": {"min": float(np.nanmin(levels["fdr"][0])), "max": float(np.nanmax(levels["fdr"][0])),
                              "hits": int(levels["fdr"][2].sum())}, "counts": shape, "event_ms": {}}
    for name, ts in times.items():
        res["event_ms"][name] = {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}
    for name in ("nb_power_fdr", "nb_power_flat"):
        res["event_ms"][name]["midp_evaluations_by_median"] = round(res["event_ms"][name]["median"] / res["event_ms"]["nb_midp_upper"]["median"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
