#!/usr/bin/env python
"""Device time of the two kernels behind the meta-cohorts of the element route -- dig_group_fisher and dig_group_sums -- on a seeded
plane of the flagship size: p f64 [4, 37, 120 091], uniform p-values with about 1 % NaN, for M = 8 groups (one of all 37 cohorts, seven
of 3 - 12 cohorts: the compiled form of up to 8 accumulators) and for M = 32 groups (the same eight, then 24 more of 3 - 12: the form of
up to 32).  Beside them a plain torch formulation of the same p-values on the same inputs in the same process: the masked -log, one sum
per group over its member rows, torch.special.gammaincc(m, s).  The outputs are compared first (the counts exactly, the p-values by
their largest relative difference where both are at least 1e-250).  Then, per repetition, every call runs once in a fixed order
between device events:

    fisher M = 8, sums M = 8 (gated), fisher M = 32, sums M = 32 (gated), torch M = 8, torch M = 32            x --reps

so that a kernel trace of the process (rocprofv3 --kernel-trace --stats -- python tools/group_fisher_bench.py) lists the dispatches of
group_fisher_kernel<8> / <32> and group_sums_kernel<8> / <32>: the LAST --reps dispatches of each are the timed ones.  One JSON line:
the event times and the bytes each call moves by its algorithm (fisher: 8 R C E read, (8 + 4) R M E written; gated sums: 16 R C E read,
8 R M E written) over them.

    python tools/group_fisher_bench.py --reps 5
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
    ap.add_argument("--R", type=int, default=4)
    ap.add_argument("--C", type=int, default=37)
    ap.add_argument("--E", type=int, default=120_091)
    ap.add_argument("--nan", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    args = ap.parse_args()
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    dev = torch.device("cuda:0")
    R, C, E = args.R, args.C, args.E
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    pv = torch.rand((R, C, E), generator=gen, device=dev, dtype=torch.float64)
    pv[torch.rand((R, C, E), generator=gen, device=dev) < args.nan] = float("nan")
    x = torch.rand((R, C, E), generator=gen, device=dev, dtype=torch.float64)
    rng = np.random.default_rng(args.seed)
    rows = [np.ones(C, bool)]
    while len(rows) < 32:
        row = np.zeros(C, bool)
        row[rng.choice(C, size=int(rng.integers(3, min(12, C) + 1)), replace=False)] = True
        rows.append(row)
    members = {M: torch.as_tensor(np.stack(rows[:M]).astype(np.uint8), device=dev) for M in (8, 32)}
    p, s = _lib.dev_ptr, _lib.stream_ptr

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def torch_form(member):
        """The same p-values in plain torch: (pval [R, M, E], m [R, M, E])."""
        ok = ~torch.isnan(pv)
        t = torch.where(ok, -torch.log(torch.where(ok, pv, torch.ones_like(pv))), torch.zeros_like(pv))
        out, cnt = [], []
        for row in member.bool():
            sg, m = t[:, row].sum(dim=1), ok[:, row].sum(dim=1)
            out.append(torch.where(m > 0, torch.special.gammaincc(m.clamp(min=1).double(), sg), torch.full_like(sg, float("nan"))))
            cnt.append(m)
        return torch.stack(out, dim=1), torch.stack(cnt, dim=1)

    cases, calls, nbytes = {}, {}, {}
    for M, member in members.items():
        c = cases[M] = dict(pval=torch.empty((R, M, E), dtype=torch.float64, device=dev), n=torch.empty((R, M, E), dtype=torch.int32, device=dev),
                            sums=torch.empty((R, M, E), dtype=torch.float64, device=dev))
        calls["fisher_M%d" % M] = lambda M=M, member=member, c=c: _lib.call("dig_group_fisher", p(pv), p(member), R, C, E, M, p(c["pval"]),
                                                                             p(c["n"]), s())
        calls["sums_M%d" % M] = lambda M=M, member=member, c=c: _lib.call("dig_group_sums", p(x), p(pv), p(member), R, C, E, M, p(c["sums"]), s())
        nbytes["fisher_M%d" % M] = 8 * R * C * E + 12 * R * M * E
        nbytes["sums_M%d" % M] = 16 * R * C * E + 8 * R * M * E
    for M, member in members.items():
        calls["torch_M%d" % M] = lambda member=member: torch_form(member)
        nbytes["torch_M%d" % M] = nbytes["fisher_M%d" % M]
    # the untimed pass of every call, and the comparison
    compare = {}
    for M, member in members.items():
        calls["fisher_M%d" % M]()
        calls["sums_M%d" % M]()
        ref, m = torch_form(member)
        torch.cuda.synchronize()
        c = cases[M]
        both = (ref >= 1e-250) & (c["pval"] >= 1e-250) & (m >= 3)
        rel = ((c["pval"] - ref).abs() / ref)[both]
        want = torch.stack([torch.where(torch.isnan(pv[:, row]), torch.zeros_like(x[:, row]), x[:, row]).sum(dim=1) for row in member.bool()], dim=1)
        compare["M%d" % M] = {"counts_equal": bool(torch.equal(c["n"].long(), m)), "nan_equal": bool(torch.equal(torch.isnan(ref), torch.isnan(c["pval"]))),
                              "pval_largest_relative_difference_from_3_members": float(rel.max()) if rel.numel() else 0.0,
                              "sums_largest_relative_difference": float(((c["sums"] - want).abs() / want.abs().clamp(min=1e-300)).max())}
    times = {name: [] for name in calls}
    for _ in range(args.reps):
        for name, fn in calls.items():
            times[name].append(timed(fn))
    out = {"R": R, "C": C, "E": E, "nan_fraction": args.nan, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "group_sizes": [int(r.sum()) for r in rows], "compare_with_torch": compare, "calls": {}}
    for name, ts in times.items():
        med = float(np.median(ts))
        out["calls"][name] = {"event_ms": {"median": round(med, 4), "min": round(min(ts), 4), "max": round(max(ts), 4)},
                              "bytes": nbytes[name], "of_hbm_peak_by_event_time": round(nbytes[name] / (med * 1e-3) / HBM_PEAK, 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
