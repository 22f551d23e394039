#!/usr/bin/env python
"""Device time of dig_pair_bits and dig_pair_fisher -- the pairs of the element route -- on random incidence rows: --cohorts (37)
cohorts of --rows (2 000) called elements over --samples (2 800) samples at --density (0.02), and one cohort of 8 192 rows.  Beside
dig_pair_fisher, in the same run: dig_pair_counts (the same kernel with the tail rule compiled out: how the time splits between the
counts and the tails) and, for the counts alone, torch's B.half() @ B.half().T per cohort.  Every call is timed by stream events,
--reps (20) times after an untimed pass; one JSON line with the medians, the pairs per second and the share of the tails.

    python tools/pair_fisher_bench.py
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cohorts", type=int, default=37)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--samples", type=int, default=2800)
    ap.add_argument("--density", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=5)
    args = ap.parse_args()
    import torch
    from digdriver_amd import _lib, engine
    _lib.require_device()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    p, s = _lib.dev_ptr, _lib.stream_ptr

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def problem(C, H, n):
        plan = engine.pair_plan([H] * C, [n] * C)
        m = torch.rand((C * H, n), generator=gen, device=dev) < args.density
        at = torch.nonzero(m)
        row, sample = at[:, 0].to(torch.int32).contiguous(), at[:, 1].to(torch.int32).contiguous()
        Ht, W, P, T = plan["H_total"], plan["W"], plan["n_pairs"], len(plan["tiles"])
        bits = torch.zeros((Ht, W), dtype=torch.int64, device=dev)
        d = {k: torch.as_tensor(plan[k], device=dev) for k in ("row_ptr", "n_samples", "pair_ptr", "tiles")}
        lnfact = torch.empty(plan["n_max"] + 1, dtype=torch.float64, device=dev)
        n_row, n_both = torch.empty(Ht, dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.int32, device=dev)
        p_co, p_ex = torch.empty(P, dtype=torch.float64, device=dev), torch.empty(P, dtype=torch.float64, device=dev)
        head = lambda: (p(bits), Ht, W, p(d["row_ptr"]), p(d["n_samples"]), p(d["pair_ptr"]), C, p(d["tiles"]), T, P, plan["n_max"], plan["h_max"])
        half = m.view(C, H, n).half()
        calls = {
            "pair_bits": lambda: _lib.call("dig_pair_bits", p(row), p(sample), row.shape[0], Ht, W, p(bits), s()),
            "pair_fisher": lambda: _lib.call("dig_pair_fisher", *head(), p(lnfact), p(n_row), p(n_both), p(p_co), p(p_ex), s()),
            "pair_counts": lambda: _lib.call("dig_pair_counts", *head(), p(n_row), p(n_both), s()),
            "torch_half_matmul": lambda: torch.bmm(half, half.transpose(1, 2)),
        }
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, fn in calls.items():
                times[k].append(timed(fn))
        med = {k: float(np.median(v)) for k, v in times.items()}
        res = {"C": C, "H": H, "n": n, "W": W, "keys": int(row.shape[0]), "pairs": P, "tiles": T,
               "event_ms": {k: {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in times.items()},
               "pairs_per_second": round(P / (med["pair_fisher"] * 1e-3)),
               "share_of_the_tails": round(1.0 - med["pair_counts"] / med["pair_fisher"], 3),
               "pval_cooccur_min": float(p_co.min()), "n_both_mean": round(float(n_both.double().mean()), 4)}
        return res

    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "density": args.density,
           "cohorts": problem(args.cohorts, args.rows, args.samples), "one_cohort_of_8192": problem(1, 8192, args.samples)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
