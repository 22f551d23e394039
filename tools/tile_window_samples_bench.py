#!/usr/bin/env python
"""Device time of the distinct-sample window counts -- dig_tile_window_sample_keys, the second key sort, dig_tile_window_samples --
at the per-base shape of bench.py's aux_rooflines (tile_samples_bench.bench_shape: regions, cohorts, bin width, tile width,
chromosomes, mutation rows), with seeded rows, at the widths 2 and 10.  Two inputs: `uniform` (rows, cohorts and samples drawn
uniformly) and `adversarial` (half of the rows moved into ONE tile of one cohort, spread over all its samples: every sample of the
cohort hits that tile, S heads on one address).  The join, dig_tile_sample_keys and the first sort are made once per input and are
not timed.  Per input the outputs are compared first: width 1 against k_samples of dig_tile_sample_counts, every width against a
count made with torch alone (the distinct (row, sample, window) triples, torch.unique and bincount).  Then 3 untimed launches and the
median of 20 timed by device events, with min and max.

dig_tile_window_samples is one call (memset, difference kernel, scan).  It is timed whole, with no keys at all (the memset alone) and
with as many keys that count nowhere (memset, a difference kernel that reads its keys and adds nothing, scan); `diff_atomics_ms` and
`scan_and_diff_reads_ms` are the differences of the medians.  For context: dig_tile_sample_counts and dig_tile_window_test on the
same input.  One JSON line.

    python tools/tile_window_samples_bench.py
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tile_samples_bench import bench_shape, card  # noqa: E402

WIDTHS = (2, 10)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples-per-cohort", type=int, default=100)
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
    sb = max(1, int(S).bit_length())                                   # the bits that hold 0 .. S

    def inputs(adversarial):
        rng = np.random.default_rng(args.seed)
        chrom, start = rng.integers(0, n_chrom, M), rng.integers(0, per * W, M).astype(np.int64)
        cohort = rng.integers(0, C, M).astype(np.int32)
        sample = (cohort * spc + rng.integers(0, spc, M)).astype(np.int32)
        if adversarial:
            half = rng.permutation(M)[:M // 2]
            chrom[half], start[half], cohort[half] = chrom[0], start[0], cohort[0]
            sample[half] = cohort[0] * spc + np.arange(len(half)) % spc
        mc, ms = be.arr(chrom, "i64"), be.arr(start, "i64")
        pm, pb = engine.overlap_join(be, start_key, runmax_key, blk_end, mc, ms, ms + 1)
        pr = be.arr(order, "i32")[pb.long()]
        n = int(pm.shape[0])
        co, sa, keys = be.arr(cohort, "i32"), be.arr(sample, "i32"), be.empty(n, "i64")       # (held until the sort below has run)
        _lib.call("dig_tile_sample_keys", p(pm), p(pr), n, p(ms), M, p(co), p(sa), None, p(first_pos), p(n_valid), B, T, R, C, S, p(keys), s())
        keys = keys.sort()[0]
        torch.cuda.synchronize()
        return keys, n

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

    def with_torch(keys_sm, width):
        """s_w from the distinct (row, sample, tile) triples with torch alone (n_valid = T everywhere: windows 0 .. T - width)."""
        u = torch.unique(keys_sm[keys_sm != torch.iinfo(torch.int64).max])
        q, t = u // T, u % T
        w = t[:, None] - torch.arange(width, device=dev)[None, :]                         # the windows that hold tile t
        ok = (w >= 0) & (w <= T - width)
        trip = torch.unique((q[:, None] * T + w)[ok])                                   # (row, sample, window), once each
        slot = (trip // T >> sb) * T + trip % T
        return torch.bincount(slot, minlength=C * R * T).reshape(C, R, T).int()

    out = {"shape": dict(sh, M=M, T=T, samples=S, widths=list(WIDTHS)), "card": card(), "launches": args.launches, "warmups": args.warmups}
    for name in ("uniform", "adversarial"):
        keys, n = inputs(name == "adversarial")
        keys_sm, nowhere = be.empty(n, "i64"), torch.full((n,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=dev)
        s_w, k_cap, k_samples = (be.empty((C, R, T), "i32") for _ in range(3))
        state = {"sorted": keys_sm}
        pt = torch.full((C, R, T), 1.0 / T, dtype=torch.float64, device=dev)
        mu = torch.full((C, R), 3.0, dtype=torch.float64, device=dev)
        win = dict(pt=be.empty((C, R, T), "f64"), k=be.empty((C, R, T), "i32"), exp=be.empty((C, R, T), "f64"),
                   pval=be.empty((C, R, T), "f64"), n_windows=be.empty(R, "i32"))

        def rekey():
            _lib.call("dig_tile_window_sample_keys", p(keys), n, C, R, T, S, p(keys_sm), s())

        def sort_keys():
            state["sorted"] = keys_sm.sort()[0]

        def samples(width, src=None, count=n):
            _lib.call("dig_tile_window_samples", p(state["sorted"] if src is None else src), count, p(n_valid), C, R, T, S, width, p(s_w), s())

        def counts():
            _lib.call("dig_tile_sample_counts", p(keys), n, C, R, T, S, 0, p(k_cap), p(k_samples), s())

        def window_test(width):
            _lib.call("dig_tile_window_test", p(pt), p(k_cap), p(mu), p(mu), p(n_valid), C, R, T, width, p(win["pt"]), p(win["k"]), p(win["exp"]),
                      p(win["pval"]), p(win["n_windows"]), s())

        rekey(), sort_keys(), counts(), samples(1)
        res = {"pairs": n, "width_1_equals_k_samples": bool(torch.equal(s_w, k_samples)), "most_samples_of_a_tile": int(k_samples.max())}
        for what, fn in (("rekey", rekey), ("sort", sort_keys), ("tile_sample_counts", counts)):
            res[what + "_ms"] = timed(fn)
        res["memset_ms"] = timed(lambda: samples(2, count=0))
        for width in WIDTHS:
            samples(width)
            want = with_torch(state["sorted"], width)
            r = {"equals_torch_count": bool(torch.equal(s_w, want)), "s_w_sum": int(s_w.sum()), "s_w_max": int(s_w.max())}
            del want
            r["window_samples_ms"] = timed(lambda: samples(width))
            r["no_key_counts_ms"] = timed(lambda: samples(width, src=nowhere))
            r["diff_atomics_ms"] = round(r["window_samples_ms"]["median"] - r["no_key_counts_ms"]["median"], 4)
            r["scan_and_diff_reads_ms"] = round(r["no_key_counts_ms"]["median"] - res["memset_ms"]["median"], 4)
            r["chain_ms"] = timed(lambda: (rekey(), sort_keys(), samples(width)))
            r["tile_window_test_ms"] = timed(lambda: window_test(width))
            res["width_%d" % width] = r
        out[name] = res
        del keys, keys_sm, nowhere, s_w, k_cap, k_samples, state, pt, mu, win
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
