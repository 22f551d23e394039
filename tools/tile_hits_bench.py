#!/usr/bin/env python
"""Device time of the hit selection of the per-base route, engine.tile_select (dig_tile_select_count, a cumulative sum,
dig_tile_select_fill), beside the torch statement of the same result -- (score <= cut) & valid, nonzero, four gathers -- on seeded
synthetic planes at the per-GPU size of BASELINE configs[4]: C = 37 cohorts, R = 36 000 regions, T = 200 tiles, uniform p-values,
cut 1e-4 (about 27 000 hits).  The parent of this route has no selection entry point, so the torch statement is the comparison.
The outputs of the two are compared first; then they take turns, behind one untimed pass of each, for --rounds rounds timed by
device events.  The count pass is also timed alone: its bytes (8 C R T) over its time.  One JSON line.

    python tools/tile_hits_bench.py --rounds 20
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
    ap.add_argument("--regions", type=int, default=36_000)
    ap.add_argument("--tiles", type=int, default=200)
    ap.add_argument("--cut", type=float, default=1e-4)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--seed", type=int, default=5)
    args = ap.parse_args()
    import torch
    from digdriver_amd import _lib, engine
    _lib.require_device()
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    C, R, T = args.cohorts, args.regions, args.tiles
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    score = torch.rand((C, R, T), generator=gen, device=dev, dtype=torch.float64)
    pt = torch.rand((C, R, T), generator=gen, device=dev, dtype=torch.float64)
    ex = torch.rand((C, R, T), generator=gen, device=dev, dtype=torch.float64) * 40
    k = torch.randint(0, 9, (C, R, T), generator=gen, device=dev, dtype=torch.int32)
    n_valid = torch.full((R,), T, dtype=torch.int32, device=dev)
    n_valid[::97] = T - 3                                                # some ragged regions; their tiles past the end are NaN
    score[:, ::97, T - 3:] = float("nan")
    cut = torch.full((C,), args.cut, dtype=torch.float64, device=dev)

    def ours():
        return engine.tile_select(score, n_valid, cut, pt=pt, exp=ex, k=k)

    def torch_statement():
        valid = torch.arange(T, device=dev)[None, None, :] < n_valid[None, :, None]
        hit = (score <= cut[:, None, None]) & valid
        c, r, t = torch.nonzero(hit, as_tuple=True)
        flat = (c * R + r) * T + t
        return dict(region=r.to(torch.int32), tile=t.to(torch.int32), score=score.reshape(-1)[flat], pt=pt.reshape(-1)[flat],
                    exp=ex.reshape(-1)[flat], k=k.reshape(-1)[flat], cohort_ptr=torch.searchsorted(c, torch.arange(C + 1, device=dev)).cpu().numpy())

    def count_pass():
        counts = torch.empty(C * R, dtype=torch.int32, device=dev)
        _lib.call("dig_tile_select_count", _lib.dev_ptr(score), _lib.dev_ptr(n_valid), _lib.dev_ptr(cut), C, R, T, _lib.dev_ptr(counts),
                  _lib.stream_ptr())
        return counts

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), res

    # the untimed pass of each (code objects, allocator), and the comparison of their outputs
    got, want = ours(), torch_statement()
    count_pass()
    same = bool(np.array_equal(got["cohort_ptr"], want["cohort_ptr"])) and all(
        torch.equal(got[n], want[n]) for n in ("region", "tile", "score", "pt", "exp", "k"))
    hits = int(got["cohort_ptr"][-1])
    del got, want
    times = {"tile_select": [], "torch_statement": [], "count_pass": []}
    for _ in range(args.rounds):
        times["tile_select"].append(timed(ours)[0])
        times["torch_statement"].append(timed(torch_statement)[0])
        times["count_pass"].append(timed(count_pass)[0])
    out = {"C": C, "R": R, "T": T, "cut": args.cut, "hits": hits, "outputs_equal": same, "rounds": args.rounds}
    for name, ts in times.items():
        out[name + "_ms"] = {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}
    plane_bytes = 8 * C * R * T
    out["count_pass_bytes"] = plane_bytes
    out["count_pass_TBps"] = round(plane_bytes / (float(np.median(times["count_pass"])) * 1e-3) / 1e12, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
