#!/usr/bin/env python
"""What --pairs adds to `DigDriver.py elementCohorts --fdr 0.1`, files to files, on BASELINE configs[2] written as files by
tools/e2e_bench.py's write_inputs (37 maps, the element container, 37 mutation files; untimed): the wall-clock of the whole command
as a FRESH process -- interpreter start, imports, device initialisation, reading, the pass, the calls, and with --pairs the bit
rows, the pair tests, their q-values and the 37 <outpfx>.pairs.txt --, the two commands ALTERNATED, --reps each, after one untimed
run of each (page cache, code objects).

    python tools/element_pairs_e2e.py [--reps 5] [--workdir DIR] [--baseline-root DIR]

--baseline-root: another checkout of the project (built) whose scripts/DigDriver.py runs the command WITHOUT --pairs: the parent
commit, for the figure of DESIGN.md.  Default: this checkout.  One JSON line."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bins", type=int, default=288_000)
    ap.add_argument("--elements", type=int, default=120_091)
    ap.add_argument("--cohorts", type=int, default=37)
    ap.add_argument("--mut-rows", type=int, default=300_000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--fdr", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs-min-samples", type=int, default=1)
    ap.add_argument("--workdir", default="/tmp/dig_pairs_e2e")
    ap.add_argument("--baseline-root", default=ROOT)
    ap.add_argument("--keep", action="store_true")
    args = ap.parse_args()
    import e2e_bench
    os.makedirs(args.workdir, exist_ok=True)
    paths = e2e_bench.write_inputs(types.SimpleNamespace(bins=args.bins, elements=args.elements, cohorts=args.cohorts, mut_rows=args.mut_rows,
                                                         seed=args.seed), args.workdir)
    prefixes = ["cohort%02d" % c for c in range(args.cohorts)]

    def command(root, outdir, pairs):
        return [sys.executable, os.path.join(root, "scripts", "DigDriver.py"), "elementCohorts", paths["ed"], "elts", "--outdir", outdir,
                "--mutation-files", *paths["mut"], "--maps", *paths["pre"], "--outpfx", *prefixes, "--fdr", repr(args.fdr)] + \
               (["--pairs", "--pairs-fdr", "0.1", "--pairs-min-samples", str(args.pairs_min_samples)] if pairs else [])

    runs = {"with_pairs": command(ROOT, os.path.join(args.workdir, "out_pairs"), True),
            "without_pairs": command(os.path.abspath(args.baseline_root), os.path.join(args.workdir, "out_plain"), False)}
    times = {k: [] for k in runs}
    for rep in range(args.reps + 1):                             # (the first round is not timed)
        for name, cmd in runs.items():
            t0 = time.perf_counter()
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
            if rep:
                times[name].append(time.perf_counter() - t0)
    hits = lambda d: {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.endswith(".hits.txt")}
    a, b = hits(os.path.join(args.workdir, "out_pairs")), hits(os.path.join(args.workdir, "out_plain"))
    stat = lambda ts: {"median": round(float(np.median(ts)), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}
    res = {"what": "elementCohorts --fdr %g [--pairs --pairs-fdr 0.1], %d cohorts x %d elements, files to files, fresh processes alternated" % (
               args.fdr, args.cohorts, args.elements), "reps": args.reps, "baseline_root_is_this_checkout": os.path.abspath(args.baseline_root) == ROOT,
           "wall_s": {k: stat(v) for k, v in times.items()}, "hit_files": len(a), "hit_files_identical": a == b,
           "pair_files": len([f for f in os.listdir(os.path.join(args.workdir, "out_pairs")) if f.endswith(".pairs.txt")]),
           "pair_rows": sum(sum(1 for _ in open(os.path.join(args.workdir, "out_pairs", f))) - 1
                            for f in os.listdir(os.path.join(args.workdir, "out_pairs")) if f.endswith(".pairs.txt")),
           "hit_rows": sum(v.count(b"\n") - 1 for v in a.values())}
    res["added_by_pairs_s"] = round(res["wall_s"]["with_pairs"]["median"] - res["wall_s"]["without_pairs"]["median"], 3)
    if not args.keep:
        shutil.rmtree(args.workdir, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
