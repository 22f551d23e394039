#!/usr/bin/env python
"""Wall time of geneDriver for many cohorts: cohort_batch.run_gene_cohorts (one pass) beside C calls of
transfer_tools.run_gene_model(fused=True), on synthetic inputs of the bench's size -- C = 37 cohorts, G = 20 091 genes, `mut-rows`
annotated rows per cohort of which `coding` carry a gene label.  The two routes take turns (batch, serial, batch, ...) behind one
untimed pass of each; the median and the range of each go to one JSON line.

    python tools/gene_cohorts_bench.py --workdir /tmp/dig_genes --rounds 3
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_inputs(args):
    from digdriver_amd.io import mapfile
    os.makedirs(args.workdir, exist_ok=True)
    G, C = args.genes, args.cohorts
    genes = np.array(["GENE%05d" % i for i in range(G)], dtype=object)
    genes[G // 2] = "TP53"
    maps, muts = [], []
    annots = np.array(["Synonymous", "Missense", "Nonsense", "Essential_Splice", "INDEL", "Stop_loss"], dtype=object)
    for c in range(C):
        r = np.random.default_rng([args.seed, c])
        f = os.path.join(args.workdir, "genes%02d.map" % c)
        maps.append(f)
        if not os.path.exists(f):
            mu = r.uniform(5, 300, G)
            p = r.uniform(1e-3, 3e-3, (G, 4))
            mapfile.write_frame(f, "genic_model", pd.DataFrame(dict(
                CHROM=(1 + np.arange(G) % 22).astype(str), GENE=genes, GENE_LENGTH=r.integers(300, 9000, G), R_SIZE=r.integers(20000, 60000, G),
                R_OBS=r.integers(20, 900, G), R_INDEL=r.integers(2, 90, G), MU=mu, SIGMA=mu * r.uniform(0.2, 0.5, G), MU_INDEL=mu * 0.1,
                SIGMA_INDEL=mu * 0.04, FLAG=np.zeros(G, np.int64), P_MIS=p[:, 0], P_NONS=p[:, 1] * 0.1, P_SILENT=p[:, 2] * 0.4,
                P_SPLICE=p[:, 3] * 0.05, P_TRUNC=p[:, 1] * 0.1 + p[:, 3] * 0.05, P_INDEL=r.uniform(0.02, 0.2, G))))
        f = os.path.join(args.workdir, "cohort%02d.annot.txt" % c)
        muts.append(f)
        if not os.path.exists(f):
            n = args.mut_rows
            coding = r.uniform(size=n) < args.coding
            annot = np.where(coding, annots[r.choice(6, n, p=[0.24, 0.55, 0.04, 0.02, 0.13, 0.02])], "Noncoding")
            indel = annot == "INDEL"
            pos = r.integers(1000, 50_000_000, n)
            pd.DataFrame({0: r.integers(1, 23, n), 1: pos, 2: pos + np.where(indel, 4, 1), 3: np.where(indel, "ACGT", "A"),
                          4: np.where(indel, "A", "T"), 5: np.char.add("S", r.integers(0, 400, n).astype(str)),
                          6: np.where(coding, genes[r.integers(0, G, n)], "."), 7: annot}).to_csv(f, sep="\t", header=False, index=False)
    return muts, maps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workdir", default="/tmp/dig_genes")
    ap.add_argument("--cohorts", type=int, default=37)
    ap.add_argument("--genes", type=int, default=20_091)
    ap.add_argument("--mut-rows", type=int, default=300_000)
    ap.add_argument("--coding", type=float, default=0.03, help="share of the rows that carry a gene label")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--selection", action="store_true")
    args = ap.parse_args()
    from digdriver_amd.driver_model import cohort_batch, transfer_tools
    muts, maps = write_inputs(args)
    cosmic = ["GENE%05d" % i for i in range(0, args.genes, 29)]
    kw = dict(all_cosmic=cosmic, selection=args.selection)

    def batch():
        return cohort_batch.run_gene_cohorts(muts, maps, **kw)

    def serial():
        return [transfer_tools.run_gene_model(m, g, fused=True, **kw) for m, g in zip(muts, maps)]

    times = {"batch": [], "serial": []}
    with contextlib.redirect_stdout(io.StringIO()):
        a, b = batch(), serial()                                     # untimed: code objects, file cache
        same = all(list(x.columns) == list(y.columns) and all(np.array_equal(x[k].values, y[k].values) for k in x.columns if k.startswith(("OBS_", "N_SAMP_")))
                   for x, y in zip(a, b))
        for _ in range(args.rounds):
            for name, fn in (("batch", batch), ("serial", serial)):
                t0 = time.perf_counter()
                fn()
                times[name].append(time.perf_counter() - t0)
    out = {"cohorts": args.cohorts, "genes": args.genes, "mut_rows": args.mut_rows, "coding_share": args.coding, "selection": args.selection,
           "counts_equal": bool(same)}
    for name, ts in times.items():
        out[name + "_s"] = {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4), "n": len(ts)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
