#!/usr/bin/env python
"""Wall time of targetDriver for many cohorts: cohort_batch.run_target_cohorts (one pass) beside C calls of
transfer_tools.run_target_model, on synthetic inputs of a panel study's size -- C = 37 cohorts, `samples` samples and `mut-rows`
annotated rows per cohort, a 341-gene panel inside gene models of G = 20 091 genes.  A targeted file lists the panel's genes
(`inside` of its rows; the others carry other genes or none).  The two routes take turns (batch, serial, batch, ...) behind one
untimed pass of each; the median and the range of each go to one JSON line, with the card's name.

    python tools/target_cohorts_bench.py --workdir /tmp/dig_target --rounds 3
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

PANEL = "MSK_341"


def write_inputs(args):
    from digdriver_amd.io import mapfile
    os.makedirs(args.workdir, exist_ok=True)
    G, C = args.genes, args.cohorts
    genes = np.array(["GENE%05d" % i for i in range(G)], dtype=object)
    genes[G // 2] = "TP53"
    panel = genes[np.random.default_rng(args.seed).choice(G, args.panel_genes, replace=False)]
    with open(os.path.join(args.workdir, "genes_%s.txt" % PANEL), "w") as f:
        f.write("\n".join(panel) + "\n")
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
            mapfile.write_attrs(f, **{"N_MUT_" + PANEL: int(r.integers(5000, 50000)), "N_SAMPLE_" + PANEL: int(r.integers(500, 3000))})
        f = os.path.join(args.workdir, "cohort%02d.annot.txt" % c)
        muts.append(f)
        if not os.path.exists(f):
            n = args.mut_rows
            where = r.uniform(size=n)
            gene = np.where(where < args.inside, panel[r.integers(0, len(panel), n)], np.where(where < args.inside + 0.1, genes[r.integers(0, G, n)], "."))
            annot = np.where(gene != ".", annots[r.choice(6, n, p=[0.24, 0.55, 0.04, 0.02, 0.13, 0.02])], "Noncoding")
            indel = annot == "INDEL"
            pos = r.integers(1000, 50_000_000, n)
            pd.DataFrame({0: r.integers(1, 23, n), 1: pos, 2: pos + np.where(indel, 4, 1), 3: np.where(indel, "ACGT", "A"),
                          4: np.where(indel, "A", "T"), 5: np.char.add("S", r.integers(0, args.samples, n).astype(str)),
                          6: gene, 7: annot}).to_csv(f, sep="\t", header=False, index=False)
    return muts, maps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workdir", default="/tmp/dig_target")
    ap.add_argument("--cohorts", type=int, default=37)
    ap.add_argument("--genes", type=int, default=20_091)
    ap.add_argument("--panel-genes", type=int, default=341)
    ap.add_argument("--samples", type=int, default=3000)
    ap.add_argument("--mut-rows", type=int, default=25_000)
    ap.add_argument("--inside", type=float, default=0.8, help="share of the rows that carry a gene of the panel")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    args = ap.parse_args()
    import torch
    from digdriver_amd.driver_model import cohort_batch, transfer_tools
    muts, maps = write_inputs(args)
    transfer_tools.set_panel_dir(args.workdir)
    kw = dict(panel=PANEL, drop_synonymous=False)                    # (as `DigDriver.py targetDriver` calls it)

    def batch():
        return cohort_batch.run_target_cohorts(muts, maps, **kw)

    def serial():
        return [transfer_tools.run_target_model(m, g, **kw) for m, g in zip(muts, maps)]

    times = {"batch": [], "serial": []}
    with contextlib.redirect_stdout(io.StringIO()):
        a, b = batch(), serial()                                     # untimed: code objects, file cache
        same = all(x.equals(y) for x, y in zip(a, b))
        for _ in range(args.rounds):
            for name, fn in (("batch", batch), ("serial", serial)):
                t0 = time.perf_counter()
                fn()
                times[name].append(time.perf_counter() - t0)
    out = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "cohorts": args.cohorts, "genes": args.genes, "panel_genes": args.panel_genes,
           "samples": args.samples, "mut_rows": args.mut_rows, "frames_equal": bool(same)}
    for name, ts in times.items():
        out[name + "_s"] = {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4), "n": len(ts)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
