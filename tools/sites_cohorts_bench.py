#!/usr/bin/env python
"""Wall time of elementDriver --f-sites for many cohorts: one cohort_batch.run_sites_cohorts call beside C serial
transfer_tools.run_sites_region_model calls (each reads the sites file again and merges it with the cohort's file on nine string
columns), on synthetic inputs -- 1 M site rows (three substitutions at a third of a million positions, 20 000 elements), C = 37
cohorts x 300 000 rows in position order, a third of them at listed sites -- with the expected-synonymous scale factor on both sides.
The serial figure is the per-cohort route's own; --serial-cohorts times only the first few of its calls (the figure then says how
many).  The stages of the batched route are timed apart on the same inputs: parse and encode (host), upload, the three kernels
(device events around each library call), the cumulative sum and the key sort.  One JSON line.

    python tools/sites_cohorts_bench.py --rounds 1
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BASES = np.array(list("ACGT"), dtype=object)
KEY = "bench_sites"


def make_sites(rng, n_sites, n_elts):
    n_pos = n_sites // 3
    chrom = np.sort(rng.integers(1, 23, n_pos))
    start = rng.integers(0, 1 << 27, n_pos)
    order = np.lexsort((start, chrom))
    chrom, start = np.repeat(chrom[order], 3), np.repeat(start[order], 3)
    ref = np.repeat(rng.integers(0, 4, n_pos), 3)
    alt = (ref + np.tile(np.arange(1, 4), n_pos)) % 4
    left, right = np.repeat(rng.integers(0, 4, n_pos), 3), np.repeat(rng.integers(0, 4, n_pos), 3)
    elt = (np.arange(3 * n_pos) * n_elts) // (3 * n_pos)
    return pd.DataFrame(dict(CHROM=chrom, START=start, END=start + 1, REF=BASES[ref], ALT=BASES[alt],
                             ELT=np.char.add("E", np.char.zfill(elt.astype(str), 6)).astype(object),
                             GENE=np.char.add("G", (elt // 8).astype(str)).astype(object),
                             ANNOT=np.where(elt % 3 == 0, "Missense", "Noncoding").astype(object),
                             MUT_TYPE=BASES[ref] + ">" + BASES[alt], CONTEXT=BASES[left] + BASES[ref] + BASES[right]))


def make_cohort(rng, sites, n_rows, hit_share=1 / 3):
    n_hit = int(n_rows * hit_share)
    hit = sites.iloc[np.sort(rng.integers(0, len(sites), n_hit))].rename(columns={"ELT": "SAMPLE"})
    n = n_rows - n_hit
    ref = rng.integers(0, 4, n)
    alt = (ref + rng.integers(1, 4, n)) % 4
    start = rng.integers(0, 1 << 27, n)
    annot = np.where(rng.uniform(size=n) < 0.02, "Synonymous", "Noncoding").astype(object)
    miss = pd.DataFrame(dict(CHROM=rng.integers(1, 23, n), START=start, END=start + 1, REF=BASES[ref], ALT=BASES[alt], SAMPLE="",
                             GENE=np.where(annot == "Synonymous", "GSYN", ".").astype(object), ANNOT=annot,
                             MUT_TYPE=BASES[ref] + ">" + BASES[alt], CONTEXT=BASES[rng.integers(0, 4, n)] + BASES[ref] + BASES[rng.integers(0, 4, n)]))
    rows = pd.concat([hit, miss], ignore_index=True).sort_values(["CHROM", "START"], kind="stable")
    rows["SAMPLE"] = np.char.add("S", rng.integers(0, 400, len(rows)).astype(str)).astype(object)
    return rows


def write_maps(tmp, rng, elts, C):
    from digdriver_amd.io import mapfile
    genes = ["G%d" % i for i in range(2000)] + ["TP53"]
    G, E = len(genes), len(elts)
    paths = []
    for c in range(C):
        mu = rng.uniform(0.05, 2.0, E)
        paths.append(os.path.join(tmp, "map%02d.map" % c))
        mapfile.write_frame(paths[-1], KEY, pd.DataFrame(dict(ELT=elts, R_OBS=rng.integers(0, 50, E), MU=mu, SIGMA=mu * rng.uniform(0.2, 0.6, E),
                                                              P_SUM=rng.uniform(1e-3, 0.3, E))))
        gmu = rng.uniform(20, 200, G)
        p = rng.uniform(1e-3, 3e-3, (G, 4))
        mapfile.write_frame(paths[-1], "genic_model", pd.DataFrame(dict(
            CHROM=[str(1 + i % 22) for i in range(G)], GENE=genes, GENE_LENGTH=rng.integers(600, 6000, G), R_SIZE=rng.integers(20000, 40000, G),
            R_OBS=rng.integers(50, 400, G), R_INDEL=rng.integers(5, 40, G), MU=gmu, SIGMA=gmu * 0.3, MU_INDEL=gmu * 0.1, SIGMA_INDEL=gmu * 0.04,
            FLAG=np.zeros(G, np.int64), P_MIS=p[:, 0], P_NONS=p[:, 1] * 0.1, P_SILENT=p[:, 2] * 0.4, P_SPLICE=p[:, 3] * 0.05,
            P_TRUNC=p[:, 1] * 0.1 + p[:, 3] * 0.05, P_INDEL=rng.uniform(0.02, 0.2, G))))
    return paths


def stage_times(f_sites, f_muts):
    """The batched route's counting, stage by stage, on the same files: seconds on the host, milliseconds on the device."""
    import torch
    from digdriver_amd import _lib
    from digdriver_amd.data_tools import cohort_rows, sites
    out = {}
    t0 = time.perf_counter()
    table = sites.encode_sites_file(f_sites)
    rows = [sites.encode_site_rows(f, table["dicts"], c) for c, f in enumerate(f_muts)]
    out["parse_encode_s"] = round(time.perf_counter() - t0, 3)
    C, E, S = len(f_muts), len(table["elt_names"]), len(table["site_pos"])
    off = cohort_rows.sample_offsets(rows)
    host = [table[k] for k in ("site_pos", "site_end", "site_attr", "site_elt")] + [cohort_rows.column(rows, k) for k in ("pos", "end", "attr")] + \
        [cohort_rows.column(rows, "sample", "i32", off), cohort_rows.column(rows, "cohort"), off]
    n = len(host[4])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dev = cohort_rows.place(host, True, "cuda")
    torch.cuda.synchronize()
    out["upload_s"] = round(time.perf_counter() - t0, 4)
    d, stream = _lib.dev_ptr, _lib.stream_ptr()
    search = [d(x) for x in dev[:4]] + [S, E] + [d(x) for x in dev[4:10]] + [n, C, int(off[-1])]

    def timed(name, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn()
        b.record()
        b.synchronize()
        out[name] = round(a.elapsed_time(b), 4)
        return res

    for rep in range(2):                                                # (the first pass loads the code objects; the second is kept)
        counts = torch.empty(n, dtype=torch.int32, device="cuda")
        timed("match_count_ms", lambda: _lib.call("dig_site_match_count", *search, d(counts), stream))
        incl = timed("cumsum_ms", lambda: torch.cumsum(counts, 0, dtype=torch.int64))
        total, offsets = int(incl[-1]), incl - counts
        keys = torch.empty(total, dtype=torch.int64, device="cuda")
        timed("match_keys_ms", lambda: _lib.call("dig_site_match_keys", *search, d(offsets), total, d(keys), stream))
        keys = timed("sort_ms", lambda: keys.sort()[0])
        obs = [torch.empty((E, C), dtype=torch.int32, device="cuda") for _ in range(2)]
        timed("site_counts_ms", lambda: _lib.call("dig_site_counts", d(keys), total, E, C, int(off[-1]), d(obs[0]), d(obs[1]), stream))
    out.update(rows=n, sites=S, elements=E, matches=total)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cohorts", type=int, default=37)
    ap.add_argument("--mut-rows", type=int, default=300_000)
    ap.add_argument("--sites", type=int, default=1_000_000)
    ap.add_argument("--elements", type=int, default=20_000)
    ap.add_argument("--serial-cohorts", type=int, default=None, help="time only the first few serial calls (default: all)")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--seed", type=int, default=11)
    args = ap.parse_args()
    import torch
    from digdriver_amd import _lib
    from digdriver_amd.driver_model import cohort_batch
    from digdriver_amd.driver_model import transfer_tools as tt
    _lib.require_device()
    assert torch.cuda.is_available()
    C = args.cohorts
    n_serial = C if args.serial_cohorts is None else min(C, args.serial_cohorts)
    rng = np.random.default_rng(args.seed)
    with tempfile.TemporaryDirectory() as tmp:
        sites_frame = make_sites(rng, args.sites, args.elements)
        f_sites = os.path.join(tmp, "sites.txt")
        sites_frame.to_csv(f_sites, sep="\t", header=False, index=False)
        f_muts = []
        for c in range(C):
            f_muts.append(os.path.join(tmp, "cohort%02d.annot.txt" % c))
            make_cohort(np.random.default_rng([args.seed, c]), sites_frame, args.mut_rows).to_csv(f_muts[-1], sep="\t", header=False, index=False)
        maps = write_maps(tmp, rng, sorted(set(sites_frame.ELT)), C)
        del sites_frame

        def batched():
            t0 = time.perf_counter()
            frames = cohort_batch.run_sites_cohorts(f_muts, f_sites, maps, KEY)
            return time.perf_counter() - t0, frames

        def serial():
            t0 = time.perf_counter()
            frames = [tt.run_sites_region_model(f_muts[c], f_sites, maps[c], KEY) for c in range(n_serial)]
            return time.perf_counter() - t0, frames

        stages = stage_times(f_sites, f_muts)                           # (also the untimed first pass of the kernels)
        times = {"batched": [], "serial": []}
        for _ in range(args.rounds):
            tb, fb = batched()
            ts, fs = serial()
            times["batched"].append(tb)
            times["serial"].append(ts)
        same = all(fb[c].equals(fs[c]) for c in range(n_serial))
    out = {"cohorts": C, "serial_cohorts_timed": n_serial, "frames_equal": bool(same), "obs_snv_sum": int(sum(f.OBS_SNV.sum() for f in fb)),
           "stages": stages}
    for name, ts in times.items():
        out[name + "_s"] = {"median": round(float(np.median(ts)), 3), "min": round(min(ts), 3), "max": round(max(ts), 3), "n": len(ts)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
