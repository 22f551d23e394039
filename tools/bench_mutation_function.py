"""The genic-function kernel at cohort scale (bench.py is not involved).

  python tools/bench_mutation_function.py [--genome-mb 3100] [--genes 20000] [--sizes 1,5,20] [--reps 20]

Prints one JSON line.  A synthetic genome of `genome-mb` Mb (hg19's chromosome lengths scaled, N runs as in
tools/bench_penta_contexts.py) is kept resident in its 2-bit form; `genes` synthetic genes (1-20 exons of 60-300 bases on both
strands) give the gene table; for each size (millions of rows) as many synthetic SNVs are drawn uniformly from the CDS bases.
  mutfunc_ms[size]   dig_mutation_function on the rows as (mutation, gene) pairs, device events, median of `reps` launches after
                     3 warm-ups;
  join_ms[size]      dig_overlap_join_count + dig_overlap_join_fill of the same rows against the gene ranges (CDS blocks and
                     splice positions), same timing, for scale;
  pairs[size], ranges, status counts of the largest size.
For the kernel time alone run it under `rocprofv3 --kernel-trace --stats`: mutation_function_kernel / overlap_kernel.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_penta_contexts import synthetic_seqs                 # noqa: E402
from digdriver_amd import _lib, engine                          # noqa: E402
from digdriver_amd._marshal import device_backend              # noqa: E402
from digdriver_amd.data_tools import gene_annotation            # noqa: E402
from digdriver_amd.data_tools.genome import PackedGenome        # noqa: E402


def synthetic_genes(g, n_genes, rng):
    names, chrom, minus, blk_ptr, bs, be, spl_ptr, sp = [], [], [], [0], [], [], [0], []
    share = g.lengths / g.lengths.sum()
    for i in range(n_genes):
        c = int(rng.choice(len(g.names), p=share))
        k = int(rng.integers(1, 21))
        sizes = rng.integers(60, 300, k)
        sizes[-1] += (3 - int(sizes.sum()) % 3) % 3
        gaps = rng.integers(80, 5000, k - 1)
        rel = np.concatenate([[0], np.cumsum(sizes[:-1] + gaps)])
        s0 = int(rng.integers(1000, int(g.lengths[c]) - int(rel[-1] + sizes[-1]) - 1000))
        s, e = (s0 + rel + 1).tolist(), (s0 + rel + sizes).tolist()
        mi = int(rng.integers(0, 2))
        names.append("g%d" % i), chrom.append(g.names[c]), minus.append(mi)
        bs += s
        be += e
        blk_ptr.append(len(bs))
        sp += gene_annotation.splice_positions(s, e, mi)
        spl_ptr.append(len(sp))
    return gene_annotation.GeneSet(names, chrom, minus, blk_ptr, bs, be, spl_ptr, sp)


def timed(launch, reps):
    import torch
    times = []
    for i in range(3 + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            times.append(e0.elapsed_time(e1))
    return round(float(np.median(times)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=3100)
    ap.add_argument("--genes", type=int, default=20000)
    ap.add_argument("--sizes", default="1,5,20", help="millions of SNVs, comma separated")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    _lib.require_device()
    import torch
    from digdriver_amd.data_tools import tabulate_gpu
    rng = np.random.default_rng(0)
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    g = PackedGenome.from_sequences(synthetic_seqs(a.genome_mb, rng))
    g.two_bit()
    res = dict(genome_bases=int(g.lengths.sum()), pack_s=round(time.perf_counter() - t0, 1))
    print("packed the genome", res, file=sys.stderr, flush=True)
    genes, gch = synthetic_genes(g, a.genes, rng).on_genome(g)
    t = lambda x: torch.as_tensor(x, device=dev)
    p = _lib.dev_ptr
    genome = g.genome2_args(dev)
    tab, _ = engine.gene_table(device_backend(dev), g, genes, gch)
    r_chrom, r_start, r_end, r_gene = genes.ranges()
    blocks = tabulate_gpu.ElementBlocks(g.chrom_index(r_chrom).astype(np.int64) + 1, r_start - 1, r_end, np.arange(len(r_start)), len(r_start), dev)
    size = genes.blk_end - genes.blk_start + 1
    cum = np.concatenate([[0], np.cumsum(size)])
    blk_gene = np.repeat(np.arange(len(genes)), np.diff(genes.blk_ptr))
    res.update(genes=len(genes), blocks=len(size), ranges=len(r_start), mutfunc_ms={}, join_ms={}, pairs={})
    for millions in [float(x) for x in a.sizes.split(",")]:
        n = int(millions * 1e6)
        r = rng.integers(0, cum[-1], n)
        b = np.searchsorted(cum, r, side="right") - 1
        pos = genes.blk_start[b] + (r - cum[b])
        pg, ps = t(blk_gene[b].astype(np.int32)), t(pos)
        kind, ref, alt = torch.zeros(n, dtype=torch.uint8, device=dev), t(rng.integers(0, 4, n).astype(np.uint8)), t(rng.integers(0, 4, n).astype(np.uint8))
        impact, status = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
        n_cds, cmin, cmax = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))

        def launch():
            _lib.call("dig_mutation_function", *genome, *[p(x) for x in tab], len(genes), p(pg), p(ps), p(ps), p(kind), p(ref), p(alt), n, p(impact), p(status), p(n_cds),
                      p(cmin), p(cmax), _lib.stream_ptr())

        key = "%gM" % millions
        res["mutfunc_ms"][key] = timed(launch, a.reps)
        # the join on the same rows: the mutation as the half-open [pos - 1, pos) against the ranges
        mc, ms, me = t(gch[blk_gene[b]].astype(np.int64) + 1), t(pos - 1), t(pos)
        counts = torch.zeros(n, dtype=torch.int32, device=dev)
        jargs = [p(blocks.start_key), p(blocks.runmax_key), p(blocks.end), blocks.n_blocks, p(mc), p(ms), p(me), n]
        _lib.call("dig_overlap_join_count", *jargs, p(counts), _lib.stream_ptr())
        incl = torch.cumsum(counts, 0, dtype=torch.int64)
        total = int(incl[-1].item())
        offsets = (incl - counts).contiguous()
        pm, pb = torch.empty(total, dtype=torch.int32, device=dev), torch.empty(total, dtype=torch.int32, device=dev)

        def join():
            _lib.call("dig_overlap_join_count", *jargs, p(counts), _lib.stream_ptr())
            _lib.call("dig_overlap_join_fill", *jargs, p(offsets), p(pm), p(pb), _lib.stream_ptr())

        res["join_ms"][key] = timed(join, a.reps)
        res["pairs"][key] = total
        res["status_counts"] = np.bincount(status.cpu().numpy(), minlength=4).tolist()
        print(key, res["mutfunc_ms"][key], res["join_ms"][key], file=sys.stderr, flush=True)
        del pg, ps, kind, ref, alt, impact, status, n_cds, cmin, cmax, mc, ms, me, counts, incl, offsets, pm, pb
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
