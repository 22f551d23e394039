"""The per-gene site-count kernel at genome scale against the route that existed before it (bench.py is not involved).

  python tools/bench_gene_site_counts.py [--genome-mb 3100] [--genes 20000] [--reps 20]

Prints one JSON line.  A synthetic genome of `genome-mb` Mb (hg19's chromosome lengths scaled, N runs as in
tools/bench_penta_contexts.py) is kept resident in its 2-bit form; `genes` synthetic genes as in tools/bench_mutation_function.py.
  site_counts_ms     dig_gene_site_counts on all genes, device events, median of `reps` launches after 3 warm-ups;
  enumeration_ms     the yardstick: dig_mutation_function + dig_mutation_contexts over the full enumeration of possible SNVs of the
                     same genes -- 3 x (CDS bases + splice positions) pairs, built once outside the timed region -- same timing
                     (each kernel alone in mutfunc_ms / mutctx_ms); the tally of their outputs into [G, 4, 192] is not timed;
  pairs, cds_bases, host_genes (genes the kernel leaves to the host), ratio = enumeration_ms / site_counts_ms.
For the kernel time alone run it under `rocprofv3 --kernel-trace --stats`: gene_site_counts_kernel.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_mutation_function import synthetic_genes, timed        # noqa: E402
from bench_penta_contexts import synthetic_seqs                   # noqa: E402
from digdriver_amd import _lib, engine                            # noqa: E402
from digdriver_amd._marshal import device_backend                # noqa: E402
from digdriver_amd.data_tools.genome import PackedGenome          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=3100)
    ap.add_argument("--genes", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    _lib.require_device()
    import torch
    rng = np.random.default_rng(0)
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    g = PackedGenome.from_sequences(synthetic_seqs(a.genome_mb, rng))
    g.two_bit()
    res = dict(genome_bases=int(g.lengths.sum()), pack_s=round(time.perf_counter() - t0, 1))
    print("packed the genome", res, file=sys.stderr, flush=True)
    genes, gch = synthetic_genes(g, a.genes, rng).on_genome(g)
    G = len(genes)
    t = lambda x: torch.as_tensor(x, device=dev)
    p = _lib.dev_ptr
    genome = g.genome2_args(dev)
    tab, _ = engine.gene_table(device_backend(dev), g, genes, gch)
    L = torch.empty((G, 4, 192), dtype=torch.int32, device=dev)
    nsl, status = torch.empty(G, dtype=torch.int32, device=dev), torch.empty(G, dtype=torch.uint8, device=dev)

    def site_counts():
        _lib.call("dig_gene_site_counts", *genome, *[p(x) for x in tab], G, p(L), p(nsl), p(status), _lib.stream_ptr())

    res.update(genes=G, cds_bases=int(genes.cds_len.sum()), splice_positions=int(len(genes.spl_pos)))
    res["site_counts_ms"] = timed(site_counts, a.reps)
    res["host_genes"] = int((status.cpu().numpy() == engine.GS_HOST).sum())
    print("site counts", res["site_counts_ms"], file=sys.stderr, flush=True)

    # the enumeration: every CDS base and splice position of every gene with its three alternates, chromosome-grouped
    size = genes.blk_end - genes.blk_start + 1
    blk_gene = np.repeat(np.arange(G), np.diff(genes.blk_ptr))
    first = np.cumsum(size) - size
    cds_pos = np.repeat(genes.blk_start - first, size) + np.arange(int(size.sum()), dtype=np.int64)
    pos = np.concatenate([cds_pos, genes.spl_pos])
    gene = np.concatenate([np.repeat(blk_gene, size), np.repeat(np.arange(G), np.diff(genes.spl_ptr))])
    order = np.lexsort((pos, gch[gene]))
    pos, gene = pos[order], gene[order]
    at = g.PAD2_BASES + g.offsets[gch[gene]] + pos - 1                # array base of the 2-bit form (a letter other than ACGT reads as A)
    ref1 = ((g.two_bit()[0][at >> 4] >> (2 * (at & 15)).astype(np.uint32)) & np.uint32(3)).astype(np.uint8)
    pg = t(np.repeat(gene, 3).astype(np.int32))
    ps = t(np.repeat(pos, 3))
    ref = t(np.repeat(ref1, 3))
    alt = t(((np.repeat(ref1, 3) + np.tile(np.arange(1, 4, dtype=np.uint8), len(pos))) & 3).astype(np.uint8))
    n = int(pg.numel())
    kind = torch.zeros(n, dtype=torch.uint8, device=dev)
    impact, mstatus = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    n_cds, cmin, cmax = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    rch, rst = t(np.repeat(gch[gene], 3).astype(np.int32)), t(np.repeat(pos - 1, 3))
    cstatus, context = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    ws = torch.empty(max(_lib.load().dig_mutation_contexts_workspace(n), 1), dtype=torch.uint8, device=dev)

    def mutfunc():
        _lib.call("dig_mutation_function", *genome, *[p(x) for x in tab], G, p(pg), p(ps), p(ps), p(kind), p(ref), p(alt), n, p(impact),
                  p(mstatus), p(n_cds), p(cmin), p(cmax), _lib.stream_ptr())

    def mutctx():
        _lib.call("dig_mutation_contexts", *genome, p(rch), p(rst), p(ref), n, 1, 1, 0, p(cstatus), p(context), p(ws), ws.numel(),
                  _lib.stream_ptr())

    def both():
        mutfunc()
        mutctx()

    res["pairs"] = n
    res["mutfunc_ms"], res["mutctx_ms"], res["enumeration_ms"] = timed(mutfunc, a.reps), timed(mutctx, a.reps), timed(both, a.reps)
    res["ratio"] = round(res["enumeration_ms"] / res["site_counts_ms"], 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
