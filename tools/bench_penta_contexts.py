"""Penta-nucleotide genome context counting at hg19 scale (bench.py is not involved).

  python tools/bench_penta_contexts.py [--genome-mb 3100] [--window 10000] [--fasta hg19.fa] [--reps 10]

Prints one JSON line:
  penta_ms      dig_count_contexts5 on the 10-kb windows of a resident 2-bit genome of `genome-mb` Mb (a real FASTA when --fasta
                is given, else a synthetic one with hg19's chromosome lengths scaled, an N run per Mb and a 3-Mb N run per
                chromosome as a centromere stand-in), device events, median of `reps` after 3 warm-ups;
  tri_ms        dig_count_contexts2 (64 contexts) on the same windows, same timing, for comparison;
  penta_centres_per_ns, out_gb  the centres counted per ns and the bytes of the [R, 1024] int32 output.
For the kernel time alone run it under `rocprofv3 --kernel-trace --stats`: context_count5_kernel / context_count2_kernel.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from digdriver_amd import _lib                                 # noqa: E402
from digdriver_amd.data_tools.genome import PackedGenome       # noqa: E402

HG19 = [249250621, 243199373, 198022430, 191154276, 180915260, 171115067, 159138663, 146364022, 141213431, 135534747, 135006516,
        133851895, 115169878, 107349540, 102531392, 90354753, 81195210, 78077248, 59128983, 63025520, 48129895, 51304566]


def synthetic_seqs(total_mb, rng, centromere=True):
    """hg19's chromosome lengths scaled to total_mb Mb: random ACGT, an N run per Mb and (centromere) a 3-Mb N run per chromosome."""
    scale = total_mb * 1e6 / sum(HG19)
    seqs = {}
    for i, n in enumerate(HG19):
        n = max(int(n * scale), 20000)
        s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n, dtype=np.uint8)].copy()
        for a in rng.integers(0, n - 5000, max(n // 1000000, 1)):
            s[a:a + int(rng.integers(100, 5000))] = ord("N")
        if centromere:
            c = n // 3
            s[c:c + min(3000000, n // 10)] = ord("N")
        seqs["chr%d" % (i + 1)] = s.tobytes()
    return seqs


def time_entry(name, g, ci, st, en, mi, K, reps):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: torch.as_tensor(a, device=dev)
    genome = g.genome2_args(dev)
    rc, rs, re_, rm = t(ci), t(st), t(en), t(mi)
    R = len(ci)
    out = torch.empty((R, K), dtype=torch.int32, device=dev)
    p = _lib.dev_ptr

    def launch():
        _lib.call(name, *genome, p(rc), p(rs), p(re_), p(rm), R, p(out), _lib.stream_ptr())

    times = []
    for i in range(3 + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            times.append(e0.elapsed_time(e1))
    return float(np.median(times)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=3100)
    ap.add_argument("--window", type=int, default=10000)
    ap.add_argument("--fasta", default="")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    _lib.require_device()
    import torch
    rng = np.random.default_rng(0)
    t0 = time.perf_counter()
    g = PackedGenome.from_fasta(a.fasta) if a.fasta else PackedGenome.from_sequences(synthetic_seqs(a.genome_mb, rng))
    g.two_bit()
    res = dict(genome=a.fasta or "synthetic", genome_bases=int(g.lengths.sum()), pack_s=round(time.perf_counter() - t0, 1))
    ci, st, en = [], [], []
    for c, L in enumerate(g.lengths):
        s = np.arange(0, int(L), a.window, dtype=np.int64)
        ci.append(np.full(len(s), c, np.int32))
        st.append(s)
        en.append(s + a.window)
    ci, st, en = np.concatenate(ci), np.concatenate(st), np.concatenate(en)
    mi = np.zeros(len(ci), np.uint8)
    R = len(ci)
    res.update(regions=R, window=a.window)
    res["penta_ms"], out5 = time_entry("dig_count_contexts5", g, ci, st, en, mi, 1024, a.reps)
    centres = int(out5.sum(dtype=torch.int64).item())
    del out5
    res["tri_ms"], out2 = time_entry("dig_count_contexts2", g, ci, st, en, mi, 64, a.reps)
    del out2
    res.update(penta_ms=round(res["penta_ms"], 3), tri_ms=round(res["tri_ms"], 3), counted_centres=centres,
               penta_centres_per_ns=round(centres / (res["penta_ms"] * 1e6), 2), out_gb=round(R * 1024 * 4 / 1e9, 3))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
