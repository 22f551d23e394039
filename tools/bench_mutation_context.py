"""addMutationContext at PCAWG scale (about 25 M rows; bench.py is not involved).

  python tools/bench_mutation_context.py [--rows 25000000] [--genome-mb 3100] [--cli-genome-mb 300] [--fasta hg19.fa]

Prints one JSON line:
  kernel_ms        dig_mutation_contexts (both launches) on `rows` chromosome-grouped rows over a resident 2-bit genome of
                   `genome-mb` Mb (a real FASTA when --fasta is given, else a synthetic one with an N run per Mb), device events,
                   median of 10 after 3 warm-ups;
  cli_*_s          write_mutation_contexts (the command line's native path, `_host` twin) on a file of `rows` rows over a
                   synthetic FASTA of `cli-genome-mb` Mb: parse / kernel (incl. staging and host-resolved rows) / write seconds;
  ref_rows_per_s   the reference's per-row loop (sequence_tools.py:130-177, restated: seq[START] test, run copy, window slice,
                   'N' test) on one CPU core over 1 M rows of a 50 Mb chromosome string.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_penta_contexts import synthetic_seqs                # noqa: E402
from digdriver_amd import engine                               # noqa: E402
from digdriver_amd.data_tools.genome import PackedGenome       # noqa: E402
from digdriver_amd.sequence_model import sequence_tools as st  # noqa: E402

def make_rows(g, n_rows, rng):
    lengths = g.lengths[[g.index["chr%d" % c] for c in range(1, 23)]]
    chrom = np.sort(rng.choice(np.arange(1, 23), n_rows, p=lengths / lengths.sum())).astype(np.int32)
    start = (rng.random(n_rows) * lengths[chrom - 1]).astype(np.int64)
    start = np.minimum(start, lengths[chrom - 1] - 1)
    return chrom, start


def time_kernel(g, chrom, start, ref):
    import torch
    dev = torch.device("cuda", 0)
    for _ in range(3):
        engine.mutation_contexts(g, chrom, start, ref, 1, 1)
    torch.cuda.synchronize()
    # the timed window: both launches only (the rows are already on the device)
    from digdriver_amd import _lib
    genome = g.genome2_args(dev)
    ci = torch.as_tensor(g.chrom_index(list(range(1, 23)))[chrom - 1], device=dev)
    s_d, r_d = torch.as_tensor(start, device=dev), torch.as_tensor(ref, device=dev)
    R = len(chrom)
    status = torch.empty(R, dtype=torch.uint8, device=dev)
    ctx = torch.empty(R, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.load().dig_mutation_contexts_workspace(R), dtype=torch.uint8, device=dev)
    p = _lib.dev_ptr
    times = []
    for _ in range(13):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.call("dig_mutation_contexts", *genome, p(ci), p(s_d), p(r_d), R, 1, 1, 0, p(status), p(ctx), p(ws), ws.numel(),
                  _lib.stream_ptr())
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times[3:]))


def ref_loop_rate(rng, n_rows=1000000):
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 50000000, dtype=np.uint8)].tobytes().decode()
    starts = np.sort(rng.integers(2, len(seq) - 2, n_rows)).tolist()
    refs = [seq[s] for s in starts]
    t0 = time.perf_counter()
    out, prev_start, prev = [], -1, ""
    for s, r in zip(starts, refs):
        if seq[s] != r:
            sub = ""
        elif s == prev_start:
            sub = prev
        else:
            sub = seq[s - 1:s + 2]
            sub = "" if "N" in sub else sub
        out.append(sub)
        prev_start, prev = s, sub
    return n_rows / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=25000000)
    ap.add_argument("--genome-mb", type=float, default=3100)
    ap.add_argument("--cli-genome-mb", type=float, default=300)
    ap.add_argument("--fasta", default="")
    ap.add_argument("--skip-cli", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    res = dict(rows=a.rows)
    t0 = time.perf_counter()
    g = PackedGenome.from_fasta(a.fasta) if a.fasta else PackedGenome.from_sequences(synthetic_seqs(a.genome_mb, rng, centromere=False))
    g.two_bit()
    res.update(genome=a.fasta or "synthetic", genome_bases=int(g.lengths.sum()), pack_s=round(time.perf_counter() - t0, 1))
    chrom, start = make_rows(g, a.rows, rng)
    ref = rng.integers(0, 4, a.rows, dtype=np.uint8)
    res["kernel_ms"] = round(time_kernel(g, chrom, start, ref), 3)
    res["kernel_rows_per_us"] = round(a.rows / (res["kernel_ms"] * 1e3), 1)
    del g
    if not a.skip_cli:
        with tempfile.TemporaryDirectory() as tmp:
            seqs = synthetic_seqs(a.cli_genome_mb, rng, centromere=False)
            fa = os.path.join(tmp, "g.fa")
            with open(fa, "wb") as f:
                for n, s in seqs.items():
                    f.write(b">" + n.encode() + b"\n" + s + b"\n")
            g2 = st.load_genome(fa)
            chrom, start = make_rows(g2, a.rows, rng)
            order = rng.permutation(a.rows)
            letters = np.array(list("ACGT"))
            ref = np.array([chr(x) for x in b"ACGT"])[rng.integers(0, 4, a.rows)]
            with open(os.path.join(tmp, "m.tsv"), "w") as f:
                for k in order:
                    f.write("%d\t%d\t%d\t%s\tT\tS%d\tG1\tMissense\n" % (chrom[k], start[k], start[k] + 1, ref[k], k % 2000))
            del seqs, letters
            tm = {}
            t0 = time.perf_counter()
            path = st.write_mutation_contexts(os.path.join(tmp, "m.tsv"), fa, os.path.join(tmp, "o.tsv"), on_device=False,
                                              timings=tm)
            res.update(cli_path=path, cli_genome_bases=int(g2.lengths.sum()), cli_total_s=round(time.perf_counter() - t0, 2),
                       **{"cli_%s_s" % k: round(v, 2) for k, v in tm.items()})
    res["ref_rows_per_s"] = round(ref_loop_rate(rng))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
