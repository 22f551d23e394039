"""Generator of tests/golden/si_count_golden.json: the reference's window context counts of genes.

Run in the build container only (it needs the reference checkout, DIG_REFERENCE or /root/reference), with
PYTHONDONTWRITEBYTECODE=1:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_si_count_golden.py

For every gene of a small synthetic genome it does what the reference's si_count_pretrain does per gene
(sequence_tools.py:386-391) with the reference's own functions -- genic_driver_tools.get_ideal_overlaps, trip_to_str and
sequence_tools.si_by_regions -- on a pysam.FastaFile look-alike over in-memory text (fetch truncates at the contig end, as pysam
does).  The container reads of si_count_pretrain (h5py) are the only lines not executed.  Recorded: the sequences, the genes,
the window, the sorted substitution keys and the [G, 192] counts.  Data only; nothing of the reference is copied.
"""
import json
import os
import sys
import types

import numpy as np

REF = os.environ.get("DIG_REFERENCE", "/root/reference")
for _name in ["pysam", "pybedtools", "h5py", "statsmodels", "statsmodels.stats", "statsmodels.stats.multitest", "seaborn", "bbi",
              "tables", "pkg_resources"]:
    if _name not in sys.modules:
        sys.modules[_name] = types.ModuleType(_name)
sys.path.insert(0, REF)

from DIGDriver.sequence_model import genic_driver_tools as ref_gdt  # noqa: E402
from DIGDriver.sequence_model import sequence_tools as ref_seq      # noqa: E402


class FakeFasta:
    def __init__(self, seqs):
        self._g = seqs

    def fetch(self, chrom, start, end):
        assert start >= 0
        return self._g[chrom][start:end]


def main():
    rng = np.random.default_rng(1907)
    window = 500
    seqs = {}
    for name, n in (("chr1", 2317), ("chr2", 1049), ("chrX", 777)):
        s = rng.choice(np.array(list("ACGT")), n)
        seqs[name] = s
    seqs["chr1"][640:702] = "N"                 # a run of N inside a window
    seqs["chr1"][1499:1502] = "N"               # ... and across a window edge
    seqs["chr2"][0:7] = "N"                     # a contig that starts with N
    seqs["chr2"][1040:1049] = "N"
    seqs["chr1"][[30, 2000]] = [c.lower() for c in seqs["chr1"][[30, 2000]]]        # soft-masked letters
    seqs = {k: "".join(v) for k, v in seqs.items()}
    # (name, chrom, strand, 1-based closed CDS blocks)
    genes = [
        ("first_window", "1", "+", [(4, 30), (90, 122)]),                            # START == 0 of the fetch
        ("over_edges", "1", "-", [(480, 500), (620, 700), (1490, 1510)]),            # blocks that end on / span a window edge
        ("same_windows", "1", "+", [(510, 530), (560, 580)]),                        # two blocks, one window: counted once
        ("last_window_1", "1", "-1", [(2200, 2250), (2290, 2316)]),                  # the window 2000-2500 is cut off at 2317
        ("last_window_2", "2", "1", [(960, 1049)]),                                   # 1000-1500 cut off at 1049, N at the end
        ("n_start", "2", "-", [(1, 99)]),
        ("on_x", "X", "-", [(100, 300), (480, 560)]),
        ("on_x_plus", "X", "+", [(700, 777)]),
    ]
    trans_idx = np.array(ref_seq.mk_trans_idx(n_up=1, n_down=1, collapse=False))
    fasta = FakeFasta(seqs)
    keys = sorted(trans_idx.tolist())
    counts = []
    for name, chrom, strand, blocks in genes:
        intervals = np.array([[b[0] for b in blocks], [b[1] for b in blocks]])
        strd = {"+": 1, "1": 1, "-": -1, "-1": -1}[strand]
        regions = [ref_gdt.trip_to_str(r) for r in ref_gdt.get_ideal_overlaps(chrom, intervals, window)]
        s_i = ref_seq.si_by_regions(fasta, trans_idx, regions, strand=strd)
        counts.append([int(v) for v in s_i.sort_index()[0].loc[keys].values])
    out = dict(window=window, seqs=seqs, genes=[dict(name=n, chrom=c, strand=s, blocks=b) for n, c, s, b in genes], keys=keys,
               counts=counts)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "si_count_golden.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, "genes", len(genes), "total", int(np.sum(counts)))


if __name__ == "__main__":
    main()
