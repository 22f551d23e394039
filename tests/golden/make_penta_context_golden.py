"""Generate the penta-nucleotide context-count golden fixture by running the REAL reference here.

Run in the build container only (it needs the reference tree, DIG_REFERENCE, default /root/reference):

    python tests/golden/make_penta_context_golden.py

* Stubs the reference's absent I/O-only dependencies as make_golden.py does; pysam.FastaFile is replaced by a stand-in whose
  fetch(chrom, start, end) behaves as pysam's: a negative start raises ValueError, the end is truncated at the chromosome end.
* Builds a small seeded genome (three chromosomes with N runs -- at the chromosome ends, long ones, and short ones fewer than
  four bases apart -- and soft-masked stretches; no IUPAC letters, on which the reference raises KeyError).
* Runs the reference's count_contexts_by_regions (n_up = n_down = 2, collapse False and True) on windows from START 0,
  random regions, empty regions, regions past the chromosome end and whole chromosomes; nonc_elt_context_count with
  mk_trans_idx(2, 2) on regions of mixed strands; train_sequence_model(n_up=2, n_down=2) with the identity whitelist of
  make_golden.py on mutations annotated by the reference's add_context_to_mutations and genome counts from the first call.
* Stores the inputs and the frames (index, columns, values) -- data only -- in penta_context_golden.json.gz.
"""
import gzip
import json
import os
import sys
import tempfile
import types

import numpy as np
import pandas as pd

REF = os.environ.get("DIG_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "penta_context_golden.json.gz")


def _read_fasta(path):
    seqs, name, parts = {}, None, []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith(">"):
                if name is not None:
                    seqs[name] = "".join(parts)
                name, parts = line[1:].split()[0], []
            elif line:
                parts.append(line)
    if name is not None:
        seqs[name] = "".join(parts)
    return seqs


class _Fasta:
    """pysam.FastaFile stand-in: fetch(chrom[, start, end]) with pysam's bounds behaviour."""
    def __init__(self, path):
        self._seqs = _read_fasta(path)

    def fetch(self, chrom, start=None, end=None):
        s = self._seqs[chrom]
        start = 0 if start is None else int(start)
        end = len(s) if end is None else int(end)
        if start < 0:
            raise ValueError("start out of range (%d)" % start)
        return s[start:end]


def install_stubs():
    for name in ["pysam", "pybedtools", "h5py", "statsmodels", "statsmodels.stats", "statsmodels.stats.multitest", "seaborn",
                 "bbi", "tables", "gpytorch", "tensorboardX", "pkg_resources"]:
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["pysam"].FastaFile = _Fasta
    sys.path.insert(0, REF)


def make_genome(rng):
    seqs = {}
    for name, n in (("chr1", 9000), ("chr2", 7000), ("chr3", 5000)):
        s = rng.choice(list("ACGT"), n)
        for _ in range(6):                                        # N runs of 1 to 40 bases
            a = int(rng.integers(0, n - 50))
            s[a:a + int(rng.integers(1, 40))] = "N"
        for _ in range(4):                                        # runs fewer than four bases apart
            a = int(rng.integers(0, n - 20))
            g = int(rng.integers(1, 4))
            s[a:a + int(rng.integers(1, 4))] = "N"
            s[a + 4 + g:a + 4 + g + int(rng.integers(1, 4))] = "N"
        if name == "chr2":
            s[1500:2700] = "N"                                    # a run longer than a window
        if name == "chr3":
            s[:5] = "N"
            s[-4:] = "N"
        s = "".join(s)
        for _ in range(8):                                        # soft-masked stretches
            a = int(rng.integers(0, n - 300))
            b = a + int(rng.integers(10, 300))
            s = s[:a] + s[a:b].lower() + s[b:]
        seqs[name] = s
    return seqs


def make_regions(rng, seqs):
    chroms, starts, ends = [], [], []

    def add(c, s, e):
        chroms.append(c)
        starts.append(int(s))
        ends.append(int(e))

    for c, s in seqs.items():
        L = len(s)
        for a in range(0, L, 1000):                               # windows from START 0, the last one past the end
            add(c, a, a + 1000)
        add(c, 0, L)                                              # the whole chromosome
        for a, b in ((L - 5, L), (L - 2, L + 10), (L - 3, L - 1), (L + 5, L + 50), (2, 3), (3, 3), (0, 2), (0, 0)):
            add(c, a, b)
        for _ in range(10):                                       # random regions, empty ones among them
            a = int(rng.integers(2, L + 20))
            add(c, a, a + int(rng.integers(0, 600)))
    return chroms, starts, ends


def make_nonc_regions(rng, seqs):
    regions = []
    strands = ["+", "-", -1, 1, "."]
    for c, s in seqs.items():
        L = len(s)
        for _ in range(10):
            a = int(rng.choice([0, int(rng.integers(2, L))]))
            regions.append((c[3:], a, a + int(rng.integers(0, 900)), strands[int(rng.integers(0, len(strands)))]))
        regions.append((c[3:], 0, L, "-"))
        regions.append((c[3:], L - 10, L + 5, "-"))
    return regions


def make_mutations(rng, seqs, n):
    up = {k: v.upper() for k, v in seqs.items()}
    rows = []
    for _ in range(n):
        c = int(rng.integers(1, 4))
        s = up["chr%d" % c]
        pos = int(rng.integers(2, len(s) - 2))
        ref = s[pos]
        if ref not in "ACGT":
            continue
        alt = str(rng.choice([b for b in "ACGT" if b != ref]))
        rows.append([str(c), pos, pos + 1, ref, alt, "S%d" % rng.integers(0, 9), "G%d" % rng.integers(0, 5), "Noncoding"])
    return "".join("\t".join(str(x) for x in r) + "\n" for r in rows)


def frame(df):
    return dict(index=[str(i) for i in df.index], columns=[str(c) for c in df.columns], values=df.values.tolist(),
                dtypes=sorted(set(str(t) for t in df.dtypes)))


def main():
    install_stubs()
    from DIGDriver.data_tools import mutation_tools as ref_mt       # noqa: E402
    from DIGDriver.sequence_model import sequence_tools as ref_seq  # noqa: E402

    rng = np.random.default_rng(20261017)
    seqs = make_genome(rng)
    fasta = "".join(">%s\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))) for n, s in seqs.items())
    chroms, starts, ends = make_regions(rng, seqs)
    nonc = make_nonc_regions(rng, seqs)
    muts = make_mutations(rng, seqs, 6000)
    out = dict(fasta=fasta, regions=dict(chrom=chroms, start=starts, end=ends), nonc_regions=[list(r) for r in nonc],
               mutations=muts)
    with tempfile.TemporaryDirectory() as tmp:
        f_fasta = os.path.join(tmp, "genome.fa")
        with open(f_fasta, "w") as f:
            f.write(fasta)
        f_mut = os.path.join(tmp, "muts.tsv")
        with open(f_mut, "w") as f:
            f.write(muts)
        df = ref_seq.count_contexts_by_regions(f_fasta, chroms, starts, ends, n_up=2, n_down=2, collapse=False)
        out["by_regions"] = frame(df)
        dfc = ref_seq.count_contexts_by_regions(f_fasta, chroms, starts, ends, n_up=2, n_down=2, collapse=True)
        out["by_regions_collapse"] = frame(dfc)
        trans_idx = ref_seq.mk_trans_idx(2, 2)
        dfn = ref_seq.nonc_elt_context_count(nonc, trans_idx, f_fasta, n_up=2, n_down=2)
        out["nonc"] = frame(dfn)
        # the genome counts of the sequence model: whole chromosomes
        names = list(seqs)
        whole = ref_seq.count_contexts_by_regions(f_fasta, names, [0] * len(names), [len(seqs[n]) for n in names], n_up=2, n_down=2)
        genome_counts = whole.sum(axis=0)
        out["genome_counts"] = dict(index=list(genome_counts.index), values=[int(v) for v in genome_counts.values])
        # identity whitelist (make_golden.py: whitelisting by bed needs bedtools)
        ref_mt.restrict_mutations_by_bed = lambda df_mut, df_bed, unique=True, remove_X=True, replace_cols=False: \
            (df_mut.drop_duplicates() if unique else df_mut).copy()
        df_mut = ref_mt.read_mutation_file(f_mut, drop_duplicates=False)
        df_mut = ref_seq.add_context_to_mutations(f_fasta, df_mut, n_up=2, n_down=2, N_proc=1, collapse=False)
        regions = np.array([[int(n[3:]), 0, len(seqs[n])] for n in names])
        df_freq_mut, df_freq_context = ref_seq.train_sequence_model(regions, df_mut, genome_counts, n_up=2, n_down=2)
        out["annotated"] = df_mut.to_csv(sep="\t", index=False, header=False)
        out["freq_mut"] = dict(MUT_TYPE=list(df_freq_mut.MUT_TYPE), CONTEXT=list(df_freq_mut.CONTEXT),
                               COUNT=[float(v) for v in df_freq_mut.COUNT], FREQ=[float(v) for v in df_freq_mut.FREQ],
                               columns=list(df_freq_mut.columns))
        out["freq_context"] = dict(index=[str(i) for i in df_freq_context.index], FREQ=[float(v) for v in df_freq_context.FREQ],
                                   columns=list(df_freq_context.columns))
        print("regions", df.shape, "collapse", dfc.shape, "nonc", dfn.shape, "mutations", len(df_mut),
              "freq_mut", df_freq_mut.shape, "freq_context", df_freq_context.shape,
              "zero genome contexts", int((genome_counts == 0).sum()))
    with gzip.open(OUT, "wt") as f:
        json.dump(out, f)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
