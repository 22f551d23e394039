"""Generate the addMutationContext golden fixture by running the REAL reference here.

Run in the build container only (it needs the reference tree, DIG_REFERENCE, default /root/reference):

    python tests/golden/make_mutation_context_golden.py

* Stubs the reference's absent I/O-only dependencies as make_golden.py does; pysam.FastaFile is replaced by a stand-in whose
  fetch(chrom) returns the whole chromosome as the FASTA spells it (mutation_contexts_by_chrom only fetches whole chromosomes).
* Builds a small seeded genome (three chromosomes with N runs, soft-masked stretches and a few R / M / Y letters) and mutation
  files that exercise every rule of the reference: runs with a mismatch in the middle, MNVs, lower-case REF, chromosome ends,
  START < n_up, chr1 / X rows, NaN-like GENE labels, INDEL duplicates, SNV / indel ties on (CHROM, START, END).
* Runs the reference's read_mutation_file + add_context_to_mutations for each case and stores the frame as to_csv writes it
  (sep TAB, no index, no header), its index labels and dtypes -- data only -- in mutation_context_golden.json.gz.
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
OUT = os.path.join(HERE, "mutation_context_golden.json.gz")


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


class _WholeFasta:
    """pysam.FastaFile stand-in: fetch(chrom) -> the whole chromosome."""
    def __init__(self, path):
        self._seqs = _read_fasta(path)

    def fetch(self, chrom):
        return self._seqs[chrom]


def install_stubs():
    for name in ["pysam", "pybedtools", "h5py", "statsmodels", "statsmodels.stats", "statsmodels.stats.multitest", "seaborn",
                 "bbi", "tables", "gpytorch", "tensorboardX", "pkg_resources"]:
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["pysam"].FastaFile = _WholeFasta
    sys.path.insert(0, REF)


def make_genome(rng):
    seqs = {}
    for name, n in (("chr1", 3000), ("chr2", 2200), ("chr3", 1700)):
        s = rng.choice(list("ACGT"), n)
        for _ in range(4):                                        # N runs (one at either end of chr3)
            a = int(rng.integers(0, n - 40))
            s[a:a + int(rng.integers(1, 30))] = "N"
        if name == "chr3":
            s[:5] = "N"
            s[-4:] = "N"
        for _ in range(6):                                        # IUPAC letters, single and in pairs
            a = int(rng.integers(0, n - 2))
            s[a:a + int(rng.integers(1, 3))] = rng.choice(list("RMY"))
        s = "".join(s)
        for _ in range(5):                                        # soft-masked stretches
            a = int(rng.integers(0, n - 200))
            b = a + int(rng.integers(10, 200))
            s = s[:a] + s[a:b].lower() + s[b:]
        seqs[name] = s
    return seqs


def make_rows(rng, seqs, n, nan_genes, edges, indels, chrom_noise):
    up = {k: v.upper() for k, v in seqs.items()}
    rows = []

    def snv(c, pos, ref=None, alt=None):
        ref = up["chr%d" % c][pos] if ref is None else ref
        alt = alt or str(rng.choice([b for b in "ACGT" if b != ref] or ["A"]))
        gene = "G%d" % rng.integers(0, 6)
        if nan_genes and rng.random() < 0.1:
            gene = str(rng.choice(["NA", "", "nan", "NULL"]))
        annot = str(rng.choice(["Missense", "Synonymous", "Nonsense", "Essential_Splice"]))
        rows.append([str(c), pos, pos + len(ref), ref, alt, "S%d" % rng.integers(0, 7), gene, annot])

    for _ in range(n):
        c = int(rng.integers(1, 4))
        L = len(up["chr%d" % c])
        pos = int(rng.integers(3, L - 3))
        r = rng.random()
        if r < 0.70:
            snv(c, pos)
        elif r < 0.78:                                            # mismatch
            snv(c, pos, ref=str(rng.choice(list("ACGT"))))
        elif r < 0.83:                                            # lower-case REF
            snv(c, pos, ref=up["chr%d" % c][pos].lower())
        elif r < 0.87:                                            # MNV
            snv(c, pos, ref=up["chr%d" % c][pos:pos + 2])
        else:                                                     # a run: same START, a mismatch somewhere in it
            k = int(rng.integers(2, 5))
            bad = int(rng.integers(0, k + 1))
            for j in range(k):
                snv(c, pos, ref=None if j != bad else str(rng.choice([b for b in "ACGT" if b != up["chr%d" % c][pos]] or ["A"])))
    if edges:                                                     # chromosome ends and START < n_up
        for c in (1, 2, 3):
            L = len(up["chr%d" % c])
            for pos in (0, 1, 2, L - 1, L - 2, L - 3):
                snv(c, pos)
    if chrom_noise:                                               # dropped by read_mutation_file
        rows.append(["chr1", 100, 101, up["chr1"][100], "T", "S1", "G1", "Missense"])
        rows.append(["X", 100, 101, "A", "T", "S1", "G1", "Missense"])
        rows.append(["01", 100, 101, up["chr1"][100], "T", "S1", "G1", "Missense"])
    if indels:
        snv_rows = [r for r in rows if r[0] in ("1", "2", "3")]
        for j in range(12):
            base = snv_rows[int(rng.integers(0, len(snv_rows)))]
            row = [base[0], base[1], base[2], "-" if j % 2 else base[3], "AT" if j % 3 else "-", "S%d" % rng.integers(0, 7),
                   base[6] if base[6] else "G0", "INDEL"]
            rows.append(row)                                      # ties with the SNV row on (CHROM, START, END)
            if j % 4 == 0:
                rows.append(list(row[:5]) + ["S9"] + row[6:])    # a duplicate (another sample): removed
        rows.append(["2", 500, 503, "ACG", "-", "S2", "G2", "FRAMESHIFT_INDEL"])      # contains INDEL, not de-duplicated
        rows.append(["2", 500, 503, "ACG", "-", "S3", "G2", "FRAMESHIFT_INDEL"])
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    return "".join("\t".join(str(x) for x in r) + "\n" for r in rows)


def main():
    install_stubs()
    from DIGDriver.data_tools import mutation_tools as ref_mt       # noqa: E402
    from DIGDriver.sequence_model import sequence_tools as ref_seq  # noqa: E402

    rng = np.random.default_rng(20261016)
    seqs = make_genome(rng)
    fasta = "".join(">%s\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))) for n, s in seqs.items())
    inputs = {
        "plain": make_rows(rng, seqs, 500, nan_genes=False, edges=True, indels=True, chrom_noise=True),
        "nan_genes": make_rows(rng, seqs, 400, nan_genes=True, edges=True, indels=True, chrom_noise=True),
        "snv_only": make_rows(rng, seqs, 400, nan_genes=False, edges=True, indels=False, chrom_noise=False),
        "collapse": make_rows(rng, seqs, 500, nan_genes=False, edges=False, indels=True, chrom_noise=False),
        "indel_only": "".join(l + "\n" for l in make_rows(rng, seqs, 200, False, False, True, False).splitlines()
                              if l.endswith("INDEL")),
    }
    runs = [("plain", 1, 1, False), ("plain", 2, 2, False), ("plain", 1, 0, False),
            ("nan_genes", 1, 1, False), ("nan_genes", 2, 2, False), ("nan_genes", 1, 0, False),
            ("snv_only", 1, 1, False), ("snv_only", 2, 2, False), ("snv_only", 1, 0, False),
            ("collapse", 1, 1, True), ("collapse", 2, 2, True), ("collapse", 1, 0, True), ("collapse", 1, 1, False),
            ("indel_only", 1, 1, False)]
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        f_fasta = os.path.join(tmp, "genome.fa")
        with open(f_fasta, "w") as f:
            f.write(fasta)
        for name, n_up, n_down, collapse in runs:
            f_mut = os.path.join(tmp, name + ".tsv")
            with open(f_mut, "w") as f:
                f.write(inputs[name])
            df_mut = ref_mt.read_mutation_file(f_mut, drop_duplicates=False)
            df = ref_seq.add_context_to_mutations(f_fasta, df_mut, n_up=n_up, n_down=n_down, N_proc=1, collapse=collapse)
            cases.append(dict(input=name, n_up=n_up, n_down=n_down, collapse=collapse,
                              expected=df.to_csv(sep="\t", index=False, header=False),
                              index=[int(i) for i in df.index], columns=list(df.columns),
                              dtypes=[str(t) for t in df.dtypes]))
            print(name, n_up, n_down, collapse, len(df_mut), "->", len(df))
    with gzip.open(OUT, "wt") as f:
        json.dump(dict(fasta=fasta, inputs=inputs, cases=cases), f)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
