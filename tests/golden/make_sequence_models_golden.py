"""Generate the many-cohort sequence-model golden (DigPretrain sequenceModels) by running the REAL reference's train_sequence_model
per cohort here.

Run in the build container only (it needs the reference tree, DIG_REFERENCE, default /root/reference):

    python tests/golden/make_sequence_models_golden.py

* Stubs the reference's absent I/O-only dependencies as make_golden.py does and imports the reference from its own location; no
  bytecode is written.
* The reference whitelists with bedtools (pybedtools), which this container does not have: its restrict_mutations_by_bed is replaced
  by this repository's pinned statement of it (digdriver_amd.data_tools.mutation_tools.restrict_mutations_by_bed), as make_golden.py
  and make_penta_context_golden.py replace it.  Everything else -- read_mutation_file(drop_duplicates=True), the INDEL filter of
  DigPretrain.py:194, train_sequence_model, mutation_freq_conditional -- is the reference's own code.
* Inputs (seeded): 180 windows on chromosomes 1, 2 and 3 -- 100 bases wide with gaps of 50 on 1, back to back on 2, back to back on
  3 with one window listed twice and two that overlap; every seventh window has mappability 0.3 and a few exactly the threshold 0.5,
  which does not pass -- and three tri-nucleotide cohorts: `none` (rows on X, Y and chromosome 9 only), `long` (one-base rows and a
  few multi-base rows with an SNV class: across the edge of two back to back windows, inside the doubled window, across the
  overlapping pair, across a window's end into a gap, and an empty interval) and `big` (about 2 000 rows: random positions, rows in
  the doubled window and in the overlap, rows on X, Y and 9, repeats of (CHROM, START, END, REF, ALT, SAMPLE) whose later copy has
  another MUT_TYPE / CONTEXT or ANNOT == 'INDEL', pairs whose FIRST copy is the INDEL, whole-row repeats, indels of several lengths
  shared between samples, and label pairs the table does not hold).  The penta-nucleotide cohort is the annotated mutation text of
  penta_context_golden.json.gz, against the same windows.
* The per-window genome counts follow a rule (tests/sequence_counts_statement.py genome_frame) and are not stored; their column sums
  over the whitelist are, as a check of the rule.
* Stores inputs and expected tables in sequence_models_golden.json -- data only.
"""
import gzip
import json
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True

import numpy as np
import pandas as pd

REF = os.environ.get("DIG_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "sequence_models_golden.json")
MAP_THRESH = 0.5
BASES = "ACGT"


def install_stubs():
    for name in ["pysam", "pybedtools", "h5py", "statsmodels", "statsmodels.stats", "statsmodels.stats.multitest", "seaborn",
                 "bbi", "tables", "gpytorch", "tensorboardX", "pkg_resources"]:
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.path.insert(0, REF)


def windows():
    idx = [(1, 150 * i, 150 * i + 100) for i in range(60)]
    idx += [(2, 100 * i, 100 * i + 100) for i in range(70)]
    idx += [(3, 100 * i, 100 * i + 100) for i in range(40)]
    idx += [(3, 4000, 4100), (3, 4000, 4100), (3, 4200, 4320), (3, 4280, 4400)]
    idx += [(3, 4400 + 100 * i, 4500 + 100 * i) for i in range(6)]
    mapp = [0.3 if i % 7 == 3 else 0.9 for i in range(len(idx))]
    for i in (10, 75, 140):
        mapp[i] = MAP_THRESH                                       # not above the threshold: out
    for i, w in enumerate(idx):
        if w in ((2, 100, 200), (2, 200, 300), (2, 300, 400), (1, 0, 100)) or (w[0] == 3 and w[1] >= 4000 and w[2] <= 4400):
            mapp[i] = 0.9
    return idx, mapp


def make_cohorts(rng):
    length = {1: 9000, 2: 7000, 3: 5000}

    def snv(ch, pos, samp, annot="Noncoding", gene=".", end=None):
        ref = BASES[rng.integers(4)]
        alt = BASES[(BASES.index(ref) + 1 + rng.integers(3)) % 4]
        ctx = BASES[rng.integers(4)] + ref + BASES[rng.integers(4)]
        return [str(ch), int(pos), int(pos) + 1 if end is None else int(end), ref, alt, samp, gene, annot, ref + ">" + alt, ctx]

    def sample():
        return "S%d" % rng.integers(10)

    big = []
    for _ in range(1500):
        ch = int(rng.integers(1, 4))
        big.append(snv(ch, rng.integers(0, length[ch]), sample()))
    big += [snv(3, rng.integers(4000, 4100), sample()) for _ in range(60)]                 # the doubled window
    big += [snv(3, rng.integers(4280, 4320), sample()) for _ in range(60)]                 # inside both overlapping windows
    big += [snv(ch, rng.integers(0, 5000), sample()) for ch in ["X"] * 40 + ["Y"] * 20 + [9] * 30]
    # repeats of (CHROM, START, END, REF, ALT, SAMPLE) in whitelisted windows of chromosome 2: the first copy counts
    for k in range(50):
        first = snv(2, 100 + rng.integers(0, 300), "R%d" % k)
        later = list(first)
        later[9] = BASES[(BASES.index(first[9][0]) + 1) % 4] + first[9][1:]                # another CONTEXT
        if k % 2:
            later[8] = first[3] + ">" + [b for b in BASES if b not in (first[3], first[4])][0]     # and another MUT_TYPE
        big += [first, later]
    for k in range(10):                                                                     # SNV first, INDEL later: counts
        first = snv(2, 100 + rng.integers(0, 300), "Q%d" % k)
        big += [first, first[:7] + ["INDEL"] + first[8:]]
    for k in range(10):                                                                     # INDEL first, SNV later: counts nowhere
        later = snv(2, 100 + rng.integers(0, 300), "P%d" % k)
        big += [later[:7] + ["INDEL"] + later[8:], later]
    for k in range(15):                                                                     # whole-row repeats
        row = snv(2, 100 + rng.integers(0, 300), "W%d" % k)
        big += [row, list(row)]
    for k in range(50):                                                                     # indels: several lengths, shared by samples
        ch = int(rng.integers(1, 4))
        pos = int(rng.integers(0, length[ch] - 10))
        row = [str(ch), pos, pos + int(rng.integers(1, 6)), "-", "ACG"[:int(rng.integers(1, 4))], sample(), "G%d" % rng.integers(3),
               "INDEL", "->A", "NNN"]
        big += [row, row[:5] + [sample()] + row[6:]]
    for k in range(40):                                                                     # label pairs the table does not hold
        row = snv(2, 100 + rng.integers(0, 300), sample())
        how = k % 4
        if how == 0:
            row[9] = row[9][0] + BASES[(BASES.index(row[3]) + 1) % 4] + row[9][2]          # the centre is not REF
        elif how == 1:
            row[9] = "N" + row[9][1:]
        elif how == 2:
            row[8] = row[3] + ">" + row[3]
        else:
            row[9] = row[9].lower()
        big.append(row)

    long = [snv(int(rng.integers(1, 4)), rng.integers(0, 5000), sample()) for _ in range(30)]
    long += [snv(2, 199, "L0", end=201),             # across the edge of two back to back windows: two pieces
             snv(3, 4050, "L1", end=4053),           # in the doubled window: the two pieces are one row
             snv(3, 4270, "L2", end=4290),           # across the overlapping pair: two pieces
             snv(1, 95, "L3", end=105),              # across a window's end into a gap: one piece
             snv(2, 350, "L4", end=350),             # an empty interval
             snv(2, 298, "L5", end=302, annot="Missense", gene="G1")]

    none = [snv(ch, rng.integers(0, 5000), sample()) for ch in ["X"] * 20 + ["Y"] * 5 + [9] * 25]
    text = lambda rows: "".join("\t".join(str(v) for v in r) + "\n" for r in rows)
    return dict(none=text(none), long=text(long), big=text(big))


def main():
    install_stubs()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from DIGDriver.data_tools import mutation_tools as ref_mt       # noqa: E402
    from DIGDriver.sequence_model import sequence_tools as ref_seq  # noqa: E402
    from digdriver_amd.data_tools import mutation_tools as pinned   # noqa: E402
    from sequence_counts_statement import genome_frame              # noqa: E402
    ref_mt.restrict_mutations_by_bed = pinned.restrict_mutations_by_bed

    rng = np.random.default_rng(20261018)
    idx, mapp = windows()
    cohorts = make_cohorts(rng)
    with gzip.open(os.path.join(HERE, "penta_context_golden.json.gz"), "rt") as f:
        penta_text = json.load(f)["annotated"]
    keep = np.array(mapp) > MAP_THRESH
    regions = np.array(idx)[keep]
    out = dict(idx=[list(w) for w in idx], mappability=mapp, map_thresh=MAP_THRESH, cohorts=cohorts, S_genome={}, models=[])
    with tempfile.TemporaryDirectory() as tmp:
        for n_up, names in ((1, ["none", "long", "big"]), (2, ["penta"])):
            contexts = list(ref_seq.mk_context_sequences(n_up, n_up).keys())
            S_genome = genome_frame(len(idx), contexts)[keep].sum(axis=0)
            out["S_genome"][str(n_up)] = [int(v) for v in S_genome.values]
            for name in names:
                f_mut = os.path.join(tmp, name + ".txt")
                with open(f_mut, "w") as f:
                    f.write(penta_text if name == "penta" else cohorts[name])
                df_mut = ref_mt.read_mutation_file(f_mut, drop_duplicates=True)             # DigPretrain.py:192-194
                df_mut = df_mut[df_mut.ANNOT != 'INDEL']
                df_freq_mut, df_freq_context = ref_seq.train_sequence_model(regions, df_mut, S_genome, n_up=n_up, n_down=n_up)
                out["models"].append(dict(
                    cohort=name, n_up=n_up, rows_read=int(len(df_mut)), columns=list(df_freq_mut.columns),
                    MUT_TYPE=list(df_freq_mut.MUT_TYPE) if n_up == 1 else None, CONTEXT=list(df_freq_mut.CONTEXT) if n_up == 1 else None,
                    COUNT=[int(v) for v in df_freq_mut.COUNT], FREQ=[float(v) for v in df_freq_mut.FREQ],
                    context_index=[str(i) for i in df_freq_context.index], context_FREQ=[float(v) for v in df_freq_context.FREQ]))
                print(name, "rows", len(df_mut), "counted", int(df_freq_mut.COUNT.sum()))
    with open(OUT, "w") as f:
        json.dump(out, f)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
