"""Inputs shared by test_target_cohorts_host.py, test_gpu_target_cohorts.py and test_gpu_panel_counts_guarded.py: a hand-written
cohort file, gene panels, gene models that carry the N_MUT_* / N_SAMPLE_* attributes, and small row sets for the panel-count
kernel with the statement's counts beside them.  Built on gene_cohort_cases.py's writers.  No test in here."""
import numpy as np

import gene_cohort_cases as K
import panel_counts_statement as S

CLASSES = {"Synonymous": 0, "Missense": 1, "Nonsense": 2, "Essential_Splice": 3, "INDEL": 4, "Noncoding": 6}      # anything else: 5

# ---- the hand-written file ---------------------------------------------------------------------------------------------------
HAND_PANELS = {"MSK_341": ["PA", "PB", "BOTH"], "MSK_230": ["BOTH", "PC"]}
HAND_ROWS = [
    ("1", 100, 101, "A", "C", "S1", "PA", "Missense"),
    ("1", 100, 101, "A", "C", "S1", "PA", "Missense"),            # the same mutation listed twice for one sample: counted once
    ("2", 200, 203, "ACG", "A", "S1", "PB", "INDEL"),
    ("2", 200, 203, "ACG", "A", "S2", "PB", "INDEL"),             # the same indel under the same gene: S2 has no other row and drops out
    ("X", 300, 301, "A", "G", "S1", "PA", "Missense"),            # not an autosome
    ("3", 400, 401, "A", "G", "S3", "PA", "Noncoding"),           # a panel gene's label on a Noncoding row: never counted
    ("3", 410, 411, "A", "G", "S3", "PA", "Stop_loss"),           # any other label counts
    ("4", 500, 501, "C", "T", "S3", "PB", "Synonymous"),          # not counted
    ("4", 510, 511, "C", "T", "S4", "PB", "Essential_Splice"),    # not counted
    ("5", 600, 601, "G", "T", "S4", "BOTH", "Nonsense"),          # a gene in two panels
    ("5", 610, 611, "G", "T", "S1", "NONE1", "Missense"),         # a gene in none
    ("6", 700, 701, "G", "A", "S5", ".", "Noncoding"),            # no gene label
    ("6", 710, 711, "G", "A", "S5", "PC", "Missense"),
]
# what the statement must say about it (worked out by hand from the comments above)
HAND_COUNTS = dict(n_cds=8, n_samples=4, panels={"MSK_341": dict(n_mut=4, n_pairs=4, n_sample=3),
                                                 "MSK_230": dict(n_mut=2, n_pairs=2, n_sample=2)})


def hand_file(tmp):
    return K.write_rows(tmp / "hand.tsv", HAND_ROWS)


def file_tuples(f_mut):
    """(gene, sample, annot) of the rows the scale factor starts from, as the serial route reads them."""
    from digdriver_amd.data_tools import mutation_tools
    rows = mutation_tools.read_mutation_file(f_mut, drop_duplicates=True)
    return list(zip(rows.GENE.tolist(), rows.SAMPLE.tolist(), rows.ANNOT.tolist()))


# ---- panels, maps and cohort files of the route tests ------------------------------------------------------------------------
ROUTE_PANELS = {"MSK_341": ["G00", "G01", "G02", "G03", "G05", "TP53", "KRAS", "OUT1"], "MSK_230": ["G01", "G02", "G04", "KRAS", "OUT2"],
                "CGC_ALL": ["G02", "G03", "G06", "KRAS", "TP53"]}
HYPER_LIMIT = 60           # tested rows per sample: only the sample of small_case's cohort 1 that carries 150 rows more is above it


def write_panel_dir(tmp, panels=ROUTE_PANELS):
    d = tmp / "panels"
    d.mkdir(exist_ok=True)
    for name, genes in panels.items():
        (d / ("genes_%s.txt" % name)).write_text("\n".join(genes) + "\n")
    return str(d)


def write_target_maps(tmp, C, genes=K.GENES, attrs=True, regions=False):
    """C maps with the gene models of gene_cohort_cases and, per map, the attributes the panel scale factors divide by (different in
    every map); regions: also a small region_params frame, for countMutations."""
    import pandas as pd
    from digdriver_amd.io import mapfile
    paths = K.write_maps(tmp, C, genes)
    for c, path in enumerate(paths):
        if attrs:
            mapfile.write_attrs(path, N_MUT_MSK_341=1000 + 37 * c, N_SAMPLE_MSK_341=40 + 3 * c, N_MUT_MSK_230=700 + 11 * c,
                                N_SAMPLE_MSK_230=30 + 7 * c)
        if regions:
            rng = np.random.RandomState(900 + c)
            mapfile.write_frame(path, "region_params", pd.DataFrame(dict(
                CHROM=np.ones(20, np.int64), START=np.arange(20) * 100, END=np.arange(20) * 100 + 100, Y_TRUE=rng.randint(0, 50, 20),
                Y_PRED=rng.uniform(1, 40, 20), STD=rng.uniform(1, 4, 20), FLAG=(rng.rand(20) < 0.2))))
    return paths


# ---- row sets for the kernel ---------------------------------------------------------------------------------------------------
def encode(cohorts, panels, blacklists=None):
    """cohorts: per cohort the (gene, sample, annot) tuples in row order; panels: dict name -> genes; blacklists: per cohort the
    sample names left out.  Returns the arguments of engine.panel_counts as a dict (label, sample, annot, cohort, sample_offsets,
    label_mask, P, skip) and `want`: the statement's counts as the arrays the engine returns."""
    labels, bits = {}, []
    for p, genes in enumerate(panels.values()):
        for g in genes:
            if g not in labels:
                labels[g] = len(bits)
                bits.append(0)
            bits[labels[g]] |= 1 << p
    L, P, C = len(bits), len(panels), len(cohorts)
    blacklists = blacklists or [()] * C
    label, sample, annot, cohort, off, skip = [], [], [], [], [0], []
    want = dict(n_mut=np.zeros((C, P), np.int64), n_pairs=np.zeros((C, P), np.int64), n_sample=np.zeros((C, P), np.int64),
                n_cds=np.zeros(C, np.int64))
    for c, tuples in enumerate(cohorts):
        ids = {}
        for g, s, a in tuples:
            label.append(labels.get(g, L))
            sample.append(ids.setdefault(s, len(ids)))
            annot.append(CLASSES.get(a, 5))
            cohort.append(c)
        off.append(off[-1] + len(ids))
        skip += [int(s in set(blacklists[c])) for s in ids]
        st = S.cohort_panel_counts(tuples, panels, blacklists[c])
        want["n_cds"][c] = st["n_cds"]
        for p, name in enumerate(panels):
            for k in ("n_mut", "n_pairs", "n_sample"):
                want[k][c, p] = st["panels"][name][k]
    args = dict(label=np.array(label, np.int32), sample=np.array(sample, np.int32), annot=np.array(annot, np.uint8),
                cohort=np.array(cohort, np.int32), sample_offsets=np.array(off, np.int64),
                label_mask=np.array(bits, np.uint64).astype(np.uint32), P=P, skip=np.array(skip, np.uint8) if any(skip) else None)
    return args, want


_ANNOTS = ["Synonymous", "Missense", "Nonsense", "Essential_Splice", "INDEL", "Stop_loss", "Noncoding"]
_TWO = {"A": ["G00", "G01", "G02", "G03", "G04", "G05"], "B": ["G04", "G05", "G06", "G07", "KRAS"]}


def lane_case(n):
    """The first n rows (600: all; 577: row 576 alone in its wave) of gene_cohort_cases.LANE_RUNS, laid on THREE cohorts run by run, so
    that the runs of one cohort -- the segments the keys kernel adds n_cds by -- begin at lane 0, end at lane 63 and cross the wave
    (row 128) and workgroup (row 256) boundaries; every third row of a run of sample 5 or 12 is Noncoding and sample 7 of its
    cohort is blacklisted, which breaks and removes segments.  The rows of a cohort are not contiguous: the kernels do not need it."""
    cohorts, r = [[], [], []], 0
    genes = K.GENES + ["OUT1"]
    for run, (s, k) in enumerate(K.LANE_RUNS):
        for j in range(k):
            if r < n:
                annot = "Noncoding" if s in (5, 12) and j % 3 == 0 else _ANNOTS[(r // 3) % 6]
                cohorts[run % 3].append((r, genes[r % 13], "R%02d" % s, annot))
            r += 1
    return cohorts


def kernel_cases():
    """name -> (arguments of engine.panel_counts, the statement's counts)."""
    cases = {}
    for n in (600, 577):
        by_cohort = lane_case(n)
        args, want = encode([[(g, s, a) for _, g, s, a in rows] for rows in by_cohort], _TWO, [(), (), ("R07",)])
        # the engine takes rows in any order: the stacked rows (cohort by cohort) go back to where lane_case numbered them
        order = np.argsort(np.array([r for rows in by_cohort for r, _, _, _ in rows]))
        for k in ("label", "sample", "annot", "cohort"):
            args[k] = np.ascontiguousarray(args[k][order])
        cases["lanes%d" % n] = (args, want)
    long_run = [("G03", "BIG", "Missense")] * 700 + [("G00", "S%d" % (i % 5), _ANNOTS[i % 7]) for i in range(60)]
    cases["long_run"] = encode([long_run], _TWO)
    many = {"P0": ["L%02d" % i for i in range(0, 80, 2)], "P1": ["L%02d" % i for i in range(1, 80, 2)] + ["L00"]}
    rows = [("L%02d" % i, "ONE", "Missense") for i in range(70)] * 2 + [("L75", "TWO", "Nonsense"), ("L76", "TWO", "INDEL")]
    cases["seventy_labels"] = encode([rows], many)
    cases["one_panel"] = encode([[("G00", "a", "Missense"), ("G01", "a", "Nonsense"), ("G00", "b", "Missense"), ("G09", "b", "Missense")]],
                                {"ONLY": ["G00", "G01"]})
    wide = {"p%02d" % p: ["COMMON"] + (["HIGH", "PAIR"] if p == 31 else []) + (["PAIR"] if p == 0 else []) for p in range(32)}
    cases["panel_31"] = encode([[("HIGH", "a", "Missense"), ("HIGH", "a", "Missense"), ("PAIR", "b", "INDEL"), ("COMMON", "c", "Stop_loss"),
                                 ("HIGH", "c", "Nonsense")], [("HIGH", "z", "Missense")]], wide)
    cases["one_label"] = encode([[("G", "a", "Missense"), ("G", "a", "Missense"), ("G", "b", "Synonymous"), ("H", "c", "Missense")]], {"ONE": ["G"]})
    cases["empty_cohorts"] = encode([[("G00", "a", "Missense")], [("G00", "q", "Synonymous"), ("G01", "q", "Noncoding"), ("G09", "r", "Missense")],
                                     [], [("G04", "z", "INDEL"), ("G04", "z", "INDEL")]], _TWO)
    between = [("G00", "A", "Missense"), ("G01", "B", "Missense"), ("G02", "C", "Nonsense"), ("G00", "B", "INDEL"), ("G04", "A", "Missense"),
               ("G04", "B", "Missense"), ("G05", "C", "Stop_loss")]
    cases["blacklist_between"] = encode([between], _TWO, [("B",)])
    return cases


def first_rows(args, n):
    """The first n rows of a case's arguments (the tables as they are)."""
    out = dict(args)
    for k in ("label", "sample", "annot", "cohort"):
        out[k] = np.ascontiguousarray(args[k][:n])
    return out


def statement_of(args):
    """The statement's counts of encoded arguments (rows cut by first_rows): the tuples are rebuilt from the ids."""
    C, P = len(args["sample_offsets"]) - 1, args["P"]
    L = len(args["label_mask"])
    names = {v: k for k, v in CLASSES.items()}
    panels = {"p%d" % p: [l for l in range(L) if (int(args["label_mask"][l]) >> p) & 1] for p in range(P)}
    want = dict(n_mut=np.zeros((C, P), np.int64), n_pairs=np.zeros((C, P), np.int64), n_sample=np.zeros((C, P), np.int64),
                n_cds=np.zeros(C, np.int64))
    for c in range(C):
        at = np.flatnonzero(args["cohort"] == c)
        tuples = [(int(args["label"][i]), int(args["sample"][i]), names.get(int(args["annot"][i]), "Other")) for i in at]
        black = () if args["skip"] is None else [s for s in range(int(args["sample_offsets"][c + 1] - args["sample_offsets"][c]))
                                                   if args["skip"][args["sample_offsets"][c] + s]]
        st = S.cohort_panel_counts(tuples, panels, black)
        want["n_cds"][c] = st["n_cds"]
        for p in range(P):
            for k in ("n_mut", "n_pairs", "n_sample"):
                want[k][c, p] = st["panels"]["p%d" % p][k]
    return want
