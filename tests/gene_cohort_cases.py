"""Inputs shared by test_gene_cohorts_host.py and test_gpu_gene_cohorts.py: small annotated cohort files and gene models with one
gene index, and the route from a file to the tuples gene_obs_statement.py counts.  No test in here."""
import numpy as np
import pandas as pd

GENES = ["G%02d" % i for i in range(10)] + ["TP53", "KRAS"]          # the models' gene index: TP53 and one CGC gene among 12
ALL_COSMIC = ["KRAS"]
_ANNOTS = ["Synonymous", "Missense", "Nonsense", "Essential_Splice", "INDEL", "Stop_loss", "Noncoding"]
_OBS = ["OBS_SYN", "OBS_MIS", "OBS_NONS", "OBS_SPL", "OBS_INDEL"]


def cohort_rows(seed, n, samples, indels=True, extra=(), absent=None):
    """n random rows (8 columns: CHROM START END REF ALT SAMPLE GENE ANNOT) + `extra`: about a tenth without a gene label, a few
    on X, genes outside the model, Stop_loss and labelled Noncoding rows; the annotations are skewed so that some (gene, sample,
    class) cells hold three rows and more; indels come from a small pool of positions, so that samples share them.  absent: a
    gene that gets no row (the serial route's count table then lacks it, and its left join leaves float OBS_* columns)."""
    rng = np.random.RandomState(seed)
    genes = GENES + ["OUT1", "OUT2", "."]
    p_gene = np.array([3, 3, 2, 2, 1, 1, 1, 1, 1, 1, 2, 2, 1, 1, 2], float)
    p_annot = np.array([5, 7, 2, 1, 2 if indels else 0, 0.5, 0.5], float)
    rows = []
    for _ in range(n):
        gene = genes[rng.choice(len(genes), p=p_gene / p_gene.sum())]
        gene = GENES[0] if gene == absent else gene
        annot = "Noncoding" if gene == "." else _ANNOTS[rng.choice(len(_ANNOTS), p=p_annot / p_annot.sum())]
        chrom = "X" if rng.rand() < 0.02 else str(rng.randint(1, 23))
        sample = samples[rng.randint(len(samples))]
        if annot == "INDEL":
            start = 5000 + 10 * int(rng.randint(12))
            rows.append((chrom if chrom == "X" else "7", start, start + 3, "ACG", "A", sample, gene, annot))
        else:
            start = int(rng.randint(1000, 3000))
            rows.append((chrom, start, start + 1, "ACGT"[rng.randint(4)], "ACGT"[rng.randint(4)], sample, gene, annot))
    return rows + list(extra)


def write_rows(path, rows):
    with open(path, "w") as f:
        for r in rows:
            f.write("\t".join(str(x) for x in r) + "\n")
    return str(path)


def small_case(tmp):
    """C = 3, about 9 samples and 400 coding rows per cohort: cohort 1 holds one sample with 150 rows more than the others (the one
    max_muts_per_sample = 150 removes), cohort 2 has no INDEL row and no row of G09; the per-gene-per-sample cap is 2."""
    files = []
    for c in range(3):
        samples = ["S%d_%d" % (c, j) for j in range(9)]
        extra = [("3", 100 + i, 101 + i, "A", "C", samples[8], GENES[i % 12], _ANNOTS[i % 4]) for i in range(150)] if c == 1 else ()
        files.append(write_rows(tmp / ("cohort%d.tsv" % c), cohort_rows(100 + c, 450, samples, indels=(c != 2), extra=extra, absent="G09" if c == 2 else None)))
    return dict(files=files, C=3, max_muts_per_sample=150, max_muts_per_gene_per_sample=2)


def long_run_case(tmp):
    """About 3 000 rows in two cohorts; in cohort 0 one (gene, sample) pair holds 700 Missense rows -- a run of sorted keys across
    three workgroups and more -- under a cap of 500."""
    big = [("5", 20000 + i, 20001 + i, "A", "G", "BIG", "G03", "Missense") for i in range(700)]
    files = [write_rows(tmp / "long0.tsv", cohort_rows(7, 2400, ["L0_%d" % j for j in range(30)], extra=big)),
             write_rows(tmp / "long1.tsv", cohort_rows(8, 300, ["L1_%d" % j for j in range(5)]))]
    return dict(files=files, C=2, max_muts_per_sample=3e9, max_muts_per_gene_per_sample=500)


# (sample, rows) runs of lane_run_case, in file order.  Rows 0 .. 599 in workgroups of 256 rows and waves of 64:
#   sample 0 starts at lane 0 and comes back in a second run (10 + 46 rows); 1 starts in the middle of a wave; 3 is one row at lane
#   63 and 4 one row at lane 0; 6 (56 rows) crosses a wave boundary (row 128) and 8 (55 rows) a workgroup boundary (row 256); 9 and
#   10 are single rows side by side; 12 (56 rows) ends at lane 63 (row 383); 13 fills three whole waves; 14 is row 576, lane 0 of the
#   last wave.  The totals of the runs on the edges are 55 and 56, so that under the limits 54, 55 and 56 each of them is once the
#   limit and once the limit + 1: one lane lost or counted twice changes a blacklist byte.
LANE_RUNS = [(0, 10), (1, 30), (2, 23), (3, 1), (4, 1), (5, 35), (6, 56), (0, 46), (7, 28), (8, 55), (9, 1), (10, 1), (11, 41), (12, 56),
             (13, 192), (14, 1), (15, 23)]
LANE_RUN_LIMITS = (54, 55, 56)


def lane_run_case(tmp, n, limit):
    """One cohort whose first n rows (600: all; 577: row 576 is alone in its wave) are those of LANE_RUNS, every row a coding row
    that every reader keeps; genes of the model and one outside it, all six classes, a per-gene-per-sample cap of 2."""
    sample = np.repeat([s for s, _ in LANE_RUNS], [k for _, k in LANE_RUNS])[:n]
    genes = GENES + ["OUT1"]
    rows = [("1", 1000 + 10 * i, 1001 + 10 * i, "A", "C", "R%02d" % s, genes[i % 13], _ANNOTS[(i // 3) % 6]) for i, s in enumerate(sample)]
    return dict(files=[write_rows(tmp / ("lanes%d.tsv" % n), rows)], C=1, max_muts_per_sample=limit,
                max_muts_per_gene_per_sample=2, sample=sample)


def coding_tuples(f_mut):
    """(gene, sample, annot) of the coding rows of a file, as the serial route reads them."""
    from digdriver_amd.driver_model import transfer_tools as tt
    rows = tt.read_mutations_cds(f_mut)
    return rows, list(zip(rows.GENE.tolist(), rows.SAMPLE.tolist(), rows.ANNOT.tolist()))


def model_frame(c, genes=GENES):
    """The stored gene model of cohort c (the columns of a map's genic_model frame)."""
    rng = np.random.RandomState(500 + c)
    G = len(genes)
    mu = rng.uniform(20, 200, G)
    p = rng.uniform(1e-3, 3e-3, (G, 4))
    return pd.DataFrame(dict(CHROM=[str(1 + i % 22) for i in range(G)], GENE=list(genes), GENE_LENGTH=rng.randint(600, 6000, G),
                             R_SIZE=rng.randint(20000, 40000, G), R_OBS=rng.randint(50, 400, G), R_INDEL=rng.randint(5, 40, G),
                             MU=mu, SIGMA=mu * rng.uniform(0.2, 0.5, G), MU_INDEL=mu * 0.1, SIGMA_INDEL=mu * 0.04,
                             FLAG=np.zeros(G, np.int64), P_MIS=p[:, 0], P_NONS=p[:, 1] * 0.1, P_SILENT=p[:, 2] * 0.4,
                             P_SPLICE=p[:, 3] * 0.05, P_TRUNC=p[:, 1] * 0.1 + p[:, 3] * 0.05, P_INDEL=rng.uniform(0.02, 0.2, G)))


def write_maps(tmp, C, genes=GENES):
    from digdriver_amd.io import mapfile
    paths = []
    for c in range(C):
        paths.append(str(tmp / ("genes%d.map" % c)))
        mapfile.write_frame(paths[-1], "genic_model", model_frame(c, genes))
    return paths


def statement_planes(case, genes=GENES):
    """The statement's counts of a case as the arrays engine.gene_counts returns (obs [G, 5, C], n_samp [G, 6, C], n_samp_indel and
    n_pairs [G, C], n_syn [C], the blacklisted sample names per cohort), and the statement's own dicts."""
    import gene_obs_statement as S
    G, C = len(genes), case["C"]
    obs, n_samp = np.zeros((G, 5, C), np.int32), np.zeros((G, 6, C), np.int32)
    n_samp_indel, n_pairs, n_syn = np.zeros((G, C), np.int32), np.zeros((G, C), np.int32), np.zeros(C, np.int64)
    black, raw = [], []
    for c, f in enumerate(case["files"]):
        st = S.cohort_counts(coding_tuples(f)[1], genes, case["max_muts_per_sample"], case["max_muts_per_gene_per_sample"])
        raw.append(st)
        for g, gene in enumerate(genes):
            for a, annot in enumerate(S.OBS_CLASSES):
                obs[g, a, c] = st["obs"].get((gene, annot), 0)
            for q, cls in enumerate(("SYN", "MIS", "NONS", "SPL", "TRUNC", "NONSYN")):
                n_samp[g, q, c] = st["n_samp"].get((gene, cls), 0)
            n_samp_indel[g, c] = st["n_samp"].get((gene, "INDEL"), 0)
            n_pairs[g, c] = st["pairs"].get(gene, 0)
        n_syn[c] = st["n_syn"]
        black.append(sorted(st["blacklist"]))
    return dict(obs=obs, n_samp=n_samp, n_samp_indel=n_samp_indel, n_pairs=n_pairs, n_syn=n_syn, blacklist=black, raw=raw)
