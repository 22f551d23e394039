"""The problems of test_sparse_tiles_host.py, test_gpu_sparse_tiles.py and test_gpu_sparse_tiles_guarded.py: host data made from
seeds, nothing computed by the library.  The genome is tile_samples_cases' (contig 1: 2 000 bases with an N run at 1000-1400, contig
2: 900 bases); the first problem is that module's own (K.IDX, K.cohort_rows()), the second adds what it lacks.

Regions of the second problem (chromosome, start, end):
  0  1:100-500     whole
  1  1:900-1100    straddles the N run's start: the window of 999 touches the N at 1000, 1000-1099 are N
  2  1:1000-1400   all N: denom 0, no tile testable
  3  1:1850-2250   cut off at the contig's end
  4  2:200-600     whole, on the second contig
  5  2:899-1000    starts on the contig's last base: no position, n_valid = 0
  6  1:300-700     overlaps region 0 on 300-499: the 70 rows at 305 count in both
  7  2:0-150       starts at 0: the first position is n_up
  8  1:1500-1900   the depleted cohort's region; overlaps region 3 on 1850-1899
Cohorts: 0 = tile_samples_cases' cohort 0 (300 rows at 1:160, 70 at 1:305, rows across borders) plus rows at 1:999 (window touches
the N), 1:1000 and 1:1050 (inside it) and a multi-base row 1:348-353 that spans a border of the tiles of 50 (and of 7); 1 = its
cohort 1 with S_prob 0 for a quarter of the contexts; 2 = its cohort 2; 3 = the depleted cohort: three rows in region 8 where
mu = 400 (sigma 40), so that at binsize 50 an EMPTY tile there has PVAL about 1.5^-100 -- a dense hit at pval_max = 1e-3 that the
sparse route leaves out and says so.  Cohorts 4 .. C - 1 repeat the pattern with other seeds (60 rows each): C = 65 crosses the
64-cohort mask word of the census.
mu[1, 3] is NaN and mu[2, 4] is 0: regions without a testable tile that hold rows all the same.
"""
import itertools

import numpy as np

import tile_samples_cases as K

BINSIZES = (1, 7, 50)
IDX = np.array([[1, 100, 500], [1, 900, 1100], [1, 1000, 1400], [1, 1850, 2250], [2, 200, 600], [2, 899, 1000], [1, 300, 700],
                [2, 0, 150], [1, 1500, 1900]], np.int64)
DEPLETED, DEPLETED_REGION = 3, 8
genome_sequences = K.genome_sequences


def regions(idx=IDX):
    return [(str(c), int(s), int(e)) for c, s, e in idx]


def s_prob(c, n_up=1):
    """S_prob of cohort c as the dict nb_model takes; cohorts 1, 5, 9, ... have 0 for a quarter of the contexts."""
    rng = np.random.default_rng(100 + c + 1000 * (n_up - 1))
    n = 4 ** (2 * n_up + 1)
    v = rng.uniform(0.5, 1.5, n) * 1e-3
    if c % 4 == 1:
        v[rng.permutation(n)[:n // 4]] = 0.0
    return {"".join(k): float(x) for k, x in zip(itertools.product("ACGT", repeat=2 * n_up + 1), v)}


def cohort_rows(C):
    """Per cohort a list of (chrom, start, end), in file order."""
    base = [[r[:3] for r in rows] for rows in K.cohort_rows()]
    base[0] = base[0] + [("1", 999, 1000), ("1", 1000, 1001), ("1", 1050, 1051), ("1", 348, 353)]
    base.append([("1", 1510, 1511), ("1", 1510, 1511), ("1", 1777, 1778)])
    out = base[:C]
    for c in range(len(out), C):
        rng = np.random.default_rng(7000 + c)
        out.append([r[:3] for r in K._background(rng, 60, ["x"])])
    return out


def mu_sigma(C, idx=IDX):
    """[C, R] each: about the rows a cohort puts into a region (sigma = mu / 4), with the special entries of the module's text."""
    rows = cohort_rows(C)
    rng = np.random.default_rng(31)
    span = (idx[:, 2] - idx[:, 1]).astype(float)
    mu = np.array([np.maximum(1.0, len(rows[c]) * span / 2900.0) for c in range(C)]) * rng.uniform(0.7, 1.3, (C, len(idx)))
    sigma = 0.25 * mu
    if C > 1:
        mu[1, 3] = np.nan
    if C > 2:
        mu[2, 4] = 0.0
    if C > DEPLETED:
        mu[DEPLETED, DEPLETED_REGION], sigma[DEPLETED, DEPLETED_REGION] = 400.0, 40.0
    return mu, sigma


def frames(rows_by_cohort):
    """The cohorts as the frames nb_model takes in place of a file."""
    import pandas as pd
    return [pd.DataFrame({"CHROM": [r[0] for r in rows], "START": [r[1] for r in rows], "END": [r[2] for r in rows]}) for rows in rows_by_cohort]


def stacked(rows_by_cohort, strays=True):
    """The rows of all cohorts as one stack: dict(chrom labels, start, end int64, cohort int32); with strays two more rows on a
    mutated tile of region 0 whose cohort index lies outside [0, C): they count nowhere."""
    chrom, start, end, cohort = [], [], [], []
    for c, rows in enumerate(rows_by_cohort):
        for r in rows:
            chrom.append(r[0]), start.append(r[1]), end.append(r[2]), cohort.append(c)
    if strays:
        for c in (len(rows_by_cohort), -1):
            chrom.append("1"), start.append(160), end.append(161), cohort.append(c)
    return dict(chrom=np.array(chrom), start=np.array(start, np.int64), end=np.array(end, np.int64), cohort=np.array(cohort, np.int32))


def statement_rows(st):
    return [(str(ch), int(s), int(e), int(c)) for ch, s, e, c in zip(st["chrom"], st["start"], st["end"], st["cohort"])]


def write_file(path, rows):
    """A bed-like mutation file of 6 columns."""
    with open(path, "w") as fh:
        fh.write("".join("\t".join([r[0], str(r[1]), str(r[2]), "A", "C", "x"]) + "\n" for r in rows))
    return str(path)
