"""The one small problem of test_gpu_tile_samples.py and test_gpu_tile_samples_guarded.py: a synthetic genome with an N run, R = 6
regions of at most 400 positions, C = 3 cohorts with about 2 800 rows.  Everything here is host data made from a seed; nothing is
computed by the library.

Regions (chromosome, start, end):
  0  1:100-500     whole
  1  1:500-850     adjacent to region 0 (a multi-base row spans the border); 350 positions: its last tile of 50 does not exist
  2  1:1000-1400   all N: its tiles exist, their probabilities and p-values do not
  3  1:1850-2250   cut off at the contig's end (2 000 bases): 149 positions
  4  2:200-600     whole, on the second contig
  5  2:899-1000    starts on the contig's last base: no position, n_valid = 0
Cohort 0 holds the rows the kernels can go wrong on:
  HOT     300 rows at 1:160 -- one (tile, sample) at either bin size, longer than a wave (64) and a workgroup (256)
  S0..S69 once each at 1:305 -- one tile hit by 70 samples
  S1      at 1:349 and 1:350 -- the same sample in adjacent tiles (bin size 50: tiles 4 and 5; bin size 1: neighbours)
  S2      1:95-105 -- overlaps region 0, starts in front of it
  S3      1:498-503 -- spans the border of regions 0 and 1, counts in region 0
  S4      1:2020 -- inside region 3's interval, behind its last tile
  S5..S9  in the N run
  HYPER   400 rows all over both contigs -- the sample --max-muts-per-sample 350 drops (HOT, with 300, stays)
and 400 background rows; cohort 1 reuses the labels S0..S39 (other people), cohort 2 has labels of its own.
"""
import itertools

import numpy as np

BINSIZES = (50, 1)
C = 3
MAX_MUTS_PER_SAMPLE = 350
CAP = 2
IDX = np.array([[1, 100, 500], [1, 500, 850], [1, 1000, 1400], [1, 1850, 2250], [2, 200, 600], [2, 899, 1000]], np.int64)
LENGTHS = {"1": 2000, "2": 900}


def genome_sequences():
    rng = np.random.default_rng(11)
    seqs = {name: "".join(rng.choice(list("ACGT"), n)) for name, n in LENGTHS.items()}
    seqs["1"] = seqs["1"][:1000] + "N" * 400 + seqs["1"][1400:]
    return seqs


def s_prob(c):
    rng = np.random.default_rng(100 + c)
    return {"".join(k): float(v) for k, v in zip(itertools.product("ACGT", repeat=3), rng.uniform(0.5, 1.5, 64) * 1e-3)}


def mu_sigma():
    """[C, R] each: about what the background puts into a region, so that ordinary tiles are no hits."""
    mu = np.array([[60.0, 55.0, 50.0, 25.0, 80.0, 1.0], [90.0, 80.0, 70.0, 30.0, 150.0, 1.0], [70.0, 60.0, 60.0, 25.0, 110.0, 1.0]])
    return mu, 0.25 * mu


def _background(rng, n, labels):
    rows = []
    for _ in range(n):
        chrom = "1" if rng.uniform() < 0.7 else "2"
        start = int(rng.integers(0, LENGTHS[chrom]))
        rows.append((chrom, start, start + int(rng.choice([1, 1, 1, 2, 6])), labels[int(rng.integers(0, len(labels)))]))
    return rows


def cohort_rows():
    """Per cohort a list of (chrom, start, end, sample label), in file order (shuffled: a sample's rows are not together)."""
    rng = np.random.default_rng(5)
    special = [("1", 160, 161, "HOT")] * 300 + [("1", 305, 306, "S%d" % d) for d in range(70)]
    special += [("1", 349, 350, "S1"), ("1", 350, 351, "S1"), ("1", 95, 105, "S2"), ("1", 498, 503, "S3"), ("1", 2020, 2021, "S4")]
    special += [("1", 1000 + 70 * d, 1001 + 70 * d, "S%d" % (5 + d)) for d in range(5)]
    c0 = special + _background(rng, 400, ["HYPER"]) + _background(rng, 400, ["S%d" % d for d in range(80)])
    c1 = [("2", 250, 251, "S0"), ("2", 251, 252, "S0")] + _background(rng, 900, ["S%d" % d for d in range(40)])
    c2 = _background(rng, 700, ["T%d" % d for d in range(30)])
    out = []
    for rows in (c0, c1, c2):
        order = rng.permutation(len(rows))
        out.append([rows[i] for i in order])
    return out


def frames(rows_by_cohort):
    """The cohorts as the frames nb_model takes in place of a file: CHROM, START, END, REF, ALT, ID."""
    import pandas as pd
    return [pd.DataFrame({"CHROM": [r[0] for r in rows], "START": [r[1] for r in rows], "END": [r[2] for r in rows], "REF": "A", "ALT": "C",
                          "ID": [r[3] for r in rows]}) for rows in rows_by_cohort]


def write_file(path, rows, chr_prefix=False, gz=False, extra_columns=0):
    """A bed-like mutation file of 6 + extra_columns columns."""
    import gzip
    text = "".join("\t".join([("chr" if chr_prefix else "") + r[0], str(r[1]), str(r[2]), "A", "C", r[3]] + ["x"] * extra_columns) + "\n"
                   for r in rows)
    with (gzip.open(path, "wt") if gz else open(path, "w")) as fh:
        fh.write(text)
    return str(path)


def stacked(rows_by_cohort):
    """The rows of all cohorts as one stack with GLOBAL sample ids (a cohort's labels numbered by first appearance, cohorts one after
    the other): dict(chrom labels, start, end int64, cohort, sample int32, sample_offsets int64 [C + 1], names: per cohort its labels)."""
    chrom, start, end, cohort, sample, names, off = [], [], [], [], [], [], [0]
    for c, rows in enumerate(rows_by_cohort):
        ids = {}
        for r in rows:
            chrom.append(r[0]), start.append(r[1]), end.append(r[2]), cohort.append(c)
            sample.append(off[-1] + ids.setdefault(r[3], len(ids)))
        names.append(list(ids))
        off.append(off[-1] + len(ids))
    return dict(chrom=np.array(chrom), start=np.array(start, np.int64), end=np.array(end, np.int64), cohort=np.array(cohort, np.int32),
                sample=np.array(sample, np.int32), sample_offsets=np.array(off, np.int64), names=names)


def statement_regions(first_pos, n_valid):
    return [(str(c), int(s), int(e), int(f), int(v)) for (c, s, e), f, v in zip(IDX, first_pos, n_valid)]


def statement_rows(st):
    return [(str(ch), int(s), int(e), int(c), int(g)) for ch, s, e, c, g in zip(st["chrom"], st["start"], st["end"], st["cohort"], st["sample"])]
