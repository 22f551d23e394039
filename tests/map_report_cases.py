"""The map report's test cases: the fixture made with the reference's own functions (tests/golden/make_map_report_golden.py), small
synthetic maps at the shapes where dig_map_windows takes another path, and what the numpy statement (map_report_statement.py) with
the test-side p-value functions (oracle/dig_oracle.py) makes of a case.  Shared by the CPU and the GPU tests; nothing here needs a
GPU."""
import functools
import os

import numpy as np

import map_report_statement as S
from conftest import GOLDEN

TAILS = ("upper", "side")
W = 10_000


@functools.lru_cache(maxsize=None)
def load_fixture():
    with np.load(os.path.join(GOLDEN, "map_report_golden.npz")) as z:
        return {k: z[k] for k in z.files}


def fixture_case():
    fx = load_fixture()
    return dict(chrom=fx["chrom"], start=fx["start"], window=int(fx["window"]), mu=fx["mu"], std=fx["std"], y=fx["y"], flag=fx["flag"])


def make_case(C, chrom_bins, seed, gaps=True):
    """C maps on a grid of sum(chrom_bins) bins of W (with gaps=True a tenth of the slots of a chromosome are missing): Y_PRED ~ Gamma(9,
    3), STD ~ Gamma(4, 1), Y_TRUE from the map's own negative binomial, one cohort in three x 300, FLAG on 8 % of the bins; a STD = 0, a
    Y_PRED = 0, a negative and a NaN Y_PRED where there is room."""
    rng = np.random.default_rng(seed)
    chrom, start = [], []
    for c, n in enumerate(chrom_bins, 1):
        slots = np.arange(n + n // 10) if gaps else np.arange(n)
        keep = np.sort(rng.choice(slots, n, replace=False))
        chrom.append(np.full(n, c, np.int32))
        start.append(keep.astype(np.int64) * W)
    chrom, start = np.concatenate(chrom), np.concatenate(start)
    N = len(chrom)
    mu, sd = rng.gamma(9.0, 3.0, (C, N)), rng.gamma(4.0, 1.0, (C, N))
    mu[1::3] *= 300.0
    sd[1::3] *= 300.0
    y = rng.poisson(rng.gamma(mu ** 2 / sd ** 2, sd ** 2 / mu)).astype(np.int32)
    flag = (rng.uniform(size=(C, N)) < 0.08).astype(np.uint8)
    if N >= 16:
        bad = rng.choice(N, 4, replace=False)
        sd[0, bad[0]], mu[0, bad[1]], mu[0, bad[2]], mu[0, bad[3]] = 0.0, 0.0, -mu[0, bad[2]], np.nan
    return dict(chrom=chrom, start=start, window=W, mu=mu, std=sd, y=y, flag=flag)


# (name, C, bins per chromosome, scale in bins, gaps): the shapes of the GPU test
SHAPES = [("1x1_s1", 1, (1,), 1, False), ("1x2_s2", 1, (2,), 2, False), ("37x257_s1", 37, (257,), 1, True),
          ("37x301_s3", 37, (101, 97, 103), 3, True), ("3x1003_s100", 3, (1003,), 100, True),
          ("2x20011_chrom", 2, (20011,), 10 ** 7, False)]


def shape_case(name):
    _, C, bins, s, gaps = next(t for t in SHAPES if t[0] == name)
    return make_case(C, bins, 1000 + len(name) + C, gaps), s


def expected(case, s, drop_flagged, tail):
    """The statement on a case at scale s (bins): dict(run_ptr, CHROM, START, END, planes n_bins / y_true / y_pred / std / pval [C, M],
    counts [C, 7], sums [C, 4]) with the p-values of the test-side functions."""
    from oracle import dig_oracle as O
    ptr, w_chrom, w_start, w_end = S.run_ptr(case["chrom"], case["start"], s * case["window"])
    C, M = case["mu"].shape[0], len(ptr) - 1
    planes = dict(n_bins=np.zeros((C, M), np.int32), y_true=np.zeros((C, M), np.int64), y_pred=np.zeros((C, M)), std=np.zeros((C, M)),
                  pval=np.zeros((C, M)))
    counts, sums = np.zeros((C, 7), np.int64), np.zeros((C, 4))
    for c in range(C):
        w = S.merge(case["mu"][c], case["std"][c], case["y"][c], case["flag"][c], ptr, drop_flagged)
        w["pval"] = S.pvalues(w, tail, O.normal_params_to_gamma, O.nb_pvalue_greater_midp, O.nb_pvalue_midp)
        for k in planes:
            planes[k][c] = w[k]
        sc = S.scores(w, w["pval"])
        counts[c], sums[c] = sc["counts"], sc["sums"]
    return dict(run_ptr=ptr, CHROM=w_chrom, START=w_start, END=w_end, planes=planes, counts=counts, sums=sums)


def clear_of_levels(pval, margin=1e-5):
    """Whether no p-value lies within `margin` relative of one of the four levels (then the counts below a level are exact under the
    1e-6 contract)."""
    p = pval[~np.isnan(pval)]
    return not any((np.abs(p / a - 1.0) <= margin).any() for a in S.LEVELS)


def same_bits(x, y):
    """Equal shapes and types and the same bits in every element; two NaNs are equal whatever their sign and payload (an invalid
    operation's NaN is -NaN on the host and +NaN on the device)."""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    if x.dtype.kind != "f":
        return bool(np.array_equal(x, y))
    both_nan = np.isnan(x) & np.isnan(y)
    return bool(np.array_equal(x.view(np.uint64)[~both_nan], y.view(np.uint64)[~both_nan]))
