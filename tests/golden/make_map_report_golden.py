"""Writes tests/golden/map_report_golden.npz: five maps on one small grid, and what the REAL reference functions make of them at five
scales -- gp_tools.merge_windows and calibration_score_by_pvals (sequence_model/gp_tools.py:125-160, :117-121),
nb_model.normal_params_to_gamma, nb_pvalue_greater_midp and nb_pvalue_midp, scipy.stats.pearsonr.

Run in the build container only (it needs the reference tree, DIG_REFERENCE, default /root/reference, scipy, pandas and matplotlib):

    python tests/golden/make_map_report_golden.py

* Stubs the reference's absent I/O-only dependencies as make_golden.py does (seaborn among them; matplotlib runs on the Agg backend)
  and imports the reference from its own location; nothing of it is copied.
* Grid: 599 bins of W = 10 000 on three chromosomes (233, 199 and 167 bins: none a multiple of 3 or 7), each with single missing
  bins and one gap of 30.
* Cohorts: 0 sparse (Y_PRED ~ Gamma(9, 3), STD ~ Gamma(4, 1), Y_TRUE drawn from the map's own negative binomial); 1 dense (x 300:
  its 100-bin windows hold 1e5 - 1e6 counts); 2 with planted hot windows (a large, sharp Y_PRED overshot by 20 - 85 %: p down to 1e-300); 3 with STD halved after the
  draw (miscalibrated); 4 with hostile bins: STD = 0, Y_PRED = 0, a negative and a NaN Y_PRED.  Every cohort carries FLAG bits; in
  cohort 1, 21 neighbouring bins that are whole windows at the scales 1, 3 and 7 are all flagged.
* Scales 1, 3, 7, 100 and 10^6 (a window is a whole chromosome), both gate settings (with drop_flagged the reference side is
  merge_windows on df[~FLAG] with the same idx_new), both tails.
* Stored per (scale, gate): run_ptr and the windows' coordinates; per cohort N_BINS and Y_TRUE (integers), the reference's Y_PRED and
  STD, its two p-values; per (scale, gate, tail, cohort) the scores: N_WINDOWS, N_TESTED, OBS_TOTAL, N_BELOW, EXP_TOTAL, R2 (NaN -> 0
  as gp_trainer.py:23-25), the fractions and CALIB_SCORE over the testable p-values.
* pandas' Series.sum() SKIPS a NaN; the contract's sums are IEEE additions, and "a NaN input" gives a NaN p-value.  So a window that
  holds a NaN Y_PRED bin (cohort 4 only) gets Y_PRED = NaN before the reference's p-value functions see it; `nan_input` marks these
  windows, whose stored Y_PRED is the contract's and not pandas'.
* Rules, asserted; the seed is redrawn until both hold: no reference p-value lies within 1e-5 relative of a level; every stored R2 of
  a cohort without a NaN (cohorts 0 - 3) has n >= 3 windows and R2 >= 0.05.
"""
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np

REF = os.environ.get("DIG_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "map_report_golden.npz")
sys.path.insert(0, os.path.dirname(HERE))

SEED0 = 20261021
W = 10_000
CHROM_BINS = (233, 199, 167)
SCALES = (1, 3, 7, 100, 10 ** 6)
LEVELS = (0.05, 0.01, 0.001, 0.0001)
MARGIN = 1e-5
C = 5


def install_stubs():
    for name in ["pysam", "pybedtools", "h5py", "statsmodels", "statsmodels.stats", "statsmodels.stats.multitest", "seaborn",
                 "bbi", "tables", "gpytorch", "tensorboardX", "pkg_resources"]:
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, REF)


def make_grid(rng):
    chrom, start = [], []
    for c, n in enumerate(CHROM_BINS, 1):
        slots = np.arange(n + 30 + 6)
        gap0 = int(rng.integers(40, n - 40))
        drop = set(range(gap0, gap0 + 30)) | set(int(v) for v in rng.choice(np.setdiff1d(slots, np.arange(gap0 - 1, gap0 + 31)), 6, replace=False))
        keep = np.array([s for s in slots if s not in drop], np.int64)
        assert len(keep) == n
        chrom.append(np.full(n, c, np.int64))
        start.append(keep * W)
    return np.concatenate(chrom), np.concatenate(start)


def make_cohorts(rng, chrom, start):
    N = len(chrom)
    mu = rng.gamma(9.0, 3.0, (C, N))
    sd = rng.gamma(4.0, 1.0, (C, N))
    mu[1] *= 300.0
    sd[1] *= 300.0
    y = rng.poisson(rng.gamma(mu ** 2 / sd ** 2, sd ** 2 / mu)).astype(np.int64)
    hot = rng.choice(N, 12, replace=False)                             # cohort 2: hot bins -- a large, sharp prediction that the
    mu[2, hot] *= 100.0                                                # count overshoots by 20 .. 85 % (z up to ~37: p down to 1e-300)
    sd[2, hot] = mu[2, hot] * 0.01
    y[2, hot] = (mu[2, hot] * np.concatenate([[1.85, 1.8, 1.7], rng.uniform(1.2, 1.6, 9)])).astype(np.int64)
    sd[3] *= 0.5
    flag = rng.uniform(size=(C, N)) < 0.06
    # cohort 1: 21 neighbouring bins that lie in one chromosome without a gap and start at a multiple of 21 W
    for i in range(N - 21):
        if start[i] % (21 * W) == 0 and chrom[i + 20] == chrom[i] and start[i + 20] - start[i] == 20 * W:
            flag[1, i:i + 21] = True
            all_flagged = i
            break
    else:
        raise AssertionError("no aligned stretch of 21 bins")
    bad = rng.choice(np.flatnonzero(~flag[4]), 8, replace=False)       # cohort 4: hostile bins, none of them flagged
    sd[4, bad[0:2]] = 0.0
    mu[4, bad[2:4]] = 0.0
    mu[4, bad[4:6]] = -mu[4, bad[4:6]]
    mu[4, bad[6:8]] = np.nan
    return mu, sd, y, flag, all_flagged


def near_level(p):
    p = p[~np.isnan(p)]
    return any((np.abs(p / a - 1.0) <= MARGIN).any() for a in LEVELS)


def build(seed, gp_tools, ref_nb, pearsonr, S):
    """The fixture's arrays for one seed, or the rule that refuses it (a string)."""
    import pandas as pd
    rng = np.random.default_rng(seed)
    chrom, start = make_grid(rng)
    mu, sd, y, flag, all_flagged = make_cohorts(rng, chrom, start)
    N = len(chrom)
    out = dict(chrom=chrom.astype(np.int32), start=start, window=np.int64(W), mu=mu, std=sd, y=y.astype(np.int32), flag=flag.astype(np.uint8),
               scales=np.array(SCALES, np.int64), all_flagged_bin=np.int64(all_flagged), seed=np.int64(seed))
    frames = [pd.DataFrame(dict(CHROM=chrom, START=start, END=start + W, Y_TRUE=y[c], Y_PRED=mu[c], STD=sd[c])) for c in range(C)]
    for si, s in enumerate(SCALES):
        ptr, w_chrom, w_start, w_end = S.run_ptr(chrom, start, s * W)
        M = len(ptr) - 1
        idx_new = np.column_stack([w_chrom, w_start, w_end])
        out["run_ptr_%d" % si] = ptr
        out["coords_%d" % si] = idx_new.astype(np.int64)
        for gate in (0, 1):
            key = "%d_%d" % (si, gate)
            n_bins, y_true, y_pred, std = np.zeros((C, M), np.int32), np.zeros((C, M), np.int64), np.zeros((C, M)), np.zeros((C, M))
            nan_input = np.zeros((C, M), bool)
            pv = np.full((2, C, M), np.nan)
            for c in range(C):
                keep = ~flag[c] if gate else np.ones(N, bool)
                merged = gp_tools.merge_windows(frames[c][keep], idx_new)
                n_bins[c] = np.add.reduceat(keep.astype(np.int64), ptr[:-1])
                y_true[c] = merged.Y_TRUE.values.astype(np.int64)
                y_pred[c], std[c] = merged.Y_PRED.values, merged.STD.values
                assert np.array_equal(y_true[c], np.add.reduceat(np.where(keep, y[c], 0), ptr[:-1]))
                nan_input[c] = np.add.reduceat((keep & np.isnan(mu[c])).astype(np.int64), ptr[:-1]) > 0
                y_pred[c, nan_input[c]] = np.nan
                has = n_bins[c] > 0
                with np.errstate(all="ignore"):
                    alpha, theta = ref_nb.normal_params_to_gamma(y_pred[c], std[c])
                    p = 1.0 / (theta + 1.0)
                    k = y_true[c].astype(np.float64)
                    pv[0, c, has] = ref_nb.nb_pvalue_greater_midp(k[has], alpha[has], p[has])
                    pv[1, c, has] = [float(ref_nb.nb_pvalue_midp(k[m], alpha[m], p[m])) for m in np.flatnonzero(has)]   # (numpy scalars: 1 / 0 is inf)
                if near_level(pv[:, c]):
                    return "a p-value of cohort %d at scale %d within %g of a level" % (c, s, MARGIN)
            out["n_bins_" + key], out["y_true_" + key], out["y_pred_" + key], out["std_" + key] = n_bins, y_true, y_pred, std
            out["nan_input_" + key], out["pval_" + key] = nan_input, pv
            counts = np.zeros((2, C, 7), np.int64)
            floats = np.zeros((2, C, 7))                               # EXP_TOTAL, R2, CALIB_SCORE, FRAC x 4
            for t in (0, 1):
                for c in range(C):
                    has = n_bins[c] > 0
                    p = pv[t, c][has]
                    ok = p[~np.isnan(p)]
                    counts[t, c] = [has.sum(), len(ok), y_true[c][has].sum()] + [int((ok < a).sum()) for a in LEVELS]
                    with np.errstate(all="ignore"):
                        r = pearsonr(y_true[c][has].astype(np.float64), y_pred[c][has])[0] if has.sum() >= 2 else 0.0
                    r2 = 0.0 if np.isnan(r) else float(r) ** 2
                    if c < 4 and not (has.sum() >= 3 and r2 >= 0.05):
                        return "R2 = %.3g over %d windows of cohort %d at scale %d, gate %d" % (r2, has.sum(), c, s, gate)
                    frac = [len(ok[ok < a]) / len(ok) for a in LEVELS]
                    floats[t, c] = [y_pred[c][has].sum(), r2, gp_tools.calibration_score_by_pvals(ok)] + frac
            out["counts_" + key], out["floats_" + key] = counts, floats
    return out


def main():
    install_stubs()
    from DIGDriver.sequence_model import gp_tools, nb_model as ref_nb      # noqa: E402
    from scipy.stats import pearsonr
    import map_report_statement as S
    for seed in range(SEED0, SEED0 + 40):
        out = build(seed, gp_tools, ref_nb, pearsonr, S)
        if not isinstance(out, str):
            break
        print("seed %d refused: %s" % (seed, out))
    else:
        raise AssertionError("no seed passes the rules")
    # the rules, asserted on what is stored
    for si in range(len(SCALES)):
        for gate in (0, 1):
            key = "%d_%d" % (si, gate)
            assert not near_level(out["pval_" + key])
            assert (out["counts_" + key][:, :4, 0] >= 3).all() and (out["floats_" + key][:, :4, 1] >= 0.05).all()
            assert out["nan_input_" + key][:4].sum() == 0 and out["nan_input_" + key][4].sum() > 0
    p1 = out["pval_0_0"][0]
    print("seed %d; windows per scale %s; smallest p at scale 1 %.3g; NaN p at scale 1 per cohort %s" % (
        out["seed"], [len(out["run_ptr_%d" % i]) - 1 for i in range(len(SCALES))], np.nanmin(np.where(p1 > 0, p1, np.nan)),
        np.isnan(p1).sum(axis=1).tolist()))
    print("zero p-values at scale 1: %d; Y_TRUE of cohort 1 at scale 100: %d .. %d" % (
        int((p1 == 0).sum()), out["y_true_3_0"][1].min(), out["y_true_3_0"][1].max()))
    assert (out["n_bins_1_1"][1] == 0).sum() >= 7 and (out["n_bins_2_1"][1] == 0).sum() >= 3      # the all-flagged stretch, scales 3 and 7
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
