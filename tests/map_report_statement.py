"""The map report's definitions (include/dig_hip.h: dig_map_windows, dig_map_scores) in plain numpy -- what the golden generator,
the CPU test and the GPU tests state the device's results against.  The p-value functions are handed in (the reference's own in the
generator, the test-side C implementation in the tests): nothing here computes a statistic.
"""
import numpy as np

LEVELS = (0.05, 0.01, 0.001, 0.0001)
CHUNK, LANES = 1024, 256                         # dig_map_scores: windows of a chunk, lanes of its workgroup


def run_ptr(chrom, start, step):
    """The runs of equal key (chrom, start // step) in grid order: (run_ptr int64 [M + 1], CHROM, START, END of the merged windows)."""
    chrom, start = np.asarray(chrom, np.int64), np.asarray(start, np.int64)
    g = start // int(step)
    n = len(chrom)
    head = np.ones(n, bool)
    head[1:] = (chrom[1:] != chrom[:-1]) | (g[1:] != g[:-1])
    first = np.flatnonzero(head)
    ptr = np.concatenate([first, [n]]).astype(np.int64)
    return ptr, chrom[first], g[first] * int(step), (g[first] + 1) * int(step)


def sequential_sum(x):
    """x[0] + x[1] + ... as sequential double additions from +0.0 (np.cumsum adds one element after the other)."""
    return np.float64(np.cumsum(np.concatenate([[0.0], np.asarray(x, np.float64)]))[-1])


def merge(mu, std, y, flag, ptr, drop_flagged):
    """One cohort's merged windows: dict(n_bins i32, y_true i64, y_pred f64, std f64) [M].  The sums restart at every run (a difference
    of one global cumulative sum would have other bits); a gated-out bin adds +0.0."""
    mu, std, y = np.asarray(mu, np.float64), np.asarray(std, np.float64), np.asarray(y, np.int64)
    gate = ~(np.asarray(flag) != 0) if drop_flagged else np.ones(len(mu), bool)
    M = len(ptr) - 1
    out = dict(n_bins=np.zeros(M, np.int32), y_true=np.zeros(M, np.int64), y_pred=np.zeros(M), std=np.zeros(M))
    var = std * std                                           # (rounded before it is added)
    with np.errstate(invalid="ignore"):
        for m in range(M):
            lo, hi = int(ptr[m]), int(ptr[m + 1])
            g = gate[lo:hi]
            out["n_bins"][m] = g.sum()
            out["y_true"][m] = y[lo:hi][g].sum()
            out["y_pred"][m] = sequential_sum(np.where(g, mu[lo:hi], 0.0))
            out["std"][m] = np.sqrt(sequential_sum(np.where(g, var[lo:hi], 0.0)))
    return out


def pvalues(w, tail, gamma, upper, side):
    """PVAL of merged windows w: NaN without a bin; else the upper mid-p ('upper') or the two-sided mid-p ('side') of y_true under
    (alpha, theta) = gamma(y_pred, std), p = 1 / (theta + 1).  gamma, upper, side: the functions to use (upper takes arrays, side one
    window at a time, as the reference's)."""
    M = len(w["n_bins"])
    pv = np.full(M, np.nan)
    with np.errstate(all="ignore"):
        alpha, theta = gamma(w["y_pred"], w["std"])
        p = 1.0 / (theta + 1.0)
        k = w["y_true"].astype(np.float64)
        has = w["n_bins"] > 0
        if tail == "upper":
            pv[has] = np.asarray(upper(k[has], alpha[has], p[has]), np.float64)
        else:
            pv[has] = [float(side(k[m], alpha[m], p[m])) for m in np.flatnonzero(has)]          # (numpy scalars: 1 / 0 is inf)
    return pv


def ordered_sum(terms):
    """The sum of one cohort's per-window terms [M] (+0.0 where a window does not count) in dig_map_scores' order: chunks of 1024; in a
    chunk lane t adds windows t, t + 256, t + 512, t + 768 from +0.0; the lane sums fold by halves; the chunk sums first to last."""
    terms = np.asarray(terms, np.float64)
    n_chunks = -(-len(terms) // CHUNK)
    padded = np.zeros(n_chunks * CHUNK)
    padded[:len(terms)] = terms
    total = np.float64(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(n_chunks):
            q = padded[c * CHUNK:(c + 1) * CHUNK].reshape(CHUNK // LANES, LANES)
            lane = np.zeros(LANES)
            for r in q:
                lane = lane + r
            w = LANES // 2
            while w:
                lane[:w] = lane[:w] + lane[w:2 * w]
                w //= 2
            total = total + lane[0]
    return np.float64(total)


def scores(w, pval):
    """One cohort's scores: dict(counts int64 [7] -- N_WINDOWS, N_TESTED, OBS_TOTAL, N_BELOW[4] --, sums f64 [4] -- EXP_TOTAL, Sxx, Syy,
    Sxy), as dig_map_scores returns them."""
    has = w["n_bins"] > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        n, obs = int(has.sum()), int(w["y_true"][has].sum())
        counts = [n, int((has & ~np.isnan(pval)).sum()), obs] + [int((has & (pval < a)).sum()) for a in LEVELS]
        e = ordered_sum(np.where(has, w["y_pred"], 0.0))
        mx, my = np.float64(obs) / np.float64(n), e / np.float64(n)
        dx, dy = w["y_true"].astype(np.float64) - mx, w["y_pred"] - my
        sums = [e] + [ordered_sum(np.where(has, t, 0.0)) for t in (dx * dx, dy * dy, dx * dy)]
    return dict(counts=np.array(counts, np.int64), sums=np.array(sums, np.float64))


def derived(counts, sums):
    """What the route forms on the host from one cohort's scores: dict(R2, FRAC [4], CALIB_SCORE).  R2 = Sxy^2 / (Sxx Syy), 0 where
    that is NaN (gp_trainer.py:23-25) or with fewer than two windows; FRAC_a = N_BELOW[a] / N_TESTED; CALIB_SCORE = sum (a - FRAC_a)^2
    (gp_tools.py:117-121)."""
    with np.errstate(all="ignore"):
        r2 = np.float64(sums[3]) * np.float64(sums[3]) / (np.float64(sums[1]) * np.float64(sums[2]))
        r2 = 0.0 if (np.isnan(r2) or counts[0] < 2) else float(r2)
        frac = np.asarray(counts[3:7], np.float64) / np.float64(counts[1])
        calib = float(sum((a - f) ** 2 for a, f in zip(LEVELS, frac)))
    return dict(R2=r2, FRAC=frac, CALIB_SCORE=calib)
