"""Maker of tests/golden/nb_routes_golden.npz: negative-binomial p-values at the switch points of csrc/dig_math.hpp, with an
80-digit reference (mpmath; the tests read only the .npz).

    python tests/golden/make_nb_routes_golden.py            # rewrites the fixture, byte for byte, from SEED

Reference (mp.dps = 80, at the exact doubles k, alpha, p that are stored):
  primary      exact summation of t_0 = p^alpha, t_{j+1} = t_j (alpha + j)(1 - p) / (j + 1).  S_k = sum_{j<k} t_j is a finite sum;
               an upper tail is 1 - S_k where that keeps fifty digits (>= 1e-25; the sum itself carries eighty) and otherwise the
               series anchored at pmf(k), continued until the term is below 1e-40 of the sum with a ratio below 1.  A row whose
               series needs more than TERM_CAP terms is dropped.  Stored per group: candidates (before anything is turned away:
               targets solve_p could not place, |k - mu| too small), rows turned away for the rounding of 1 - p (below), drawn (what
               went to the reference and stayed) and kept (drawn minus those over the term cap).
  cross-check  mp.betainc(regularized=True) + the loggamma pmf wherever mp.betainc converges (`checked` flag per row); it has
               to agree with the primary form to 1e-30 or the maker stops.
The side of nb_pvalue_exact / nb_pvalue_midp is decided with the double expression mu = alpha (1 - p) / p (nb_model.py); rows with
|k - mu| < 1e-9 mu are not drawn, nor are rows at which the rounding of 1 - p in the reference's own betainc(k + 1, alpha, 1 - p)
moves the value by more than 1e-9 (tiny p with alpha << 1: see main()).

Tables
  singles  k, alpha, p + five references (midp_upper = 0.5 pmf + P(X > k), geq = P(X >= k), exact, midp two-sided, pmf) +
           route / path labels.  Where the parameter transform of the fused kernels can reach the row, (alpha, p) ARE the doubles
           oracle.element_stats forms from the stored (mu, sigma) with pi = cj = 1, so one reference serves the elementwise entry
           points and the fused kernels; rows it cannot reach (p = 1, p ~ 2^-1022, means beyond 1e140) have mu = sigma = NaN.
  pairs    k1, k2 sharing (mu, sigma) -> (alpha, p), the upper mid-p reference of each count.
Labels
  path   what classify() says about the scalar upper mid-p dispatch of nb_midp_upper: the thresholds of dig_math.hpp applied to
         the inputs and to the reference value (PATHS; -1 where p is outside the recurrences' domain).
  route  groups 0..5 are the paths themselves; 6..9 are directed groups (quad pmf sources, quad direction, lower side, limits)
         whose rows keep the group they were drawn for.
  tail_terms / quad_blocks / quad_upper: double-precision emulations of the two convergence tests (terms of the scalar tail series
         in steps of 8, blocks of the quad series, its direction), used to place rows and to say in a failure what a row exercised.
"""
import os
import sys
import zipfile
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "nb_routes_golden.npz")
SEED = 4096
TERM_CAP = 200_000
MAX_BYTES = 571_160                      # the largest fixture committed before this one (coresident_parent_outputs.npz)
MIN_NORMAL = 2.2250738585072014e-308

ROUTES = ["fast_accepted", "fast_cancelled", "slow_recurrence", "tail_converged", "tail_nonconvergent", "recurrence_skipped",
          "quad_pmf_source", "quad_direction", "lower_side", "limits"]
PATHS = ROUTES[:6]
K_SMALL, K_RECUR, K_TAIL_MAX, DIRECT_MIN = 128, 2048, 4096, 1e-6          # kSmallK, kRecurK, kTailMax, kDirectMin


# ---- the thresholds of dig_math.hpp ---------------------------------------------------------------------------------------
def fast_lp0_min(kmax):
    return -400.0 if kmax <= 64 else -200.0


def lp0_of(alpha, p):
    with np.errstate(all="ignore"):
        return np.asarray(alpha, float) * np.log(np.asarray(p, float))


def classify(k, alpha, p, midp_upper, tail_terms):
    """Path of nb_midp_upper(k, alpha, p) from the inputs and the reference value; -1 outside MIN_NORMAL <= p < 1."""
    if not (MIN_NORMAL <= p < 1.0):
        return -1
    lp0 = float(lp0_of(alpha, p))
    if k <= K_SMALL and lp0 > fast_lp0_min(k):
        return 0 if midp_upper >= DIRECT_MIN else 1
    if k <= K_RECUR and lp0 > -500.0:
        if midp_upper >= (DIRECT_MIN if k <= 256 else 1e-4):
            return 2
        return 3 if (0 <= tail_terms <= K_TAIL_MAX and midp_upper > 1e-290) else 4
    return 5


def tail_terms_emulated(k, alpha, p, limit=2 * K_TAIL_MAX):
    """Terms (a multiple of 8) after which the scalar tail series of nb_midp_upper_slow2 passes its test
    term <= 2^-56 sum; -1 if not within `limit`."""
    alpha, p = float(alpha), float(p)
    x, j, term, total = 1.0 - p, float(k), 1.0, 0.0
    n = 0
    while n < limit:
        for _ in range(8):
            term *= (alpha + j) * x / (j + 1.0)
            j += 1.0
            total += term
        n += 8
        if term <= total * 2.0 ** -56:
            return n
    return -1


def quad_emulated(k, alpha, p, max_blocks=64):
    """(blocks, upper) of nb_midp_upper_quad's series: the number of 64-term blocks after which its bound closes the series
    (max_blocks + 1: it never does and the scalar routine takes over) and the direction it sums in."""
    k, alpha, p = float(k), float(alpha), float(p)
    x = 1.0 - p
    ax = alpha * x
    upper = (alpha + k) * x < k + 1.0
    base, V = 1.0, 0.0
    for blk in range(max_blocks):
        for m in range(64 * blk, 64 * blk + 64):
            if upper:
                j = k + m
                base *= (j * x + ax) / (j + 1.0)
            else:
                j = k - m
                base *= (j / ((j - 1.0) * x + ax)) if j >= 1.0 else 0.0
            V += base
        mn = 64.0 * (blk + 1)
        if upper:
            j = k + mn
            num, den = ((j * x + ax), j + 1.0) if alpha > 1.0 else (x, 1.0)
        else:
            j = k - mn
            num, den = (j, (j - 1.0) * x + ax) if j >= 1.0 else (0.0, 1.0)
        if num < den and base * num <= (0.5 + V) * 2.0 ** -54 * (den - num):
            return blk + 1, upper
    return max_blocks + 1, upper


# ---- the 80-digit reference -------------------------------------------------------------------------------------------------
def reference(row):
    """(k, alpha, p) -> None (dropped: series longer than TERM_CAP) or
    (midp_upper, geq, exact, midp, pmf, checked, leq = P(X <= k)) as doubles + flag."""
    import mpmath
    from mpmath import mp, mpf
    mp.dps = 80
    k, alpha, p = int(row[0]), float(row[1]), float(row[2])
    if p < 2.0 ** -180:
        mp.prec = 1400                    # 1 - p has to stay exact (p down to 2^-1022), with eighty digits to spare
    with np.errstate(all="ignore"):
        mu = float(np.float64(alpha) * (np.float64(1.0) - np.float64(p)) / np.float64(p))
    lower_side = k < mu
    if p == 1.0:
        pmf = mpf(1 if k == 0 else 0)
        gt, geq, S = mpf(0), pmf, mpf(0)
    else:
        a, pp = mpf(alpha), mpf(p)
        x = 1 - pp
        t = pp ** a
        S = mpf(0)
        for j in range(k):
            S += t
            t = t * (a + j) * x / (j + 1)
        pmf = t

        def series():
            term, j, total, n = pmf, k, mpf(0), 0
            while True:
                ratio = (a + j) * x / (j + 1)
                term = term * ratio
                j += 1
                n += 1
                total += term
                if ratio < 1 and term < total * mpf("1e-40"):
                    return total
                if n > TERM_CAP:
                    return None

        gt = 1 - S - pmf
        if gt < mpf("1e-25"):
            gt = series()
            if gt is None:
                return None
        geq = 1 - S
        if geq < mpf("1e-25"):
            geq = pmf + gt
    midp_upper = pmf / 2 + gt
    le = S + pmf

    def pv_rule(v):                       # nb_model.py: `if pval == 0: pval = pmf`, on the doubles
        return float(pmf) if float(v) == 0.0 else float(v)

    if lower_side:
        exact = float(le)
    elif k == 0:
        exact = float("nan")              # nb_model.py evaluates betainc(0, alpha, 1 - p) here: NaN in scipy, kept by the project
    else:
        exact = pv_rule(geq)
    midp = float(pmf / 2 + (S if k > 0 else 0)) if lower_side else float(midp_upper)
    checked = 0
    if p < 1.0:
        try:
            a, pp = mpf(alpha), mpf(p)
            x = 1 - pp
            lg = mpmath.loggamma
            pmf2 = mpmath.exp(lg(k + a) - lg(k + 1) - lg(a) + a * mpmath.log(pp) + k * mpmath.log(x))
            up2 = pmf2 / 2 + mpmath.betainc(k + 1, a, 0, x, regularized=True)
            le2 = mpmath.betainc(a, k + 1, 0, pp, regularized=True)
            checked = 1
        except Exception:                 # mp.betainc: NoConvergence and friends -- the check did not run
            checked = 0
        if checked:
            for what, v, w in (("midp_upper", midp_upper, up2), ("P(X <= k)", le, le2), ("pmf", pmf, pmf2)):
                if abs(v - w) > mpf("1e-30") * abs(v) and abs(v) > mpf("1e-2000"):
                    raise AssertionError("cross-check of %s failed at k=%d alpha=%r p=%r: %s vs %s" %
                                         (what, k, alpha, p, mpmath.nstr(v, 40), mpmath.nstr(w, 40)))
    return float(midp_upper), float(geq), exact, midp, float(pmf), checked, float(le)


# ---- drawing rows -----------------------------------------------------------------------------------------------------------
def oracle_module():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import dig_oracle
    return dig_oracle


def solve_p(k, alpha, target):
    """p with 0.5 pmf(k) + P(X > k) = target (scipy, bisection on the logit; good to place rows, not to judge them).
    Returns p and a mask of the rows where the target was reached within a factor of 3."""
    O = oracle_module()
    k, alpha, target = (np.asarray(v, float) for v in np.broadcast_arrays(k, alpha, target))
    lo, hi = np.full(k.shape, -700.0), np.full(k.shape, 36.0)
    with np.errstate(all="ignore"):
        for _ in range(90):
            mid = 0.5 * (lo + hi)
            v = O.nb_pvalue_greater_midp(k, alpha, 1.0 / (1.0 + np.exp(-mid)))
            big = v > target
            lo, hi = np.where(big, mid, lo), np.where(big, hi, mid)
        p = 1.0 / (1.0 + np.exp(-0.5 * (lo + hi)))
        v = O.nb_pvalue_greater_midp(k, alpha, p)
        ok = (p < 1.0) & (p >= MIN_NORMAL) & (np.abs(np.log10(v) - np.log10(target)) < 0.5)
    return p, ok


def loguniform(rng, lo, hi, n):
    return 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), n)


def with_edges(rng, edges, lo, hi, n):
    """n counts: the listed edges in turn, then random ones in [lo, hi]."""
    out = rng.integers(lo, hi + 1, n).astype(float)
    m = min(n, 3 * len(edges))
    out[:m] = np.resize(np.asarray(edges, float), m)
    return out


def near(rng, centre, n, rel=0.01):
    """n values within +-rel of centre, both sides."""
    return centre * (1.0 + rng.uniform(-rel, rel, n))


def draw_singles(rng):
    """group, k, alpha_target, p_target arrays + the number of candidates per group (rows solve_p could not place included)."""
    rows = []
    candidates = np.zeros(len(ROUTES), np.int32)          # per group, before any row is turned away

    def add(group, k, alpha, p, ok=None):
        k, alpha, p = (np.asarray(v, float) for v in np.broadcast_arrays(k, alpha, p))
        m = np.isfinite(alpha) & (alpha > 0) & (p > 0) & (p <= 1) if ok is None else ok
        candidates[group] += len(k)
        rows.append((np.full(int(m.sum()), group), k[m], alpha[m], p[m]))

    def at_lp0(lp0, alpha):
        with np.errstate(all="ignore"):
            return np.exp(lp0 / alpha)

    fast_edges = [0, 1, 2, 63, 64, 65, 127, 128]
    # -- 0 fast, accepted: value within a factor 2 of 1e-6 (both sides: the lower half lands in group 1), mid range, near 1
    for lo, hi, n in ((5e-7, 2e-6, 150), (1e-5, 0.9, 120), (0.9, 0.999999, 80)):
        k = with_edges(rng, fast_edges[1:], 1, 128, n)
        alpha = loguniform(rng, 1e-2, 300, n)
        p, ok = solve_p(k, alpha, loguniform(rng, lo, hi, n))
        add(0, k, alpha, p, ok)
    add(0, np.zeros(12), loguniform(rng, 1e-2, 100, 12), rng.uniform(0.01, 0.99, 12))
    # lp0 within 1 % of the fast minimum, both sides (the far side lands in group 2)
    k = with_edges(rng, [0, 1, 2, 63, 64], 0, 64, 80)
    alpha = loguniform(rng, 0.6, 1000, 80)
    add(0, k, alpha, at_lp0(near(rng, -400.0, 80), alpha))
    k = with_edges(rng, [65, 127, 128], 65, 128, 80)
    alpha = loguniform(rng, 0.3, 1000, 80)
    add(0, k, alpha, at_lp0(near(rng, -200.0, 80), alpha))
    # -- 1 fast, cancelled: values down through 1e-100, 1e-249, 1e-251, 1e-291
    n = 260
    k = with_edges(rng, [19, 20, 63, 64, 65, 127, 128], 1, 128, n)
    alpha = loguniform(rng, 1e-2, 100, n)
    tgt = loguniform(rng, 1e-295, 1e-6, n)
    tgt[:80] = np.resize([1e-100, 1e-249, 1e-251, 1e-291], 80) * rng.uniform(0.5, 2.0, 80)
    k[:80] = rng.integers(24, 129, 80)
    p, ok = solve_p(k, alpha, tgt)
    add(1, k, alpha, p, ok)
    # -- 2 slow recurrence: accepted values, lp0 around -500
    slow_edges = [129, 256, 257, 2047, 2048]
    n = 200
    k = with_edges(rng, slow_edges, 129, 2048, n)
    alpha = loguniform(rng, 0.05, 2000, n)
    tgt = np.where(k <= 256, loguniform(rng, 1e-6, 1, n), loguniform(rng, 1e-4, 1, n))
    p, ok = solve_p(k, alpha, tgt)
    add(2, k, alpha, p, ok)
    k = with_edges(rng, slow_edges, 129, 2048, 100)
    alpha = loguniform(rng, 30, 3000, 100)
    add(2, k, alpha, at_lp0(near(rng, -500.0, 100), alpha))
    # -- 3 tail series that converges: small values, 1e-6 .. 1e-4 above k = 256, and series of close to 4096 terms
    n = 160
    k = with_edges(rng, slow_edges, 129, 2048, n)
    alpha = loguniform(rng, 1.0, 2000, n)
    p, ok = solve_p(k, alpha, loguniform(rng, 1e-285, 1e-6, n))
    add(3, k, alpha, p, ok)
    n = 60
    k = with_edges(rng, [257, 2047, 2048], 257, 2048, n)
    alpha = loguniform(rng, 1.0, 2000, n)
    p, ok = solve_p(k, alpha, loguniform(rng, 1e-6, 1e-4, n))
    add(3, k, alpha, p, ok)
    n = 140                               # 39 / p terms to 2^-56: 3000 .. 4096 for p in 0.0095 .. 0.013 (longer ones land in group 4)
    add(3, rng.integers(1200, 2049, n), loguniform(rng, 0.05, 1.0, n), rng.uniform(0.0086, 0.014, n))
    # -- 4 tail series that cannot converge in 4096 terms: alpha <= 1, small p (92 / p terms for the reference)
    n = 70
    add(4, rng.integers(600, 2049, n), loguniform(rng, 1e-3, 0.3, n), rng.uniform(2e-3, 8e-3, n))
    # -- 5 recurrence skipped: k > 2048 or lp0 <= -500, both orientations of the continued fraction
    n = 200
    k = with_edges(rng, [2049, 4096, 4097, 5000], 2049, 5000, n)
    alpha = loguniform(rng, 0.05, 5000, n)
    tgt = np.where(rng.uniform(size=n) < 0.5, loguniform(rng, 1e-200, 1e-2, n), rng.uniform(0.01, 0.999, n))
    p, ok = solve_p(k, alpha, tgt)
    add(5, k, alpha, p, ok)
    n = 120
    alpha = loguniform(rng, 30, 1e4, n)
    p = at_lp0(rng.uniform(-700, -500, n), alpha)
    with np.errstate(all="ignore"):
        mean = alpha * (1 - p) / p
    k = np.clip(np.rint(np.minimum(mean, 4000) * rng.uniform(0.3, 2.5, n)), 0, 5000)
    add(5, k, alpha, p)
    # -- 6 quad pmf sources: k = 64 / 65 around lp0 = -690, k = 4096 / 4097, alpha around 4096
    n = 90
    alpha = loguniform(rng, 1.2, 2000, n)
    add(6, np.resize([64.0, 65.0], n), alpha, at_lp0(near(rng, -690.0, n), alpha))
    n = 60
    k = np.resize([4096.0, 4097.0], n)
    alpha = loguniform(rng, 0.5, 4000, n)
    p, ok = solve_p(k, alpha, np.where(rng.uniform(size=n) < 0.5, loguniform(rng, 1e-150, 1e-2, n), rng.uniform(0.01, 0.99, n)))
    add(6, k, alpha, p, ok)
    n = 90
    alpha = np.resize([4095.9, 4096.0, 4096.1, 4000.0, 4200.0], n)
    k = rng.integers(129, 4097, n).astype(float)
    p, ok = solve_p(k, alpha, np.where(rng.uniform(size=n) < 0.5, loguniform(rng, 1e-150, 1e-2, n), rng.uniform(0.01, 0.99, n)))
    add(6, k, alpha, p, ok)
    # -- 7 quad direction
    n = 120                               # (alpha + k) x within 1e-3 of k + 1, both sides (k > 128: the pass gets no pmf)
    k = rng.integers(129, 3000, n).astype(float)
    alpha = loguniform(rng, 2, 5000, n)
    delta = loguniform(rng, 1e-6, 1e-3, n) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    x = (k + 1) * (1 + delta) / (alpha + k)
    add(7, k, alpha, 1 - x, (x > 0) & (x < 1))
    n = 90                                # alpha around the switch of the convergence bound
    alpha = np.resize([1 - 1e-3, 1.0, 1 + 1e-3], n)
    k = np.where(np.arange(n) < 45, rng.integers(10, 129, n), rng.integers(129, 1000, n)).astype(float)
    p, ok = solve_p(k, alpha, np.where(np.arange(n) < 45, loguniform(rng, 1e-100, 1e-8, n), loguniform(rng, 1e-30, 0.5, n)))
    add(7, k, alpha, p, ok)
    n = 112                               # downward series ending at j = 0 (reached only below the fast minimum of lp0)
    k = np.resize([1, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 127, 128], n).astype(float)
    alpha = np.where(np.arange(n) < 56, rng.uniform(1.01, 3.0, n), loguniform(rng, 3, 1000, n))
    lp0 = np.where(k <= 64, rng.uniform(-650, -405, n), rng.uniform(-650, -202, n))
    add(7, k, alpha, at_lp0(lp0, alpha))
    n = 60                                # ... and from counts above the table, where the lower tail is not negligible
    alpha = loguniform(rng, 1.5, 3000, n)
    mean = loguniform(rng, 200, 3000, n)
    k = np.clip(np.rint(mean * rng.uniform(0.6, 0.98, n)), 129, 5000)
    add(7, k, alpha, alpha / (alpha + mean))
    n = 60                                # upward series of one or two blocks
    k = rng.integers(129, 1500, n).astype(float)
    alpha = loguniform(rng, 0.5, 500, n)
    add(7, k, alpha, rng.uniform(0.15, 0.9, n))
    n = 160                               # ... of 63 .. 64 blocks and beyond (39 / p terms: p around 0.0094)
    add(7, rng.integers(129, 1200, n), loguniform(rng, 0.02, 1.0, n), rng.uniform(0.0088, 0.0100, n))
    # -- 8 lower side
    n = 110                               # nb_exact_fast
    alpha = loguniform(rng, 0.1, 1000, n)
    mean = loguniform(rng, 1, 400, n)
    k = np.minimum(np.floor(mean * rng.uniform(0, 0.999, n)), 128)
    k[:8] = [0, 0, 1, 1, 0, 1, 0, 1]
    add(8, k, alpha, alpha / (alpha + mean))
    n = 90                                # nb_lower_cdf_small: lp0 between the fast minimum and -690
    k = with_edges(rng, [0, 1, 64, 65, 128], 0, 128, n)
    alpha = loguniform(rng, 150, 3000, n)
    lp0 = np.where(k <= 64, rng.uniform(-689, -401, n), rng.uniform(-689, -201, n))
    add(8, k, alpha, at_lp0(lp0, alpha))
    n = 60                                # general betainc: lp0 below -690
    alpha = loguniform(rng, 600, 5000, n)
    p = at_lp0(rng.uniform(-1500, -691, n), alpha)
    mean = alpha * (1 - p) / p
    k = np.clip(np.floor(mean * rng.uniform(0.55, 0.999, n)), 0, 5000)
    k[:12] = rng.integers(0, 129, 12)
    add(8, k, alpha, p)
    n = 120                               # general betainc: k > 128, both orientations of the continued fraction
    alpha = loguniform(rng, 0.5, 3000, n)
    mean = loguniform(rng, 150, 6000, n)
    k = np.clip(np.floor(mean * rng.uniform(0.2, 0.999, n)), 129, 5000)
    add(8, k, alpha, alpha / (alpha + mean), k < mean * 0.9995)
    n = 40                                # ... the narrow band below the mean where betainc(alpha, k + 1, p) takes 1 - I_{1-p}(k + 1, alpha)
    alpha = loguniform(rng, 200, 5000, n)
    k = np.floor(np.minimum(alpha * rng.uniform(0.1, 1.8, n), 5000))
    k = np.maximum(k, 129)
    lo, hi = (alpha + 1) / (alpha + k + 3), alpha / (alpha + k)
    add(8, k, alpha, lo + (hi - lo) * rng.uniform(0.05, 0.9, n), hi > lo)
    # -- 9 limits
    tiny = MIN_NORMAL
    lim = [(k, a, 1.0) for k in (0, 1, 5) for a in (1e-3, 4.0, 1e6)]
    lim += [(k, a, pp) for k in (0, 1, 10, 100, 129) for a in (0.1, 0.3, 0.5) for pp in (tiny, 2 * tiny)]    # (scipy raises at alpha = 0.6, k = 100)
    lim += [(k, a, 1.0 - 2.0 ** -53) for k in (0, 1, 2, 5, 15) for a in (1e-3, 1.0, 50.0, 1e6)]
    lam = loguniform(rng, 0.1, 100, 30)   # Poisson limit
    lim += [(float(rng.poisson(l) + i % 4), 1e6, 1e6 / (1e6 + l)) for i, l in enumerate(lam)]
    lim += [(float(k), 1e-3, 1.0 - e) for k in (0, 1, 2, 5) for e in (1e-3, 1e-6, 1e-9)]
    lim += [(3000.0, 4.0, 0.5), (1050.0, 4.0, 0.5), (1040.0, 4.0, 0.5), (900.0, 4.0, 0.5)]   # pv == 0 -> pmf; subnormal results
    lim = np.array(lim, float)
    add(9, lim[:, 0], lim[:, 1], lim[:, 2])
    return [np.concatenate([r[i] for r in rows]) for i in range(4)] + [candidates]


def through_transform(alpha_t, p_t, direct=False):
    """(mu, sigma, alpha, p): the doubles oracle.element_stats forms with pi = cj = 1 from mu = mean, sigma = mean / sqrt(alpha);
    rows the transform cannot reach, and the `direct` ones (limits: exact values of p), keep their targets and get mu = sigma = NaN."""
    O = oracle_module()
    with np.errstate(all="ignore"):
        mean = alpha_t * (1.0 - p_t) / p_t
        sigma = mean / np.sqrt(alpha_t)
        one = np.ones_like(mean)
        r = O.element_stats(mean, sigma, one, one, 0 * one, 0 * one, 0 * one, 1.0, 1.0)
        alpha, p = r["ALPHA"], 1 / (r["THETA"] * one + 1)
        ok = (mean > 1e-140) & (mean < 1e140) & np.isfinite(alpha) & (alpha > 0) & (p >= 1e-300) & (p < 1.0) & (p_t < 1.0)
        ok &= (np.abs(alpha / alpha_t - 1) < 1e-12) & ~np.asarray(direct)
    return np.where(ok, mean, np.nan), np.where(ok, sigma, np.nan), np.where(ok, alpha, alpha_t), np.where(ok, p, p_t)


def draw_pairs(rng):
    """k1, k2, alpha_target, p_target for the fused kernels (one recurrence per pair, limits taken from the larger count)."""
    rows = []

    def add(k1, k2, alpha, p, ok=None):
        k1, k2, alpha, p = (np.asarray(v, float) for v in np.broadcast_arrays(k1, k2, alpha, p))
        m = np.ones(k1.shape, bool) if ok is None else ok
        rows.append(np.stack([k1[m], k2[m], alpha[m], p[m]], axis=1))

    def both_orders(k1, k2, alpha, p, ok=None):
        add(k1, k2, alpha, p, ok)
        add(k2, k1, alpha, p, ok)

    n = 45                                # the three orderings, both accepted
    alpha = loguniform(rng, 0.05, 300, n)
    mean = loguniform(rng, 0.1, 60, n)
    k1 = np.minimum(rng.poisson(mean * rng.uniform(0.5, 2, n)), 128)
    k2 = np.where(np.arange(n) % 3 == 0, k1, np.where(np.arange(n) % 3 == 1, rng.binomial(k1, 0.7), np.minimum(k1 + rng.integers(1, 20, n), 128)))
    add(k1, k2, alpha, alpha / (alpha + mean))
    for ka, kb in ((128, 129), (64, 65), (0, 128), (10, 100), (10, 50), (128, 128), (64, 64), (65, 65)):
        for lp0 in (-20.0, -150.0, -199.0, -201.0, -250.0, -300.0, -399.0, -401.0, -450.0, -499.0, -501.0, -600.0):
            alpha = float(loguniform(rng, 3, 600, 1)[0])
            both_orders(ka, kb, alpha, np.exp(lp0 / alpha))
    n = 40                                # the edge pairs where the values are not 1: near the mean and above it
    alpha = loguniform(rng, 0.5, 300, n)
    for ka, kb in ((128, 129), (64, 65), (0, 128), (127, 128)):
        p, ok = solve_p(np.full(n, kb), alpha, loguniform(rng, 1e-12, 0.9, n))
        both_orders(np.full(n, ka), np.full(n, kb), alpha, p, ok)
    n = 50                                # one cancelled and the other accepted, both cancelled
    k2 = rng.integers(20, 129, n).astype(float)
    alpha = loguniform(rng, 0.05, 100, n)
    p, ok = solve_p(k2, alpha, loguniform(rng, 1e-120, 1e-7, n))
    both_orders(np.floor(k2 * rng.uniform(0.0, 0.3, n)), k2, alpha, p, ok)
    both_orders(k2 - rng.integers(0, 4, n), k2, alpha, p, ok)
    n = 40                                # one or both counts beyond the table
    k2 = rng.integers(129, 3000, n).astype(float)
    alpha = loguniform(rng, 0.5, 1000, n)
    p, ok = solve_p(k2, alpha, loguniform(rng, 1e-60, 0.9, n))
    both_orders(np.floor(k2 * rng.uniform(0.02, 1.0, n)), k2, alpha, p, ok)
    return np.concatenate(rows)


# ---- writing ----------------------------------------------------------------------------------------------------------------
def save_npz(path, arrays):
    """np.savez_compressed with fixed member dates, so that the file depends on its content alone."""
    import io
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    import multiprocessing
    rng = np.random.default_rng(SEED)
    group, k, alpha_t, p_t, candidates_per_group = draw_singles(rng)
    mu, sigma, alpha, p = through_transform(alpha_t, p_t, direct=group == 9)
    with np.errstate(all="ignore"):
        mean = alpha * (1 - p) / p
        keep = ~(np.abs(k - mean) < 1e-9 * mean) & (k <= 5000)
    group, k, mu, sigma, alpha, p = (v[keep] for v in (group, k, mu, sigma, alpha, p))
    pk1, pk2, pa_t, pp_t = draw_pairs(rng).T
    pair_placed = len(pk1)
    pmu, psigma, palpha, pp = through_transform(pa_t, pp_t)
    ok = np.isfinite(pmu)
    pk1, pk2, pmu, psigma, palpha, pp = (v[ok] for v in (pk1, pk2, pmu, psigma, palpha, pp))

    jobs = list(zip(k, alpha, p)) + list(zip(pk1, palpha, pp)) + list(zip(pk2, palpha, pp))
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        res = pool.map(reference, jobs, chunksize=8)
    n, m = len(k), len(pk1)
    single, r1, r2 = res[:n], res[n:n + m], res[n + m:]

    # The reference evaluates betainc(k + 1, alpha, 1 - p) with 1 - p ROUNDED: where p is tiny and p^alpha is not (alpha << 1), that
    # rounding moves the reference's own value (to 1.0 where the true tail is 0.54 at alpha = 0.02, p = 5e-17) while the recurrences,
    # which start from p^alpha, stay with the truth.  Such rows cannot meet both and are not drawn: the effect of the rounding
    # d = |fl(1 - p) - (1 - p)| (0 from p = 0.5 on) on the upper tail, d dI_x(k + 1, alpha)/dx = d pmf(k) (k + alpha) / p and never
    # more than P(X <= k), has to stay below 1e-9 of the value.
    def harmless(kk, aa, ppp, rr):
        out = np.ones(len(kk), bool)
        for i, r in enumerate(rr):
            if r is not None and ppp[i] < 1.0:
                d = float(abs(Fraction(1.0 - float(ppp[i])) - (1 - Fraction(float(ppp[i])))))
                out[i] = min(d * r[4] * (kk[i] + aa[i]) / ppp[i], r[6]) <= 1e-9 * r[0]
        return out

    fine = harmless(k, alpha, p, single)
    rounding_filtered_per_group = np.bincount(group[~fine].astype(int), minlength=len(ROUTES))
    single = [r for r, f in zip(single, fine) if f]
    group, k, mu, sigma, alpha, p = (v[fine] for v in (group, k, mu, sigma, alpha, p))
    pfine = harmless(pk1, palpha, pp, r1) & harmless(pk2, palpha, pp, r2)
    r1, r2 = [r for r, f in zip(r1, pfine) if f], [r for r, f in zip(r2, pfine) if f]
    pk1, pk2, pmu, psigma, palpha, pp = (v[pfine] for v in (pk1, pk2, pmu, psigma, palpha, pp))
    m = len(pk1)
    kept = np.array([r is not None for r in single])
    drawn_per_group = np.bincount(group.astype(int), minlength=len(ROUTES))
    kept_per_group = np.bincount(group[kept].astype(int), minlength=len(ROUTES))
    group, k, mu, sigma, alpha, p = (v[kept] for v in (group, k, mu, sigma, alpha, p))
    vals = np.array([r for r in single if r is not None], float)
    tail_terms = np.array([tail_terms_emulated(*r) if (MIN_NORMAL <= r[2] < 1 and r[0] <= K_RECUR) else -1 for r in zip(k, alpha, p)], np.int32)
    quad = [quad_emulated(*r) if MIN_NORMAL <= r[2] < 1 else (0, False) for r in zip(k, alpha, p)]
    path = np.array([classify(*r) for r in zip(k, alpha, p, vals[:, 0], tail_terms)], np.int32)
    route = np.where((group <= 5) & (path >= 0), path, group).astype(np.int32)
    order = np.argsort(route, kind="stable")

    pkept = np.array([a is not None and b is not None for a, b in zip(r1, r2)])
    pv1 = np.array([r[0] for r, g in zip(r1, pkept) if g], float)
    pv2 = np.array([r[0] for r, g in zip(r2, pkept) if g], float)
    pc = np.array([min(a[5], b[5]) for a, b, g in zip(r1, r2, pkept) if g], np.uint8)

    def pair_path(kk, vv):
        return np.array([classify(a, b, c, v, tail_terms_emulated(a, b, c) if a <= K_RECUR else -1)
                         for a, b, c, v in zip(kk[pkept], palpha[pkept], pp[pkept], vv)], np.int32)

    out = dict(
        seed=np.int64(SEED), route_names=np.array(ROUTES), path_names=np.array(PATHS),
        k=k[order], alpha=alpha[order], p=p[order], mu=mu[order], sigma=sigma[order],
        route=route[order], path=path[order], group=group[order].astype(np.int32), checked=vals[order, 5].astype(np.uint8),
        midp_upper=vals[order, 0], geq=vals[order, 1], exact=vals[order, 2], midp=vals[order, 3], pmf=vals[order, 4], leq=vals[order, 6],
        tail_terms=tail_terms[order], quad_blocks=np.array([q[0] for q in quad], np.int32)[order],
        quad_upper=np.array([q[1] for q in quad], np.uint8)[order],
        candidates_per_group=candidates_per_group, rounding_filtered_per_group=rounding_filtered_per_group.astype(np.int32),
        drawn_per_group=drawn_per_group.astype(np.int32), kept_per_group=kept_per_group.astype(np.int32),
        pair_placed=np.int32(pair_placed), pair_rounding_filtered=np.int32(int((~pfine).sum())),
        pair_k1=pk1[pkept], pair_k2=pk2[pkept], pair_mu=pmu[pkept], pair_sigma=psigma[pkept], pair_alpha=palpha[pkept],
        pair_p=pp[pkept], pair_midp_upper1=pv1, pair_midp_upper2=pv2, pair_checked=pc,
        pair_path1=pair_path(pk1, pv1), pair_path2=pair_path(pk2, pv2),
        pair_drawn=np.int32(m), pair_kept=np.int32(int(pkept.sum())))
    save_npz(OUT, out)
    size = os.path.getsize(OUT)
    print("%d single rows, %d pairs, %d bytes" % (len(order), int(pkept.sum()), size))
    for g, name in enumerate(ROUTES):
        print("  %-20s rows %4d   candidates %4d  turned away for the rounding of 1 - p %3d  drawn %4d  kept %4d   checked %4d" %
              (name, int((route == g).sum()), candidates_per_group[g], rounding_filtered_per_group[g], drawn_per_group[g],
               kept_per_group[g], int(vals[route == g, 5].sum())))
    assert size <= MAX_BYTES, "fixture larger than the largest one committed before it"


if __name__ == "__main__":
    main()
