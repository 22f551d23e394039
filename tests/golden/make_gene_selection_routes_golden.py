"""Maker of tests/golden/gene_selection_routes_golden.npz: the 34 planes of csrc/dig_genesel.hip where its formulas are
delicate, with an 80-digit reference (mpmath + numpy only; reads gene_selection_golden.npz and nb_routes_golden.npz for
inputs, nothing else), and a table for fisher_combine_fast around its switch at p1 p2 = 1e-290.

    python tests/golden/make_gene_selection_routes_golden.py     # rewrites the fixture, byte for byte, from SEED

Arithmetic.  restate() forms rate, tps, t_syn (alpha <= 1 branch, Python's max), mrfold, ex, ex_ml, p, sel, th0, lam, p0, p1
in numpy float64, one operation each, in the order the kernel documents.  T_SYN, MRFOLD, EXP_c_ML and SEL_c of it are the
expected values of the 14 arithmetic planes (stored: bit equality is asserted); the others are the exact doubles at which the
80-digit part starts -- the rounding of p0 = 1 / (1 + th0) is honoured by starting from that double, as the kernel does.  They
are not stored (at ~100 doubles a pair the file would hold 700 pairs): numpy's +, *, / are IEEE operations, the tests recompute
them with restate() and compare their checksums (`sum64_*`: the uint64 views summed) with what the maker saw.

Reference (mp.dps = 80), per pair and likelihood-ratio plane, from those doubles:
  class term  d = alpha (ln p0 - ln p1) + k (ln(1 - p0) - ln(1 - p1))  (k term absent at k = 0), or pois_llr = k (ln lam - ln k) - lam + k
  x = -2 d, or -2 (d1 + d2) for the df 2 tests;  sf1 = erfc(sqrt(x / 2)),  sf2 = exp(-x / 2),  x < 0 -> 1
  S = the sum of the magnitudes of the terms of x;  A = pdf(x) / sf(x) = -d ln sf / dx  (1/2 for df 2); stored as S and the
  product AS (float32, rounded up: A = AS / S alone overflows float32 as x -> 0, where AS ~ sqrt(x) is harmless)
so that an evaluation in doubles with a few ulp per term lands within  M 2^-53 (1 + A S)  of the reference.  At x = 0 exactly
(p0 and p1 the same double, or every term 0) the result is 1 in any arithmetic and A is stored as 0.  The six burden p-values
come from reference() of make_nb_routes_golden.py at the stored (k, alpha, p).

Pairs whose bound exceeds 1e-9 on a likelihood-ratio plane at M = 16 say nothing at this precision (x within rounding of 0,
where sf1 moves like sqrt(x)) and are not drawn; no group may lose more than 2 % of its candidates that way.  x is negative
only by rounding (the alternative is the maximum of the likelihood), so this also means that NO pair of this fixture reaches the
`x < 0 -> 1` branch of chi2_sf1 / chi2_sf2: the edge block of gene_selection_golden.npz is what covers it.  `check` [34, G, C]
marks what is asserted: 0 on a burden plane whose rounded p is exactly 1 (or whose series exceeds the term cap), and on a plane
whose 80-digit value lies within a factor 4 of 2^-1075, where rounding to 0 or to the smallest subnormal is a coin toss.

Pairs whose rounded p0, p1 are exactly 0 or 1 with a count above 0, or whose inputs are NaN, infinite or negative, stay with the
edge block of gene_selection_golden.npz: their result is IEEE sign logic, not precision.  Of gamma_ok only `t_syn > 0` and
`scale > 0` can fail with finite positive inputs (by underflow: two genes of the Gamma-Poisson group); `scale < inf` fails only
together with p = 0, and `t_syn == 0 && alpha == 1` only together with `scale == 0`.
"""
import importlib.util
import os
import sys
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "gene_selection_routes_golden.npz")
SEED = 20261018
C = 3
N_REGULAR_GENES = 150
BOUND_CAP = 1e-9
M_CAP = 16                     # the M at which the cap on uninformative pairs is applied (>= the M of DESIGN.md 5.2)
U = 2.0 ** -53

GROUPS = ["regular", "ratio_near_zero", "deep_tail", "small_theta_pi", "alpha_le_1", "mrfold_floor", "near_poisson",
          "gamma_poisson", "burden"]
CLASSES = ("SYN", "MIS", "NONS", "SPL", "TRUNC", "NONSYN")
PLANES = (("T_SYN", "MRFOLD") + tuple("EXP_%s_ML" % c for c in CLASSES) + tuple("PVAL_%s_BURDEN_DNDS" % c for c in CLASSES)
          + tuple("PVAL_%s_SEL_NB" % c for c in ("SYN", "MIS", "TRUNC", "NONSYN"))
          + tuple("PVAL_%s_SEL_PG" % c for c in ("SYN", "MIS", "NONS", "NONSYN"))
          + tuple("SEL_%s" % c for c in CLASSES) + tuple("PVAL_%s_SEL" % c for c in CLASSES))
ARITH = list(range(0, 8)) + list(range(22, 28))
BURDEN = list(range(8, 14))
LR = list(range(14, 22)) + list(range(28, 34))
DF2 = (17, 21)
SUMMED = ("p", "p0_nb", "p1_nb", "lam", "p0_sel", "p1_sel")


def _routes_maker():
    spec = importlib.util.spec_from_file_location("make_nb_routes_golden", os.path.join(HERE, "make_nb_routes_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules.setdefault(spec.name, mod)          # (multiprocessing pickles reference() by its module's name)
    spec.loader.exec_module(mod)
    return mod


def sum64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64).sum(dtype=np.uint64)


# ---- the kernel's formulas in numpy float64 ---------------------------------------------------------------------------------
def pymax(a, b):
    """Python's max(a, b): a unless b > a."""
    return np.where(b > a, b, a)


def _fl(fr):
    return float(fr)               # Fraction -> nearest double: one rounding


_erfc = np.frompyfunc(__import__("math").erfc, 1, 1)      # (the C library's: scipy.special.erfc returns 0 for subnormal results)


def restate(alpha, theta, pi, obs, mutant=None, erfc=None):
    """alpha, theta [G, C]; pi [G, 6, C]; obs [G, 5, C] -> dict of the intermediates and `planes` [34, G, C] (burden planes NaN:
    they are not restated here).  `mutant` names one deliberate error (tests/test_gene_selection_routes_fixture.py)."""
    erfc = erfc or _erfc
    alpha, theta, pi = (np.asarray(v, np.float64) for v in (alpha, theta, pi))
    G, Cc = alpha.shape
    if mutant == "pi_next_cohort":
        pi = pi[:, :, (np.arange(Cc) + 1) % Cc]
    ki = [np.asarray(obs)[:, q, :].astype(np.int64) for q in range(4)]
    ki.append(ki[2] + ki[3])
    ki.append(ki[1] + ki[4])
    k = [v.astype(np.float64) for v in ki]
    inf = np.inf
    with np.errstate(all="ignore"):
        rate = alpha * theta
        exp_syn = rate * pi[:, 0]
        tps = theta * pi[:, 0]
        num = (k[0] + alpha) - 1.0
        t_syn = num / (1.0 + 1.0 / tps)
        if mutant == "fma_t_syn":            # the quotient rounded once: 1 + 1 / tps kept exact
            ok = np.isfinite(tps) & (tps > 0) & np.isfinite(num)
            t_syn = t_syn.copy()
            for i in zip(*np.nonzero(ok)):
                t_syn[i] = _fl(Fraction(float(num[i])) / (1 + 1 / Fraction(float(tps[i]))))
        t_syn = np.where(alpha <= 1.0, pymax(alpha * tps, t_syn), t_syn)
        ratio = t_syn / exp_syn
        if mutant == "fmax_mrfold":
            mrfold = np.fmax(1e-10, ratio)
        elif mutant == "maximum_mrfold":
            mrfold = np.maximum(1e-10, ratio)
        else:
            mrfold = pymax(np.full_like(ratio, 1e-10), ratio)
        ex = np.stack([rate * pi[:, q] for q in range(6)])
        ex_ml = ex * mrfold
        if mutant == "fma_ex_ml":            # rate * pi * mrfold rounded once
            ok = np.isfinite(ex_ml) & (ex_ml != 0)
            ex_ml = ex_ml.copy()
            for i in zip(*np.nonzero(ok)):
                ex_ml[i] = _fl(Fraction(float(rate[i[1:]])) * Fraction(float(pi[i[1], i[0], i[2]])) * Fraction(float(mrfold[i[1:]])))
        tp = np.stack([theta * pi[:, q] for q in range(6)])
        p = 1.0 / (ex_ml / alpha + 1.0)
        kk = np.stack(k)
        den = ex + 1e-16
        if mutant == "fma_sel_denominator":   # fma(rate, Pi_c, 1e-16): the product not rounded before the sum
            den = den.copy()
            for i in zip(*np.nonzero(np.isfinite(den))):
                den[i] = _fl(Fraction(float(rate[i[1:]])) * Fraction(float(pi[i[1], i[0], i[2]])) + Fraction(1e-16))
        sel = (kk + 1e-16) / den

        def fin(v):
            return (v >= 0.0) & (v < inf)

        def nb_llr(kq, th0, th1):
            p0, p1 = 1.0 / (1.0 + th0), 1.0 / (1.0 + th1)
            l0 = -np.log1p(th0) if mutant == "log1p_theta" else np.log(p0)
            d = alpha * (l0 - np.log(p1))
            d = np.where(kq != 0.0, d + kq * (np.log1p(-p0) - np.log1p(-p1)), d)
            return np.where((alpha > 0) & fin(alpha) & fin(th0) & fin(th1), d, np.nan), p0, p1

        def sf1(x):
            neg = (x <= 0.0) if mutant == "x_le_0" else (x < 0.0)
            e = erfc(np.sqrt(0.5 * np.where(neg | np.isnan(x), 0.0, x))).astype(np.float64)
            if mutant == "erfc_1e-9":
                e = e * (1.0 + 1e-9)
            return np.where(np.isnan(x), np.nan, np.where(neg, 1.0, e))

        def sf2(x):
            neg = (x <= 0.0) if mutant == "x_le_0" else (x < 0.0)
            return np.where(np.isnan(x), np.nan, np.where(neg, 1.0, np.exp(-0.5 * np.where(neg, 0.0, x))))

        def tests(d, z, ok):
            bad = np.isnan(d[0]) | np.isnan(d[1]) | np.isnan(d[2]) | ~ok
            nan = lambda m, v: np.where(m, np.nan, v)
            return [nan(bad | z[1] | z[2], sf1(-2.0 * d[0])), nan(bad | z[0] | z[2], sf1(-2.0 * d[1])),
                    nan(bad | z[0] | z[1], sf1(-2.0 * d[2])), nan(bad | z[0], sf2(-2.0 * (d[1] + d[2])))]

        d_sel, p0_sel, p1_sel = nb_llr(kk, tp, tp * sel)
        pv_sel = sf1(-2.0 * d_sel)
        qs = (0, 1, 4)
        th0 = np.stack([(theta * pi[:, q]) * mrfold for q in qs])
        knb = np.stack([k[q] for q in qs])
        d_nb, p0_nb, p1_nb = nb_llr(knb, th0, knb / alpha)
        z_nb = (knb > 0.0) & (th0 == 0.0)
        lam = np.stack([(rate * pi[:, s]) * mrfold for s in range(3)])
        kpg = np.stack(k[:3])
        kt = np.where(kpg == 0.0, 0.0, kpg * (np.log(lam) - np.log(np.where(kpg == 0.0, 1.0, kpg))))
        d_pg = np.where(fin(lam), kt - lam + kpg, np.nan)
        z_pg = (kpg > 0.0) & (lam == 0.0)
        scale = tps * mrfold
        gamma_ok = ((alpha > 0) & (alpha < inf) & (scale > 0) & (scale < inf) &
                    (((t_syn > 0) & (t_syn < inf)) | ((t_syn == 0) & (alpha == 1.0))))
        pv_nb = tests(d_nb, z_nb, np.ones_like(gamma_ok))
        pv_pg = tests(d_pg, z_pg, gamma_ok)
    planes = np.full((34, G, Cc), np.nan)
    planes[0], planes[1] = t_syn, mrfold
    planes[2:8], planes[22:28], planes[28:34] = ex_ml, sel, pv_sel
    planes[14:18], planes[18:22] = np.stack(pv_nb), np.stack(pv_pg)
    return dict(planes=planes, k=kk, rate=rate, tps=tps, t_syn=t_syn, mrfold=mrfold, ex=ex, ex_ml=ex_ml, p=p, sel=sel, tp=tp,
                th0=th0, lam=lam, p0_nb=p0_nb, p1_nb=p1_nb, p0_sel=p0_sel, p1_sel=p1_sel, gamma_ok=gamma_ok, z_nb=z_nb, z_pg=z_pg,
                k_nb=knb, k_pg=kpg)


def fisher_restate(p1, p2):
    """fisher_combine_fast of dig_math.hpp in numpy."""
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    with np.errstate(all="ignore"):
        q = p1 * p2
        fast = (q > 1e-290) & (p1 <= 1.0) & (p2 <= 1.0)
        direct = q * (1.0 - np.log(np.where(fast, q, 1.0)))
        h = -(np.log(p1) + np.log(p2))
        slow = np.where(np.isnan(h), np.nan, np.where(h < 0, 1.0, np.where(np.isinf(h), 0.0, np.exp(np.log1p(np.where(h < 0, 0.0, h)) - h))))
    return np.where(fast, direct, slow)


# ---- the 80-digit part ----------------------------------------------------------------------------------------------------
def _nb_term(mp, alpha, k, p0, p1):
    """(d, sum of |terms|) of one class from the doubles; None where the kernel's argument check gives NaN."""
    a, P0, P1 = mp.mpf(alpha), mp.mpf(p0), mp.mpf(p1)
    t = [a * mp.log(P0), -a * mp.log(P1)]
    if k != 0:
        t += [k * mp.log(1 - P0), -k * mp.log(1 - P1)]
    return sum(t), sum(abs(v) for v in t)


def _pois_term(mp, k, lam):
    L = mp.mpf(lam)
    t = [-L]
    if k != 0:
        t += [k * mp.log(L), -k * mp.log(mp.mpf(k)), mp.mpf(k)]
    return sum(t), sum(abs(v) for v in t)


def _sf(mp, x, S2, df):
    """(want, A, S, near_flip) from x = -2 d and S2 = 2 sum |terms|."""
    if x == 0:
        return 1.0, 0.0, float(S2), False
    if x < 0:
        return 1.0, float("inf"), float(S2), False
    if df == 1:
        v = mp.erfc(mp.sqrt(x / 2))
        A = mp.exp(-x / 2) / mp.sqrt(2 * mp.pi * x) / v
    else:
        v = mp.exp(-x / 2)
        A = mp.mpf(0.5)
    tiny = mp.mpf(2) ** -1075
    flip = tiny / 4 < v < tiny * 4
    return float(v), float(A), float(S2), bool(flip)


def lr_reference(job):
    """One pair: (alpha, nb (k, p0, p1) x 3, nb_nan, pg (k, lam) x 3, pg_nan, sel (k, p0, p1) x 6) ->
    14 x (want, A, S, flip) in the order of LR."""
    from mpmath import mp
    mp.dps = 80
    alpha, nb, nb_nan, pg, pg_nan, sel = job
    nan = (float("nan"), 0.0, 0.0, False)
    out = []
    if nb_nan:
        out += [nan] * 4
    else:
        t = [_nb_term(mp, alpha, *r) for r in nb]
        out += [_sf(mp, -2 * d, 2 * s, 1) for d, s in t]
        out.append(_sf(mp, -2 * (t[1][0] + t[2][0]), 2 * (t[1][1] + t[2][1]), 2))
    if pg_nan:
        out += [nan] * 4
    else:
        t = [_pois_term(mp, *r) for r in pg]
        out += [_sf(mp, -2 * d, 2 * s, 1) for d, s in t]
        out.append(_sf(mp, -2 * (t[1][0] + t[2][0]), 2 * (t[1][1] + t[2][1]), 2))
    for r in sel:
        d, s = _nb_term(mp, alpha, *r)
        out.append(_sf(mp, -2 * d, 2 * s, 1))
    return out


def fisher_reference(row):
    from mpmath import mp
    mp.dps = 80
    p1, p2 = row
    if np.isnan(p1) or np.isnan(p2) or p1 < 0 or p2 < 0:
        return float("nan"), 0.0
    if p1 == 0 or p2 == 0:
        return 0.0, float("inf")
    h = -(mp.log(mp.mpf(p1)) + mp.log(mp.mpf(p2)))
    if h < 0:
        return 1.0, 0.0
    return float(mp.exp(-h) * (1 + h)), float(h)


# ---- the bound --------------------------------------------------------------------------------------------------------------
TINY = 2.2250738585072014e-308
SUB = 4.0 * 2.0 ** -1074


def ratios(got, want, AS):
    """|got / want - 1| in units of 2^-53 (1 + A S); subnormal references get 4 x 2^-1074 absolute on top; 0 -> 0 exactly
    (inf otherwise); NaN positions must match (inf otherwise).  Same shape as want."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(all="ignore"):
        unit = U * (1.0 + np.asarray(AS, np.float64))
        err = np.abs(got - want)
        err = np.where((want < TINY) & (want > 0), np.maximum(err - SUB, 0.0), err)
        r = err / np.abs(want) / unit
    r = np.where(want == 0, np.where(got == 0, 0.0, np.inf), r)
    r = np.where(np.isnan(want), np.where(np.isnan(got), 0.0, np.inf), r)
    return np.where(np.isnan(got) & ~np.isnan(want), np.inf, r)


# ---- drawing pairs ----------------------------------------------------------------------------------------------------------
def loguniform(rng, lo, hi, n):
    return 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), n)


class Pairs:
    def __init__(self):
        self.rows, self.group = [], []

    def add(self, group, alpha, theta, pi4, obs4, pi56=None):
        pi4 = [float(v) for v in pi4]
        p4 = pi4[2] + pi4[3]
        pi = pi4 + ([p4, pi4[1] + p4] if pi56 is None else [float(v) for v in pi56])
        self.rows.append([float(alpha), float(theta)] + pi + [float(int(v)) for v in obs4])
        self.group.append(GROUPS.index(group))

    def with_expectations(self, group, alpha, tps, k0, E, obs, pi0=0.03, pi56=None):
        """A pair whose EXP_c_ML for MIS, NONS, SPL come out at E (up to rounding): EXP_c_ML = EXP_SYN_ML Pi_c / Pi_SYN."""
        theta = tps / pi0
        t = ((k0 + alpha) - 1.0) / (1.0 + 1.0 / tps)
        if alpha <= 1.0:
            t = max(alpha * tps, t)
        m = max(1e-10, t / (alpha * theta * pi0))
        exp_syn_ml = alpha * theta * pi0 * m
        self.add(group, alpha, theta, [pi0] + [pi0 * e / exp_syn_ml for e in E], [k0] + list(obs), pi56)


def x_nb(k, alpha, E):
    """-2 (ll0 - ll1) of the NB test in doubles, for placing rows."""
    k, alpha, E = float(k), float(alpha), float(E)
    return 2.0 * (k * np.log(k / E) - (k + alpha) * np.log((alpha + k) / (alpha + E)))


def solve_E(k, alpha, x_target):
    """E < k with x_nb(k, alpha, E) = x_target (bisection on log E); None if out of reach."""
    lo, hi = np.log(1e-280), np.log(k)
    if x_nb(k, alpha, np.exp(lo)) < x_target:
        return None
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if x_nb(k, alpha, np.exp(mid)) > x_target:
            lo = mid
        else:
            hi = mid
    return float(np.exp(0.5 * (lo + hi)))


def draw(rng):
    P = Pairs()
    # -- regular: the first genes of gene_selection_golden.npz (hot genes included), Pi perturbed per cohort
    g = np.load(os.path.join(HERE, "gene_selection_golden.npz"), allow_pickle=False)
    assert int(g["n_regular"]) >= N_REGULAR_GENES
    for i in range(N_REGULAR_GENES):
        for c in range(C):
            pi4 = g["pi"][i, :4] * (1.0 + 0.2 * rng.uniform(-1, 1, 4))
            P.add("regular", g["alpha"][i, c], g["theta"][i, c], pi4, g["obs"][i, :4, c])
    # -- ratio near zero: counts at, one below and one above the expectation; the expectation off an integer by 0.3 .. 0.003
    for alpha in (0.05, 0.3, 1.7, 9.0, 60.0, 400.0, 3e3, 2e4, 1.5e5, 1e6):
        for off in (0.3, -0.3, 0.03, -0.03, 0.003):
            for dk in (-1, 0, 1):
                n = rng.integers(2, 40 if abs(off) > 0.01 else 12, 3)
                k0 = int(rng.integers(1, 12))
                P.with_expectations("ratio_near_zero", alpha, float(loguniform(rng, 0.1, 10, 1)[0]), k0, n + off, n + dk)
    for i in range(12):                     # x = 0 exactly: EXP_c = OBS_c in binary (SEL_c = 1, th1 = th0)
        k = int(rng.integers(1, 50))
        P.add("ratio_near_zero", 2.0 * k, 1.0, [0.5, 0.5, 0.25, 0.25], [k, k, k // 2 + 1, k // 3], pi56=None)
    # -- deep tail: MIS or NONS with k up to 9000 far above its expectation, placed by the df 1 NB value
    targets = [100, 249, 251, 300, 309, 316, 322, 330, 400]                  # -log10 of the p-value aimed at
    for i in range(90):
        k = int(rng.integers(300, 9001)) if i % 3 else 9000
        alpha = float(loguniform(rng, 0.5, 500, 1)[0])
        xt = 2.0 * (targets[i % len(targets)] * np.log(10.0) - np.log(float(rng.uniform(0.5, 2.0))))
        xt = xt - np.log(np.pi * xt / 2.0) if (i // len(targets)) % 2 == 0 else xt        # df 1 (asymptotic) or df 2
        E = solve_E(k, alpha, xt)
        if E is None:
            continue
        small = rng.uniform(0.5, 4.0, 2)
        cls = i % 2
        Es = [E, small[0], small[1]] if cls == 0 else [small[0], E, small[1]]
        obs = [k, rng.poisson(small[0]), rng.poisson(small[1])] if cls == 0 else [rng.poisson(small[0]), k, rng.poisson(small[1])]
        P.with_expectations("deep_tail", alpha, float(loguniform(rng, 0.1, 10, 1)[0]), int(rng.integers(0, 8)), Es, obs)
    # -- small theta Pi: 1e-3 .. 1e-15
    for i in range(90):
        alpha = float(loguniform(rng, 0.3, 300, 1)[0])
        tp = loguniform(rng, 1e-15, 1e-3, 4)
        if i % 3 == 0:
            tp[:] = 10.0 ** -(3 + i % 13)
        theta = float(loguniform(rng, 0.5, 20, 1)[0])
        P.add("small_theta_pi", alpha, theta, tp / theta, rng.integers(0, 4, 4))
    # -- alpha at or below 1, both sides of the max: alpha tps > k0 - 1
    for alpha in (0.25, 1.0 - 2.0 ** -53, 1.0, 1.0 + 2.0 ** -52, 1.5):
        for k0 in (0, 1, 5, 40):
            for f in (0.5, 0.999, 1.001, 2.0):
                tps = f * max(k0 - 1, 1) / alpha
                E = rng.uniform(0.5, 6.0, 3)
                P.with_expectations("alpha_le_1", alpha, tps, k0, E, rng.poisson(E))
    # -- MRFOLD on its floor 1e-10 and within 1e-3 of it: t_syn / exp_syn = (k0 + alpha - 1) / (alpha (1 + tps))
    for i in range(72):
        alpha = float(loguniform(rng, 1.2, 50, 1)[0])
        k0 = int(rng.integers(0, 6))
        edge = 1e10 * (k0 + alpha - 1.0) / alpha
        f = [1e-3, -1e-3, 1e-4, -1e-4, 1e-6, -1e-6, 0.5, 30.0][i % 8]
        tps = edge * (1.0 + f) if abs(f) < 0.1 else edge * (1.0 + f) * 2.0
        E = rng.uniform(0.5, 6.0, 3)
        P.with_expectations("mrfold_floor", alpha, tps, k0, E, rng.poisson(E))
    # -- near-Poisson genes
    for i in range(72):
        alpha = float(loguniform(rng, 300, 1e6, 1)[0])
        E = loguniform(rng, 0.05, 30, 3)
        P.with_expectations("near_poisson", alpha, float(loguniform(rng, 1e-4, 0.05, 1)[0]), int(rng.poisson(3)), E,
                            rng.poisson(E) + (i % 3 == 0) * rng.integers(0, 4, 3))
    # -- Gamma-Poisson: lam tiny and huge, k = 0 and k > 0; the two clauses of gamma_ok that finite positive inputs can fail
    for i in range(78):
        alpha = float(loguniform(rng, 0.4, 200, 1)[0])
        kind = i % 6
        if kind < 3:                         # tiny lam (with a count above 0 only while 1 / (1 + lam / alpha) stays below 1)
            E = loguniform(rng, 1e-300, 1e-6, 3) if kind == 0 else loguniform(rng, 1e-12 * alpha, 1e-6 * max(alpha, 1.0), 3)
            obs = [0, 0, 0] if kind == 0 else rng.integers(0, 3, 3)
        else:                                # huge lam
            E = loguniform(rng, 50, 3000, 3)
            obs = [0, 0, 0] if kind == 3 else np.maximum(rng.poisson(E) + rng.integers(-60, 60, 3), 0)
        P.with_expectations("gamma_poisson", alpha, float(loguniform(rng, 0.1, 10, 1)[0]), int(rng.integers(0, 9)), E, obs)
    for c in range(C):                       # t_syn = 0 with alpha != 1: alpha tps underflows
        P.add("gamma_poisson", 1e-200, 1e-150 * (1 + c), [0.03, 0.09, 0.004, 0.002], [0, 0, 0, 0])
    for c in range(C):                       # t_syn = 0 with alpha = 1, and scale = 0: theta Pi_SYN underflows
        P.add("gamma_poisson", 1.0, 1e-200 * (1 + c), [1e-200, 0.09, 0.004, 0.002], [0, 0, 0, 0])
    # -- burden: (k, alpha, p) of nb_routes_golden.npz at the thresholds of the dispatch, as the MIS class
    r = np.load(os.path.join(HERE, "nb_routes_golden.npz"), allow_pickle=False)
    k, a, p, v = r["k"], r["alpha"], r["p"], r["midp_upper"]
    with np.errstate(all="ignore"):
        lp0 = a * np.log(p)
    usable = (p > 1e-12) & (p < 1 - 1e-9) & (a > 1e-2) & (a < 1e5)
    picks = []
    for kk in (0, 1, 64, 65, 128, 129, 2048, 2049, 5000):
        picks += list(np.flatnonzero(usable & (k == kk))[:6])
    for centre in (-200.0, -400.0, -500.0):
        for side in (1, -1):
            m = usable & (np.abs(lp0 / centre - 1) < 0.01) & ((lp0 - centre) * side > 0)
            picks += list(np.flatnonzero(m)[:10])
    for side in (1, -1):
        m = usable & (v > 5e-7) & (v < 2e-6) & ((v - 1e-6) * side > 0)
        picks += list(np.flatnonzero(m)[:12])
    picks = picks[:len(picks) - len(picks) % C]
    for i in picks:
        E_mis = a[i] * (1.0 - p[i]) / p[i]
        small = rng.uniform(0.5, 4.0, 2)
        P.with_expectations("burden", a[i], float(loguniform(rng, 0.1, 10, 1)[0]), int(rng.integers(0, 8)),
                            [E_mis, small[0], small[1]], [k[i], rng.poisson(small[0]), rng.poisson(small[1])])
    return np.array(P.rows), np.array(P.group, np.int32)


def to_inputs(rows):
    """[N, 12] pairs -> alpha, theta [G, C], pi [G, 6, C], obs [G, 5, C]."""
    G = len(rows) // C
    r = rows.reshape(G, C, 12)
    obs = np.zeros((G, 5, C), np.int32)
    obs[:, :4, :] = r[:, :, 8:12].transpose(0, 2, 1).astype(np.int32)
    return r[:, :, 0].copy(), r[:, :, 1].copy(), np.ascontiguousarray(r[:, :, 2:8].transpose(0, 2, 1)), obs


def fisher_rows(rng):
    rows = []
    up, dn = np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0)
    for f in (0.5, 0.7, 0.99, 0.9999, 1.0001, 1.01, 1.4, 2.0):            # p1 p2 = f 1e-290
        q = f * 1e-290
        rows += [(np.sqrt(q), np.sqrt(q)), (q, 1.0), (1.0, q), (q / 0.37, 0.37), (1e-3, q / 1e-3), (q / 1e-250, 1e-250), (dn, q)]
    rows += [(1.0, 1.0), (1.0, 0.3), (0.3, 1.0), (1.0, 1e-300), (dn, dn), (up, 0.5), (0.5, up), (up, 1e-300), (up, up), (up, 1.0)]
    sub = 5e-324
    rows += [(0.0, 0.5), (0.5, 0.0), (0.0, 0.0), (sub, 1.0), (sub, 0.5), (1e-310, 1e-3), (sub, sub), (1e-320, 1e-320),
             (np.nan, 0.5), (0.5, np.nan), (np.nan, 0.0)]
    rows += [(1e-200, 1e-200), (1e-160, 1e-170), (1e-300, 1e-10), (1e-308, 1e-308)]                 # the product underflows
    for e in (295, 300, 303, 305, 306, 307, 308, 310, 312, 315, 318, 320, 322, 323, 324, 326, 330):  # results down to 0
        v = 10.0 ** -(e / 2.0 + 1.4)
        rows += [(v, v * float(rng.uniform(0.5, 2)))]
    p = loguniform(rng, 1e-150, 1.0, 60)
    rows += list(zip(p, loguniform(rng, 1e-150, 1.0, 60)))
    return np.array(rows, np.float64)


def pow2_ceil(v):
    return float(2.0 ** np.ceil(np.log2(v)))


def main():
    import multiprocessing
    routes = _routes_maker()
    rng = np.random.default_rng(SEED)
    rows, group = draw(rng)
    n = len(rows) - len(rows) % C
    rows, group = rows[:n], group[:n]
    candidates = np.bincount(group, minlength=len(GROUPS))
    alpha, theta, pi, obs = to_inputs(rows)
    R = restate(alpha, theta, pi, obs)
    G = alpha.shape[0]
    jobs = []
    for g in range(G):
        for c in range(C):
            f = lambda a, *i: float(a[i + (g, c)])
            jobs.append((float(alpha[g, c]),
                         [(f(R["k_nb"], s), f(R["p0_nb"], s), f(R["p1_nb"], s)) for s in range(3)],
                         bool(np.isnan(R["planes"][14:18, g, c]).all()),
                         [(f(R["k_pg"], s), f(R["lam"], s)) for s in range(3)],
                         bool(np.isnan(R["planes"][18:22, g, c]).all()),
                         [(f(R["k"], q), f(R["p0_sel"], q), f(R["p1_sel"], q)) for q in range(6)]))
    # what the maker does not draw: a count above 0 with a rounded p0 or p1 of exactly 0 or 1 (IEEE sign logic)
    for j, job in enumerate(jobs):
        for kq, p0, p1 in job[1] + job[5]:
            assert 0.0 < p0 <= 1.0 and 0.0 < p1 <= 1.0 and (kq == 0 or (p0 < 1.0 and p1 < 1.0)), (GROUPS[group[j]], j, kq, p0, p1)
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        ref = pool.map(lr_reference, jobs, chunksize=8)
    want_lr = np.array([[r[0] for r in row] for row in ref]).T            # [14, N]
    A = np.array([[r[1] for r in row] for row in ref]).T
    S = np.array([[r[2] for r in row] for row in ref]).T
    flip = np.array([[r[3] for r in row] for row in ref]).T
    with np.errstate(all="ignore"):
        bound = M_CAP * U * (1.0 + A * S)
        # a reference of 0 (80-digit value below 2^-1077) stays 0 while x moves by less than 1: nothing relative to bound
        bound = np.where((want_lr == 0) & ~flip & (M_CAP * U * S < 1.0), 0.0, bound)
    informative = ~(bound > BOUND_CAP).any(axis=0)                          # per pair
    if os.environ.get("DIG_MAKER_VERBOSE"):
        for j in np.flatnonzero(~informative):
            q = int(np.argmax(bound[:, j]))
            print("not drawn:", GROUPS[group[j]], PLANES[LR[q]], "bound %.3g A %.3g S %.3g" % (bound[q, j], A[q, j], S[q, j]), rows[j])
    drawn = np.bincount(group[informative], minlength=len(GROUPS))
    lost = candidates - drawn
    assert (lost <= 0.02 * candidates).all(), dict(zip(GROUPS, zip(candidates, drawn)))
    # pairs are independent of each other: the drawn ones are regrouped into genes of C cohorts
    keep = np.flatnonzero(informative)
    keep = keep[:len(keep) - len(keep) % C]
    if len(keep) % 256 == 0:
        keep = keep[:-C]
    rows, group = rows[keep], group[keep].reshape(-1, C)
    alpha, theta, pi, obs = to_inputs(rows)
    G = alpha.shape[0]
    sh = lambda a: np.ascontiguousarray(a[:, keep].reshape(a.shape[0], G, C))
    want_lr, A, S, flip = sh(want_lr), sh(A), sh(S), sh(flip)
    R = restate(alpha, theta, pi, obs)

    # burden planes
    bj = [(float(R["k"][q, g, c]), float(alpha[g, c]), float(R["p"][q, g, c])) for q in range(6) for g in range(G) for c in range(C)]
    todo = [j for j in bj if 0.0 < j[2] < 1.0]
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        res = dict(zip(todo, pool.map(routes.reference, todo, chunksize=4)))
    burden = np.full((6, G, C), np.nan)
    bcheck = np.zeros((6, G, C), np.uint8)
    for n, j in enumerate(bj):
        r = res.get(j)
        if r is not None:
            q, rem = divmod(n, G * C)
            burden[q, rem // C, rem % C] = r[0]
            bcheck[q, rem // C, rem % C] = 1

    want = R["planes"].copy()
    want[LR] = want_lr
    want[BURDEN] = burden
    check = np.ones((34, G, C), np.uint8)
    check[BURDEN] = bcheck
    check[LR] = ~flip
    kept = np.bincount(group.ravel(), minlength=len(GROUPS))

    # the CPU double restatement against the 80-digit values
    with np.errstate(all="ignore"):
        AS = np.where(S == 0, 0.0, A * S)
    rr = ratios(R["planes"][LR], want_lr, AS)
    rr = np.where(check[LR] == 1, rr, 0.0)
    cpu_worst = np.array([rr[:, group == gi].max() if (group == gi).any() else 0.0 for gi in range(len(GROUPS))])
    assert np.isfinite(cpu_worst).all(), cpu_worst

    ft = fisher_rows(rng)
    fr = [fisher_reference(r) for r in ft]
    f_want, f_h = np.array([r[0] for r in fr]), np.array([r[1] for r in fr])
    with np.errstate(all="ignore"):
        f_ratio = ratios(fisher_restate(ft[:, 0], ft[:, 1]), f_want, np.where(np.isfinite(f_h), f_h, 0.0))
    assert np.isfinite(f_ratio).all()

    out = dict(seed=np.int64(SEED), group_names=np.array(GROUPS), plane_names=np.array(PLANES),
               alpha=alpha, theta=theta, pi=pi, obs=obs, group=group.astype(np.int8), want=want, check=check,
               S=S.astype(np.float32), AS=np.nextafter(AS.astype(np.float32), np.float32(np.inf)),
               candidates_per_group=candidates.astype(np.int32), drawn_per_group=drawn.astype(np.int32),
               kept_per_group=kept.astype(np.int32), cpu_worst_ratio_per_group=cpu_worst,
               pi_sums=np.array([(pi[:, 4] == pi[:, 2] + pi[:, 3]).all() and (pi[:, 5] == pi[:, 1] + pi[:, 4]).all()]),
               fisher_p1=ft[:, 0], fisher_p2=ft[:, 1], fisher_want=f_want, fisher_h=f_h, fisher_cpu_worst_ratio=np.float64(f_ratio.max()),
               **{"sum64_" + n: sum64(R[n]) for n in SUMMED})
    routes.save_npz(OUT, out)
    size = os.path.getsize(OUT)
    print("%d genes x %d cohorts = %d pairs, %d Fisher rows, %d bytes" % (G, C, G * C, len(ft), size))
    for gi, name in enumerate(GROUPS):
        print("  %-16s candidates %4d  drawn %4d  kept %4d   CPU restatement worst ratio %.3g" %
              (name, candidates[gi], drawn[gi], kept[gi], cpu_worst[gi]))
    w = float(cpu_worst.max())
    print("CPU restatement: worst ratio %.3g -> M = %g;  Fisher: worst ratio %.3g -> M_f = %g" %
          (w, pow2_ceil(4 * w), float(f_ratio.max()), pow2_ceil(4 * float(f_ratio.max()))))
    print("burden planes checked: %d of %d" % (int(bcheck.sum()), bcheck.size))
    assert (G * C) % 256 != 0
    assert size <= routes.MAX_BYTES, "fixture larger than the largest one committed before it"


if __name__ == "__main__":
    main()
