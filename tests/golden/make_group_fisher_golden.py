"""Writes tests/golden/group_fisher_golden.npz: 80-digit references of Fisher's method over m = 3 .. 64 p-values, the m >= 3 clause of
dig_group_fisher (include/dig_hip.h).  Needs mpmath and no GPU; a run takes seconds.

A row is m doubles p[0 .. m); its reference is

    want = Q(m, s) = gammainc(m, s, inf, regularized=True),   s = -sum ln p_i

with every logarithm, the sum and Q at 80 digits, rounded ONCE to the nearest double (through a Fraction, so that a subnormal result is
rounded once as well).  `s` itself, rounded once, is stored too: the bound of a row is stated in it,

    |got / want - 1| <= M_G 2^-53 (1 + s)      (+ 4 x 2^-1074 absolute where want is subnormal; got = 0 where want = 0)

-- an error of one ulp on s moves Q by up to s ulps, as for the two-member form (tests/test_gene_selection_routes_fixture.py,
check_fisher).  The groups of rows, two rows per (group, m):

    uniform        p uniform in (0, 1)
    log12          p log-uniform in [1e-12, 1]
    log300         p log-uniform in [1e-300, 1]: the results are far below the doubles and round to 0; every other row is scaled so
                   that the product stays above 1e-300 (a result that is a number, with s up to 690)
    one_extreme    one member log-uniform in [1e-320, 1e-200] among uniform ones
    subnormal_in   one member subnormal (2^-1074 .. 2^-1023) among uniform ones in (0.05, 1); every other row one to three among
                   log12 ones (results that round to 0)
    subnormal_out  p drawn so that Q(m, s) itself is subnormal: s - ln r(s) in (712, 742)

restate() is the rule in doubles as the kernel states it -- the sum in ascending order, Horner, one exponential -- with its mutants;
main() prints its worst ratio per group, the figure M_G is derived from (tests/test_group_fisher_fixture.py)."""
import os
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "group_fisher_golden.npz")
SEED = 20261
U = 2.0 ** -53
TINY = 2.2250738585072014e-308
SUB = 4.0 * 2.0 ** -1074
CMAX = 64
GROUPS = ["uniform", "log12", "log300", "one_extreme", "subnormal_in", "subnormal_out"]
ROWS_PER_CELL = 2


def restate(p, mutant=None):
    """The m >= 3 clause for the rows of p f64 [N, 64] (NaN: no member) in doubles: (value [N], m [N], s [N]).  mutant: "exp_times_r"
    (exp(-s) r for exp(log(r) - s)), "m_with_nan" (every column counted as a member), "horner_short" (the last term left out)."""
    p = np.asarray(p, np.float64)
    ok = ~np.isnan(p)
    with np.errstate(all="ignore"):
        s = np.zeros(len(p))
        for c in range(p.shape[1]):
            s = s + np.where(ok[:, c], -np.log(np.where(ok[:, c], p[:, c], 1.0)), 0.0)
        m = ok.sum(axis=1) if mutant != "m_with_nan" else np.full(len(p), p.shape[1])
        top = m - 1 if mutant != "horner_short" else m - 2
        r = np.ones(len(p))
        for j in range(p.shape[1] - 1, 0, -1):
            r = np.where(j <= top, 1.0 + s / j * r, r)
        val = np.exp(-s) * r if mutant == "exp_times_r" else np.exp(np.log(r) - s)
        val = np.where(np.isnan(s), np.nan, np.where(s < 0, 1.0, np.where(np.isinf(s), 0.0, val)))
    return val, m, s


def ratios(got, want, s):
    """|got / want - 1| in units of 2^-53 (1 + s); a subnormal reference gets 4 x 2^-1074 absolute on top; want = 0 -> got must be 0
    (inf otherwise); a NaN on one side only -> inf."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(all="ignore"):
        err = np.abs(got - want)
        err = np.where((want < TINY) & (want > 0), np.maximum(err - SUB, 0.0), err)
        r = err / np.abs(want) / (U * (1.0 + np.asarray(s, np.float64)))
    r = np.where(want == 0, np.where(got == 0, 0.0, np.inf), r)
    return np.where(np.isnan(got) | np.isnan(want), np.where(np.isnan(got) & np.isnan(want), 0.0, np.inf), r)


def pow2_ceil(v):
    return float(2.0 ** np.ceil(np.log2(v)))


def _fl(x):
    """An mpf -> the nearest double, one rounding (subnormals included)."""
    sign, man, exp, _ = x._mpf_
    fr = Fraction(int(man)) * (Fraction(2) ** int(exp))
    return float(-fr if sign else fr)


def reference(row):
    """(want, s) of one row of doubles at 80 digits, each rounded once."""
    import mpmath as mp
    mp.mp.dps = 80
    s = -sum(mp.log(mp.mpf(float(v))) for v in row)
    return _fl(mp.gammainc(len(row), s, mp.inf, regularized=True)), _fl(s)


def _loguniform(rng, lo, hi, n):
    return 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), n)


def _s_for_exponent(m, t):
    """s with s - ln r(s) = t (doubles, bisection): where Q(m, s) = exp(-t)."""
    lo, hi = 0.0, 745.0 * m
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        r = 1.0
        for j in range(m - 1, 0, -1):
            r = 1.0 + mid / j * r
        lo, hi = (mid, hi) if mid - np.log(r) < t else (lo, mid)
    return lo


def draw(rng):
    rows, group = [], []
    for gi, name in enumerate(GROUPS):
        for m in range(3, CMAX + 1):
            for rep in range(ROWS_PER_CELL):
                if name == "uniform":
                    p = rng.uniform(size=m)
                elif name == "log12":
                    p = _loguniform(rng, 1e-12, 1.0, m)
                elif name == "log300":
                    x = rng.uniform(0.0, 300.0, m)                 # p = 10^-x
                    if rep == 0 and x.sum() > 300.0:               # the product kept above 1e-300: a result that is a number
                        x *= 300.0 / x.sum() * rng.uniform(0.5, 1.0)
                    p = 10.0 ** -x
                elif name == "one_extreme":
                    p = rng.uniform(size=m)
                    p[rng.integers(0, m)] = _loguniform(rng, 1e-320, 1e-200, 1)[0]
                elif name == "subnormal_in":
                    p = rng.uniform(0.05, 1.0, m) if rep == 0 else _loguniform(rng, 1e-12, 1.0, m)
                    for i in rng.choice(m, size=1 if rep == 0 else int(rng.integers(1, 4)), replace=False):
                        p[i] = np.ldexp(rng.uniform(0.5, 1.0), int(rng.integers(-1073, -1022)))
                else:
                    s = _s_for_exponent(m, rng.uniform(712.0, 742.0))
                    share = rng.dirichlet(np.ones(m))
                    while (s * share > 700.0).any():
                        share = rng.dirichlet(np.ones(m))
                    p = np.exp(-s * share)
                assert (p > 0).all() and (p <= 1).all()
                rows.append(np.asarray(p, np.float64))
                group.append(gi)
    return rows, np.array(group, np.int32)


def main():
    rng = np.random.default_rng(SEED)
    rows, group = draw(rng)
    ref = [reference(r) for r in rows]
    want, s = np.array([w for w, _ in ref]), np.array([v for _, v in ref])
    p = np.full((len(rows), CMAX), np.nan)
    for i, r in enumerate(rows):
        p[i, :len(r)] = r
    got, m, _ = restate(p)
    ratio = ratios(got, want, s)
    worst = np.array([ratio[group == gi].max() for gi in range(len(GROUPS))])
    for gi, name in enumerate(GROUPS):
        k = group == gi
        print("%-14s rows %4d  subnormal %3d  zero %3d  worst ratio of the double restatement %.3f" % (
            name, int(k.sum()), int(((want[k] > 0) & (want[k] < TINY)).sum()), int((want[k] == 0).sum()), worst[gi]))
    print("worst ratio %.3f -> M_G = %g" % (worst.max(), pow2_ceil(4 * worst.max())))
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    np.savez_compressed(OUT, p=np.concatenate(rows), ptr=ptr, want=want, s=s, group=group, group_names=np.array(GROUPS),
                        cpu_worst_ratio_per_group=worst)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


def load():
    """The table as dict(p f64 [N, 64] NaN-padded, m [N], want, s, group, group_names, cpu_worst_ratio_per_group)."""
    d = dict(np.load(OUT, allow_pickle=False))
    ptr = d.pop("ptr")
    flat = d["p"]
    p = np.full((len(ptr) - 1, CMAX), np.nan)
    for i in range(len(ptr) - 1):
        p[i, :ptr[i + 1] - ptr[i]] = flat[ptr[i]:ptr[i + 1]]
    d["p"], d["m"] = p, np.diff(ptr).astype(np.int64)
    return d


if __name__ == "__main__":
    main()
