"""Writes tests/golden/nb_power_golden.npz: critical counts of the upper mid-p burden test and the powers at them (dig_nb_power,
include/dig_hip.h), computed by the REAL reference functions nb_pvalue_greater_midp and nb_pvalue_greater.

Run in the build container only (it needs the reference tree, DIG_REFERENCE, default /root/reference, scipy and mpmath):

    python tests/golden/make_nb_power_golden.py

* Stubs the reference's absent I/O-only dependencies as make_golden.py does and imports the reference from its own location; nothing
  of it is copied.  The scan over k is tests/nb_power_statement.py with the reference's two functions handed in.
* A row is (alpha, theta, pi, cj, level, k_max); theta' = theta * cj.  Rows that share (level, cj, k_max) form a BLOCK: one row of a
  [R, n] plane, which has one level and one scale per row.  FOLDS = (1, 2, 5, 10, 100, 0.5).
* Regular blocks: levels {0.05, 1e-3, 1e-6, 1e-12, 1e-30} x cj {0.2, 0.7, 3}, ROWS_PER_BLOCK rows each in the SURVEY 8c ranges (mu
  log-uniform [0.05, 500], sigma / mu log-uniform [0.05, 1.5], Pi log-uniform [1e-5, 1]), k_max = 2^15 (a row that no k <= 2^15 brings
  to its level is stored as K = -1).
* Edge blocks (edge_rows()): Pi = 0, mu < 0, sigma = 0, a NaN in each input, levels {0, 1, NaN, -1, 0.5, 1 - 2^-53}, M(0) <= level,
  K = k_max, K = k_max + 1, k_max = 0, K = kSmallK - 1 .. kSmallK + 2 (the two paths of the device's statistic on either side of a
  crossing), and ONE tie: Pi = 0 at level 0.5, where M(0) = 0.5 = level exactly in doubles (the row that tells <= from <).
* Stored per row: K, M(K - 1) and M(K) by the reference (NaN where there is none), the six powers.
* The margin rule: a row is kept only if neither M(K - 1) nor M(K) (M(k_max) for K = -1 out of reach) lies within 1e-6 relative of
  the level -- the project's p-value tolerance -- and is redrawn otherwise (an edge row that misses it is an error); the tie is the
  one exception and is flagged.  Both values are confirmed at 80 digits with mpmath (the pmf recurrence summed from 0, every term
  exact to 80 digits, rounded once): the same side of the level, and within 1e-9 relative of the reference's doubles.
"""
import os
import sys
import types
from fractions import Fraction

sys.dont_write_bytecode = True

import numpy as np

REF = os.environ.get("DIG_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "nb_power_golden.npz")
sys.path.insert(0, os.path.dirname(HERE))

SEED = 20261021
FOLDS = (1.0, 2.0, 5.0, 10.0, 100.0, 0.5)
LEVELS = (0.05, 1e-3, 1e-6, 1e-12, 1e-30)
CJS = (0.2, 0.7, 3.0)
ROWS_PER_BLOCK = 200
K_MAX = 1 << 15
MARGIN = 1e-6
K_SMALL = 128                      # kSmallK (digdriver_amd/csrc/dig_math.hpp)


def install_stubs():
    for name in ["pysam", "pybedtools", "h5py", "statsmodels", "statsmodels.stats", "statsmodels.stats.multitest", "seaborn",
                 "bbi", "tables", "gpytorch", "tensorboardX", "pkg_resources"]:
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.path.insert(0, REF)


def _fl(x):
    """An mpf -> the nearest double, one rounding (subnormals included)."""
    sign, man, exp, _ = x._mpf_
    fr = Fraction(int(man)) * (Fraction(2) ** int(exp))
    return float(-fr if sign else fr)


def midp_80(ks, alpha, p):
    """M(k) for the ascending counts ks at 80 digits, each rounded once: 1 - sum_{j<k} pmf(j) - pmf(k) / 2 by the pmf recurrence."""
    import mpmath as mp
    mp.mp.dps = 80
    a, pp = mp.mpf(float(alpha)), mp.mpf(float(p))
    x = 1 - pp
    t, S, out, j = mp.power(pp, a), mp.mpf(0), [], 0
    for k in ks:
        while j < k:
            S += t
            t = t * (a + j) * x / (j + 1)
            j += 1
        out.append(_fl(1 - S - t / 2))
    return out


def near(m, level):
    return abs(m / level - 1.0) <= MARGIN


class Maker:
    def __init__(self, ref_nb):
        import nb_power_statement as S
        self.S, self.ref = S, ref_nb
        self.rows, self.worst_mp, self.closest = [], 0.0, np.inf

    def midp(self, k, alpha, p):
        with np.errstate(all="ignore"):
            return self.ref.nb_pvalue_greater_midp(k, alpha, p)

    def greater(self, k, alpha, p):
        with np.errstate(all="ignore"):
            return float(self.ref.nb_pvalue_greater(k, alpha, p))

    def count(self, alpha, theta, pi, cj, level, k_max):
        p = float(self.S.success_prob(theta, pi, 1.0, cj))
        return self.S.critical_count(alpha, p, level, k_max, midp=self.midp) + (p,)

    def row(self, alpha, theta, pi, cj, level, k_max, tie=False):
        """The stored row, or None where the margin rule refuses it."""
        K, undefined, p = self.count(alpha, theta, pi, cj, level, k_max)
        m_lo = m_hi = np.nan
        if not undefined:
            ks = [k_max] if K < 0 else ([K - 1] if K > 0 else []) + [K]
            ms = [float(self.midp(np.array([float(k)]), alpha, p)[0]) for k in ks]
            if not tie:
                if any(near(m, level) for m in ms):
                    return None
                self.closest = min([self.closest] + [abs(m / level - 1.0) for m in ms])
            if p < 1.0:
                for m, m80, k in zip(ms, midp_80(ks, alpha, p), ks):
                    assert (m <= level) == (m80 <= level) and (tie or not near(m80, level)), (alpha, p, level, k, m, m80)
                    if m80 >= 1e-250:
                        self.worst_mp = max(self.worst_mp, abs(m / m80 - 1.0))
            if K >= 0:
                m_hi, m_lo = ms[-1], (ms[0] if K > 0 else np.nan)
                assert m_hi <= level and (K == 0 or m_lo > level)
            else:
                assert ms[0] > level
        power = [(np.nan if undefined else 0.0) if K < 0 else
                 self.greater(K, alpha, float(self.S.success_prob(theta, pi, f, cj))) for f in FOLDS]
        return [alpha, theta, pi, cj, level, k_max, K, m_lo, m_hi, float(tie)] + power

    def add(self, *args, **kw):
        r = self.row(*args, **kw)
        assert r is not None, ("an edge row within the margin of its level", args)
        self.rows.append(r)
        return r

    def tune_theta(self, target, alpha, pi, cj, level):
        """theta at which K = target (K does not fall as theta grows): bisection on log theta."""
        lo, hi = np.log(1e-3), np.log(1e7)
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            K = self.count(alpha, float(np.exp(mid)), pi, cj, level, 1 << 20)[0]
            if K == target:
                return float(np.exp(mid))
            lo, hi = (mid, hi) if K < target else (lo, mid)
        raise AssertionError("no theta gives K = %d" % target)


def regular(mk, rng):
    for level in LEVELS:
        for cj in CJS:
            kept = 0
            while kept < ROWS_PER_BLOCK:
                mu = float(np.exp(rng.uniform(np.log(0.05), np.log(500.0))))
                sigma = mu * float(np.exp(rng.uniform(np.log(0.05), np.log(1.5))))
                pi = float(np.exp(rng.uniform(np.log(1e-5), 0.0)))
                alpha, theta = mk.ref.normal_params_to_gamma(np.float64(mu), np.float64(sigma))
                r = mk.row(float(alpha), float(theta), pi, cj, level, K_MAX)
                if r is not None:
                    mk.rows.append(r)
                    kept += 1


def edge_rows(mk):
    nan = float("nan")
    g = lambda mu, sigma: tuple(float(v) for v in mk.ref.normal_params_to_gamma(np.float64(mu), np.float64(sigma)))
    a0, t0 = g(3.0, 2.0)                                          # an ordinary element: alpha 2.25, theta 1.33
    # Pi = 0: p = 1, M(0) = 0.5 and M(k > 0) = 0
    mk.add(a0, t0, 0.0, 0.7, 0.05, K_MAX)
    mk.add(a0, t0, 0.0, 0.7, 0.7, K_MAX)
    mk.add(a0, t0, 0.0, 0.7, 0.5, K_MAX, tie=True)                # M(0) = level exactly: K = 0 by <=, 1 by <
    mk.add(a0, t0, 0.0, 0.7, 0.05, 0)                             # ... and out of reach with k_max = 0
    # mu < 0, sigma = 0, mu = 0, a NaN in each input
    with np.errstate(all="ignore"):
        for mu, sigma in ((-3.0, 2.0), (5.0, 0.0), (0.0, 2.0), (0.0, 0.0)):
            mk.add(*g(mu, sigma), 0.01, 0.7, 1e-3, K_MAX)
    mk.add(nan, t0, 0.01, 0.7, 1e-3, K_MAX)
    mk.add(a0, nan, 0.01, 0.7, 1e-3, K_MAX)
    mk.add(a0, t0, nan, 0.7, 1e-3, K_MAX)
    mk.add(a0, t0, 0.01, nan, 1e-3, K_MAX)
    # levels outside (0, 1), a NaN level, and two odd ones inside
    for level in (0.0, 1.0, nan, -1.0, 0.5, 1.0 - 2.0 ** -53):
        for pi in (0.01, 0.5):
            mk.add(a0, t0, pi, 0.7, level, K_MAX)
    # M(0) <= level: K = 0, every power 1
    mk.add(a0, t0, 1e-3, 0.2, 0.9, K_MAX)
    mk.add(a0, t0, 1e-3, 0.2, 0.9, 0)
    # K = k_max, K = k_max + 1, k_max = 0 under a K > 0
    for alpha, theta, pi, cj, level in ((a0, t0, 0.3, 0.7, 1e-6), (40.0, 2.0, 0.5, 3.0, 1e-12), (0.3, 50.0, 0.2, 0.2, 1e-3)):
        K = mk.count(alpha, theta, pi, cj, level, 1 << 20)[0]
        assert K > 1
        for k_max in (K, K - 1, K + 1, 0):
            r = mk.add(alpha, theta, pi, cj, level, k_max)
            assert r[6] == (K if k_max >= K else -1)
    # K around kSmallK, at a small and a large dispersion and two levels
    for alpha, pi, cj, level in ((4.0, 0.01, 0.7, 1e-6), (0.4, 0.3, 3.0, 1e-3), (60.0, 0.05, 0.2, 1e-12)):
        for target in range(K_SMALL - 1, K_SMALL + 3):
            r = mk.add(alpha, mk.tune_theta(target, alpha, pi, cj, level), pi, cj, level, K_MAX)
            assert r[6] == target


def main():
    install_stubs()
    from DIGDriver.sequence_model import nb_model as ref_nb        # noqa: E402
    mk = Maker(ref_nb)
    regular(mk, np.random.default_rng(SEED))
    n_regular = len(mk.rows)
    edge_rows(mk)
    t = np.array(mk.rows, np.float64)
    # rows that share (level, cj, k_max) are one block (NaNs compared by their bits); the edge rows keep to blocks of their own
    key = np.ascontiguousarray(np.column_stack([t[:, 3:6], np.arange(len(t)) >= n_regular])).view(np.int64)
    _, first, block = np.unique(key, axis=0, return_index=True, return_inverse=True)
    block = np.argsort(np.argsort(first))[block.reshape(-1)]       # numbered in order of appearance: the regular blocks first
    K = t[:, 6].astype(np.int32)
    print("rows %d (%d regular, %d edge), blocks %d; K max %d, median %g, out of reach %d, undefined %d" % (
        len(t), n_regular, len(t) - n_regular, block.max() + 1, K.max(), np.median(K[:n_regular]),
        int(((K < 0) & ~np.isnan(t[:, 10])).sum()), int(np.isnan(t[:, 10]).sum())))
    print("closest |M / level - 1| kept %.3g; worst |reference / 80 digits - 1| of M(K - 1), M(K) %.3g" % (mk.closest, mk.worst_mp))
    assert mk.worst_mp <= 1e-9
    np.savez_compressed(OUT, alpha=t[:, 0], theta=t[:, 1], pi=t[:, 2], cj=t[:, 3], level=t[:, 4], k_max=t[:, 5].astype(np.int32),
                        k_crit=K, m_below=t[:, 7], m_at=t[:, 8], tie=t[:, 9] != 0, power=np.ascontiguousarray(t[:, 10:].T),
                        folds=np.array(FOLDS), block=block.astype(np.int32), n_regular=np.int64(n_regular),
                        rows_per_block=np.int64(ROWS_PER_BLOCK), closest=np.float64(mk.closest), worst_80=np.float64(mk.worst_mp))
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
