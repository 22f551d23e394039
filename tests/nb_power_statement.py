"""The plain numpy / scipy statement of dig_nb_power (include/dig_hip.h): the critical count of the upper mid-p burden test by a
brute-force scan of k with the reference's two-line formulas, and the power at it.  What tests/test_nb_power_fixture.py,
test_gpu_nb_power.py, test_gpu_nb_power_guarded.py and test_gpu_element_power.py compare against.

    midp(k, alpha, p)     = 0.5 nbinom.pmf(k, alpha, p) + betainc(k + 1, alpha, 1 - p)          nb_model.py:271-278
    greater(k, alpha, p)  = 1 for k = 0, else betainc(k, alpha, 1 - p), nbinom.pmf where that is 0   nb_model.py:243-256
    p(f)                  = 1 / (((theta * scale) * pi) * f + 1), every product one multiplication, left to right

The scan is vectorised over k in growing chunks and stops at the first k whose statistic is <= the level.  `midp` and `greater` may
be replaced (the fixture is written with the reference's own functions in their place; the mutants of the fixture test replace
them too)."""
import numpy as np
import scipy.special
import scipy.stats


def midp(k, alpha, p):
    with np.errstate(all="ignore"):
        return 0.5 * scipy.stats.nbinom.pmf(k, alpha, p) + scipy.special.betainc(k + 1.0, alpha, 1.0 - p)


def greater(k, alpha, p):
    """Scalar k, as the reference's."""
    if k == 0:
        return 1.0
    with np.errstate(all="ignore"):
        pv = scipy.special.betainc(float(k), alpha, 1.0 - p)
        if pv == 0:
            pv = scipy.stats.nbinom.pmf(k, alpha, p)
    return float(pv)


def success_prob(theta, pi, fold=1.0, scale=None):
    with np.errstate(all="ignore"):
        t = np.asarray(theta, np.float64) if scale is None else np.asarray(theta, np.float64) * scale
        return 1.0 / ((t * pi) * fold + 1.0)


def critical_count(alpha, p, level, k_max, midp=midp, strict=False):
    """(K, undefined) for scalars: the smallest k in [0, k_max] with midp(k) <= level (strict=True: <, a mutant); K = -1 with
    undefined = False where none reaches it, with undefined = True where the statistic is NaN or the level not inside (0, 1)."""
    if not (level > 0.0 and level < 1.0) or np.isnan(midp(np.array([0.0]), alpha, p)[0]):
        return -1, True
    lo, size = 0, 64
    while lo <= k_max:
        k = np.arange(lo, min(lo + size, k_max + 1), dtype=np.float64)
        v = midp(k, alpha, p)
        hit = np.flatnonzero(v < level if strict else v <= level)
        if len(hit):
            return lo + int(hit[0]), False
        lo, size = lo + size, min(size * 4, 1 << 16)
    return -1, False


def nb_power(alpha, theta, pi, level, scale=None, folds=(), k_max=1 << 20, midp=midp, greater=greater, strict=False, power_at=0):
    """k_crit i32 [R, n] and power f64 [F, R, n] of planes [R, n], level / scale [R].  power_at: the power is taken at K + power_at
    (a mutant of the fixture test)."""
    alpha, theta, pi = (np.atleast_2d(np.asarray(x, np.float64)) for x in (alpha, theta, pi))
    R, n = alpha.shape
    level = np.broadcast_to(np.asarray(level, np.float64), (R,))
    scale = None if scale is None else np.broadcast_to(np.asarray(scale, np.float64), (R,))
    K, power = np.empty((R, n), np.int32), np.empty((len(folds), R, n))
    for r in range(R):
        sc = None if scale is None else scale[r]
        p1 = success_prob(theta[r], pi[r], 1.0, sc)
        pf = [success_prob(theta[r], pi[r], f, sc) for f in folds]
        for e in range(n):
            k, undefined = critical_count(alpha[r, e], p1[e], level[r], k_max, midp=midp, strict=strict)
            K[r, e] = k
            for j in range(len(folds)):
                power[j, r, e] = (np.nan if undefined else 0.0) if k < 0 else greater(k + power_at, alpha[r, e], pf[j][e])
    return K, power


def check_power(got, want, k_crit, what=""):
    """The README / SURVEY 8c contract: |got / want - 1| <= 1e-6 where want >= 1e-250, both below 1e-250 otherwise; the clauses
    -- NaN and 0.0 at K = -1, 1.0 at K = 0 -- must match exactly.  got, want [F, ...], k_crit [...]: the reference's counts.  Prints
    the worst ratio, raises under the name `what`."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    exact = np.isnan(want) | np.broadcast_to(np.asarray(k_crit) <= 0, want.shape)
    ok = np.where(np.isnan(want), np.isnan(got), got == want)
    small = ~exact & (want < 1e-250)
    ok = np.where(small, (got < 1e-250) & (got >= 0), ok)
    rest = ~exact & ~small
    with np.errstate(all="ignore"):
        rel = np.abs(got / want - 1.0)
    ok = np.where(rest, rel <= 1e-6, ok)
    print("%s power: %d values, %d exact clauses, %d below 1e-250, worst |got / want - 1| %.3g" % (
        what, got.size, int(exact.sum()), int(small.sum()), float(rel[rest].max()) if rest.any() else 0.0))
    bad = np.argwhere(~ok)
    if len(bad):
        raise AssertionError("%s: %d powers miss the contract\n" % (what, len(bad)) + "\n".join(
            "%s: at %s got %r, want %r" % (what, tuple(int(v) for v in i), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:10]))
