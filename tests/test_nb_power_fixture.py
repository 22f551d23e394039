"""The table of critical counts and powers (tests/golden/nb_power_golden.npz, written by tests/golden/make_nb_power_golden.py with the
reference's own nb_pvalue_greater_midp and nb_pvalue_greater) checked on its own, without a GPU, and the proof that its checkers
have teeth.

check_counts() and nb_power_statement.check_power() are the checkers of this test and of tests/test_gpu_nb_power*.py.

    K       equality on EVERY row.  That is a condition on the table, not a measurement: the maker keeps a row only if neither
            M(K - 1) nor M(K) lies within 1e-6 relative of the level (the project's p-value tolerance, README), so a statistic
            within that tolerance of the reference's finds the reference's count.  The one flagged tie, Pi = 0 at level 0.5, has
            M(0) = 0.5 = level exactly in doubles, in the reference and on the device (the p == 1 clause of the statistic).
    power   |got / want - 1| <= 1e-6 where want >= 1e-250, both below 1e-250 otherwise; NaN and 0.0 at K = -1 and 1.0 at K = 0 match
            exactly (README / SURVEY 8c).

Three mutants of the statement are each rejected under their name: the statistic without the mid-p half-weight (pmf(k) counted
whole), <= replaced by < (it moves the tie), and the power taken at K + 1."""
import os

import numpy as np
import pytest
import scipy.special
import scipy.stats

import nb_power_statement as S
from conftest import GOLDEN

PATH = os.path.join(GOLDEN, "nb_power_golden.npz")
K_SMALL = 128


def load_fixture():
    d = dict(np.load(PATH, allow_pickle=False))
    d["folds"] = tuple(float(f) for f in d["folds"])
    return d


def blocks_of(fx):
    """[(rows of the block, level, cj, k_max)] in block order: the rows that one row of a plane can hold."""
    out = []
    for b in range(int(fx["block"].max()) + 1):
        rows = np.flatnonzero(fx["block"] == b)
        i = rows[0]
        out.append((rows, float(fx["level"][i]), float(fx["cj"][i]), int(fx["k_max"][i])))
    return out


def check_counts(got, fx, what="", rows=None):
    """K [N] (or the rows `rows` of it) against the table: equality on every row; raises under the name `what`."""
    rows = np.arange(len(fx["k_crit"])) if rows is None else np.asarray(rows)
    got, want = np.asarray(got).reshape(-1), fx["k_crit"][rows]
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    print("%s K: %d rows, %d differ" % (what, len(rows), len(bad)))
    if len(bad):
        raise AssertionError("%s: %d of %d critical counts differ\n" % (what, len(bad), len(rows)) + "\n".join(
            "%s: row %d (alpha %r, theta %r, pi %r, cj %r, level %r, k_max %d): got %d, want %d (M(K - 1) %r, M(K) %r)" % (
                what, rows[i], fx["alpha"][rows[i]], fx["theta"][rows[i]], fx["pi"][rows[i]], fx["cj"][rows[i]], fx["level"][rows[i]],
                fx["k_max"][rows[i]], got[i], want[i], fx["m_below"][rows[i]], fx["m_at"][rows[i]]) for i in bad[:10]))


def statement_rows(fx, rows, **kw):
    """The statement applied to the rows `rows`, one at a time: (K [n], power [F, n])."""
    K, power = np.empty(len(rows), np.int32), np.empty((len(fx["folds"]), len(rows)))
    for j, i in enumerate(rows):
        k, pw = S.nb_power(fx["alpha"][i], fx["theta"][i], fx["pi"][i], fx["level"][i], scale=fx["cj"][i], folds=fx["folds"],
                           k_max=int(fx["k_max"][i]), **kw)
        K[j], power[:, j] = k[0, 0], pw[:, 0, 0]
    return K, power


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.fixture(scope="module")
def sample(fx):
    """Every edge row and the first 40 rows of every regular block: what the mutants are run on."""
    n, per = int(fx["n_regular"]), int(fx["rows_per_block"])
    return np.concatenate([np.flatnonzero(np.arange(n) % per < 40), np.arange(n, len(fx["k_crit"]))])


def test_table_covers_what_it_was_written_for(fx):
    assert os.path.getsize(PATH) <= 512 * 1024
    K, level, k_max, n = fx["k_crit"], fx["level"], fx["k_max"], int(fx["n_regular"])
    assert n >= 3000 and fx["folds"] == (1.0, 2.0, 5.0, 10.0, 100.0, 0.5) and fx["power"].shape == (6, len(K))
    assert sorted(set(level[:n].tolist())) == [1e-30, 1e-12, 1e-6, 1e-3, 0.05] and sorted(set(fx["cj"][:n].tolist())) == [0.2, 0.7, 3.0]
    reg = blocks_of(fx)[:15]
    assert all(len(rows) == int(fx["rows_per_block"]) and rows[-1] < n for rows, _, _, _ in reg)
    # the margin rule, on every row but the one tie
    free = ~fx["tie"]
    with np.errstate(all="ignore"):
        for m in (fx["m_below"], fx["m_at"]):
            assert not (np.abs(m / level - 1.0) <= 1e-6)[free].any()
    assert (fx["m_at"][K >= 0] <= level[K >= 0]).all() and (fx["m_below"][K > 0] > level[K > 0]).all()
    assert np.isnan(fx["m_below"][K <= 0]).all() and np.isnan(fx["m_at"][K < 0]).all()
    assert int(fx["tie"].sum()) == 1 and fx["m_at"][fx["tie"]][0] == 0.5 == level[fx["tie"]][0] and K[fx["tie"]][0] == 0
    # the clauses of the power
    undefined = np.isnan(fx["power"][0])
    assert (K[undefined] == -1).all() and np.isnan(fx["power"][:, undefined]).all() and undefined.sum() >= 14
    unreached = (K < 0) & ~undefined
    assert (fx["power"][:, unreached] == 0.0).all() and unreached.sum() >= 7 and (fx["power"][:, K == 0] == 1.0).all()
    # the edges
    edge = np.arange(len(K)) >= n
    assert (fx["pi"][edge] == 0).sum() >= 4 and (K == k_max)[edge & (k_max > 0)].sum() >= 3 and (K == 0)[edge & (k_max == 0)].any()
    assert ((K == -1) & (k_max == 0) & ~undefined).any()
    for target in range(K_SMALL - 1, K_SMALL + 3):
        assert (K[edge] == target).sum() >= 3
    for v in (0.0, 1.0, -1.0, 0.5, 1.0 - 2.0 ** -53):
        assert (level[edge] == v).any()
    assert np.isnan(level[edge]).any() and all(np.isnan(fx[c][edge]).any() for c in ("alpha", "theta", "pi", "cj"))
    assert K.max() > 1 << 14 and np.median(K[:n]) >= 2


def test_statement_reproduces_the_table(fx):
    rows = np.arange(len(fx["k_crit"]))
    K, power = statement_rows(fx, rows)
    check_counts(K, fx, "statement")
    S.check_power(power, fx["power"], fx["k_crit"], "statement")
    # ... and whole blocks at once, as planes [3, n] with a level and a scale per row
    b = blocks_of(fx)
    pick = [b[0], b[7], b[14]]
    K3, p3 = S.nb_power(*[np.stack([fx[c][r] for r, _, _, _ in pick]) for c in ("alpha", "theta", "pi")], [l for _, l, _, _ in pick],
                        scale=[c for _, _, c, _ in pick], folds=fx["folds"][:2], k_max=pick[0][3])
    for j, (r, _, _, _) in enumerate(pick):
        check_counts(K3[j], fx, "statement, planes", rows=r)
        assert np.array_equal(p3[:, j], power[:2, r], equal_nan=True)


def _no_half_weight(k, alpha, p):
    with np.errstate(all="ignore"):
        return scipy.stats.nbinom.pmf(k, alpha, p) + scipy.special.betainc(k + 1.0, alpha, 1.0 - p)


def test_mutants_of_the_statement_are_rejected_by_name(fx, sample):
    K, _ = statement_rows(fx, sample, midp=_no_half_weight)
    with pytest.raises(AssertionError, match="^no_half_weight: "):
        check_counts(K, fx, "no_half_weight", rows=sample)
    tie = np.flatnonzero(fx["tie"])
    K, _ = statement_rows(fx, tie, strict=True)
    assert K[0] == 1
    with pytest.raises(AssertionError, match="^strict_less: "):
        check_counts(K, fx, "strict_less", rows=tie)
    K, power = statement_rows(fx, sample, power_at=1)
    check_counts(K, fx, "power_at_k_plus_1", rows=sample)                  # (the counts are the table's ...)
    with pytest.raises(AssertionError, match="^power_at_k_plus_1: "):      # (... the powers are not)
        S.check_power(power, fx["power"][:, sample], fx["k_crit"][sample], "power_at_k_plus_1")


def test_checkers_reject_a_single_wrong_value(fx):
    K = fx["k_crit"].copy()
    K[5] += 1
    with pytest.raises(AssertionError, match="row 5 "):
        check_counts(K, fx, "edge")
    i = int(np.flatnonzero(fx["k_crit"] > 0)[0])
    for v in (np.nan, fx["power"][1, i] * (1 + 3e-6), 0.0):
        bad = fx["power"].copy()
        bad[1, i] = v
        with pytest.raises(AssertionError, match=r"at \(1, %d\)" % i):
            S.check_power(bad, fx["power"], fx["k_crit"], "edge")
    j = int(np.flatnonzero(fx["k_crit"] == 0)[0])
    bad = fx["power"].copy()
    bad[0, j] = 1.0 - 2.0 ** -53
    with pytest.raises(AssertionError, match=r"at \(0, %d\)" % j):
        S.check_power(bad, fx["power"], fx["k_crit"], "edge")
