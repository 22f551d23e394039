"""The fixture of tests/test_gpu_nb_routes.py checked on its own (no GPU): tests/golden/nb_routes_golden.npz has every route
populated at its switch points, few rows dropped, the cross-check run on nearly all rows, and it agrees with the scipy oracle --
which would not be so if the maker (tests/golden/make_nb_routes_golden.py) summed or labelled wrongly."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN, rel_close


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "nb_routes_golden.npz")))


@pytest.fixture(scope="module")
def maker():
    spec = importlib.util.spec_from_file_location("make_nb_routes_golden", os.path.join(GOLDEN, "make_nb_routes_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)           # (mpmath is imported only where a reference is evaluated)
    return mod


def test_every_route_is_populated_and_few_rows_were_dropped(fx, maker):
    names = list(fx["route_names"])
    assert names == maker.ROUTES and list(fx["path_names"]) == maker.PATHS
    counts = np.bincount(fx["route"], minlength=len(names))
    assert (counts >= 40).all(), dict(zip(names, counts))
    drawn, kept = fx["drawn_per_group"], fx["kept_per_group"]
    assert (drawn >= 40).all() and (kept >= 0.95 * drawn).all(), (drawn, kept)
    assert fx["pair_kept"] >= 0.95 * fx["pair_drawn"] and fx["pair_kept"] == len(fx["pair_k1"])
    # ... and no group was thinned on the way to `drawn`: rows turned away because the reference's own rounding of 1 - p decides
    # their value stay below a tenth of a group, candidates that could not be placed at all (solve_p) below a fifth
    turned = fx["rounding_filtered_per_group"]
    assert (turned <= 0.10 * (drawn + turned)).all(), (turned, drawn)
    assert (drawn + turned >= 0.80 * fx["candidates_per_group"]).all(), (fx["candidates_per_group"], drawn, turned)
    assert fx["pair_rounding_filtered"] <= 0.10 * fx["pair_placed"] and fx["pair_drawn"] + fx["pair_rounding_filtered"] <= fx["pair_placed"]
    small = (fx["k"] <= 4200) & (fx["p"] < 1)
    assert fx["checked"][small].mean() >= 0.90
    assert fx["pair_checked"].mean() >= 0.90
    assert os.path.getsize(os.path.join(GOLDEN, "nb_routes_golden.npz")) <= maker.MAX_BYTES
    with np.errstate(all="ignore"):
        mu = fx["alpha"] * (1 - fx["p"]) / fx["p"]
        assert not (np.abs(fx["k"] - mu) < 1e-9 * mu).any()
    assert (fx["k"] >= 0).all() and (fx["k"] == np.floor(fx["k"])).all() and fx["k"].max() <= 5000


def test_scipy_oracle_agrees_with_the_fixture(fx):
    """1e-6 is the contract; what scipy is actually off by on this fixture is 2.3e-10 (k = 92, alpha = 0.21, p = 2.3e-9: the
    upper entry points, where the reference evaluates betainc(k + 1, alpha, 1 - p) at the ROUNDED 1 - p) and 1e-12 on the lower
    side.  That is so only because the maker turns rows away once that rounding moves the upper tail by more than 1e-9: before it
    did, rows with p ~ 1e-13 stood at 3e-6 to 8e-7 and rows with p ~ 5e-17, alpha ~ 0.02 at 85 %.  So a
    disagreement above ~1e-9 here means the maker or its filter is wrong, long before 1e-6 says so."""
    from oracle import dig_oracle as O
    k, alpha, p = fx["k"], fx["alpha"], fx["p"]
    greater = np.where(k == 0, 1.0, np.where(fx["geq"] == 0, fx["pmf"], fx["geq"]))
    with np.errstate(all="ignore"):
        rel_close(O.nb_pvalue_greater_midp(k, alpha, p), fx["midp_upper"], 1e-6)
        rel_close(O.nb_pvalue_greater(k, alpha, p), greater, 1e-6)
        rel_close(O.nb_pvalue_exact(k, alpha, p), fx["exact"], 1e-6)
        rel_close(O.nb_pvalue_midp(k, alpha, p), fx["midp"], 1e-6)
        rel_close(O.nb_pvalue_greater_midp(fx["pair_k1"], fx["pair_alpha"], fx["pair_p"]), fx["pair_midp_upper1"], 1e-6)
        rel_close(O.nb_pvalue_greater_midp(fx["pair_k2"], fx["pair_alpha"], fx["pair_p"]), fx["pair_midp_upper2"], 1e-6)
        # the stored (alpha, p) are the doubles the fused kernels form from (mu, sigma) with pi = cj = 1
        f = np.isfinite(fx["mu"])
        one = np.ones(int(f.sum()))
        r = O.element_stats(fx["mu"][f], fx["sigma"][f], one, one, 0 * one, 0 * one, 0 * one, 1.0, 1.0)
        assert np.array_equal(r["ALPHA"], alpha[f]) and np.array_equal(1 / (r["THETA"] * one + 1), p[f])
        one = np.ones(len(fx["pair_mu"]))
        r = O.element_stats(fx["pair_mu"], fx["pair_sigma"], one, one, 0 * one, 0 * one, 0 * one, 1.0, 1.0)
        assert np.array_equal(r["ALPHA"], fx["pair_alpha"]) and np.array_equal(1 / (r["THETA"] * one + 1), fx["pair_p"])
    assert f.mean() > 0.7
    # relations between the five stored values
    ok = np.isfinite(fx["exact"])
    assert (fx["midp_upper"] <= fx["geq"] * (1 + 1e-15)).all() and (fx["pmf"] <= fx["geq"] * (1 + 1e-15)).all()
    big = fx["geq"] > 1e-300
    np.testing.assert_allclose((fx["geq"] - 0.5 * fx["pmf"])[big], fx["midp_upper"][big], rtol=1e-13, atol=1e-17)
    assert ok.sum() >= len(k) - 12          # NaN only where the reference evaluates betainc(0, ., .): k = 0 at or above the mean


def test_labels_match_the_stored_values(fx, maker):
    k, alpha, p, v, route, path = fx["k"], fx["alpha"], fx["p"], fx["midp_upper"], fx["route"], fx["path"]
    again = np.array([maker.classify(*r) for r in zip(k, alpha, p, v, fx["tail_terms"])])
    assert np.array_equal(again, path)
    assert np.array_equal(route[fx["group"] <= 5], np.where(path >= 0, path, fx["group"])[fx["group"] <= 5])
    assert np.array_equal(route[fx["group"] > 5], fx["group"][fx["group"] > 5])
    with np.errstate(all="ignore"):
        lp0 = alpha * np.log(p)
    R = {n: route == i for i, n in enumerate(fx["route_names"])}
    fast_min = np.where(k <= 64, -400.0, -200.0)
    m = R["fast_accepted"]
    assert (v[m] >= 1e-6).all() and (k[m] <= 128).all() and (lp0[m] > fast_min[m]).all()
    assert {0, 1, 2, 63, 64, 65, 127, 128} <= set(k[m])
    assert ((v[m] < 2e-6).sum() >= 10) and ((v[m] > 0.9).sum() >= 10)
    for centre, sel in ((-400.0, k <= 64), (-200.0, (k > 64) & (k <= 128))):           # both sides of the fast minimum
        assert (m & sel & (lp0 > centre) & (lp0 < 0.99 * centre)).sum() >= 10
        assert (R["slow_recurrence"] & sel & (lp0 <= centre) & (lp0 > 1.01 * centre)).sum() >= 10
    m = R["fast_cancelled"]
    assert (v[m] < 1e-6).all() and (k[m] <= 128).all() and (lp0[m] > fast_min[m]).all() and (v[m] > 5e-7).sum() >= 10
    for decade in (1e-100, 1e-249, 1e-251, 1e-291):
        assert ((v[m] > decade / 3) & (v[m] < decade * 3)).sum() >= 5, decade
    m = R["slow_recurrence"]
    assert (v[m] >= np.where(k[m] <= 256, 1e-6, 1e-4)).all() and (k[m] <= 2048).all() and (lp0[m] > -500).all()
    assert {129, 256, 257, 2047, 2048} <= set(k[m])
    assert (m & (lp0 < -495)).sum() >= 10 and (R["recurrence_skipped"] & (lp0 <= -500) & (lp0 > -505)).sum() >= 10
    m = R["tail_converged"]
    assert (v[m] < np.where(k[m] <= 256, 1e-6, 1e-4)).all() and (v[m] > 1e-290).all()
    assert (fx["tail_terms"][m] > 0).all() and (fx["tail_terms"][m] <= 4096).all()
    assert (m & (k > 256) & (v >= 1e-6)).sum() >= 10                   # 1e-6 .. 1e-4 above k = 256 takes the tail
    assert (fx["tail_terms"][m] > 3500).sum() >= 5                     # close to, and under, 4096 terms
    m = R["tail_nonconvergent"]
    assert ((fx["tail_terms"][m] < 0) | (fx["tail_terms"][m] > 4096) | (v[m] <= 1e-290)).all()
    assert ((alpha[m] <= 1) & (fx["tail_terms"][m] != 0)).sum() >= 40
    m = R["recurrence_skipped"]
    assert ((k[m] > 2048) | (lp0[m] <= -500)).all() and {2049, 4096, 4097, 5000} <= set(k[m])
    x, a, b = 1 - p, k + 1, alpha
    direct = x < (a + 1) / (a + b + 2)                                 # orientation of nb_upper_tail_from_pmf
    assert (m & direct).sum() >= 20 and (m & ~direct).sum() >= 20
    m = R["quad_pmf_source"]
    for kk in (64, 65):
        assert (m & (k == kk) & (lp0 > -690) & (lp0 < -683)).sum() >= 5 and (m & (k == kk) & (lp0 <= -690) & (lp0 > -697)).sum() >= 5
    assert (m & (k == 4096)).sum() >= 5 and (m & (k == 4097)).sum() >= 5
    assert (m & (alpha > 4095) & (alpha <= 4096)).sum() >= 5 and (m & (alpha > 4096) & (alpha < 4097)).sum() >= 5
    m = R["quad_direction"]
    edge = (alpha + k) * x / (k + 1) - 1
    assert (m & (edge > 0) & (edge < 1.1e-3)).sum() >= 20 and (m & (edge < 0) & (edge > -1.1e-3)).sum() >= 20
    assert (m & (alpha < 1) & (alpha > 0.998)).sum() >= 5 and (m & (alpha == 1)).sum() >= 5 and (m & (alpha > 1) & (alpha < 1.002)).sum() >= 5
    down = m & (fx["quad_upper"] == 0)
    assert {1, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 127, 128} <= set(k[down])
    up = fx["quad_blocks"][m & (fx["quad_upper"] == 1)]
    assert (up == 1).any() and (up == 2).any() and ((up == 63) | (up == 64)).any() and (up == 65).any()
    m = R["lower_side"]
    with np.errstate(all="ignore"):
        mu = alpha * (1 - p) / p
    assert (k[m] < mu[m]).all()
    assert (m & (k <= 128) & (lp0 > fast_min)).sum() >= 20                                  # nb_exact_fast
    assert (m & (k <= 128) & (lp0 <= fast_min) & (lp0 > -690)).sum() >= 20                  # nb_lower_cdf_small
    gen = m & ((lp0 <= -690) | (k > 128))                                                   # general betainc
    assert (gen & (lp0 <= -690)).sum() >= 10 and (gen & (k > 128)).sum() >= 20
    direct = p < (alpha + 1) / (alpha + k + 3)
    assert (gen & direct).sum() >= 10 and (gen & ~direct).sum() >= 10
    assert (m & (k == 0)).sum() >= 3 and (m & (k == 1)).sum() >= 3
    m = R["limits"]
    tiny = 2.2250738585072014e-308
    for pp in (1.0, tiny, 2 * tiny, 1 - 2.0 ** -53):
        assert (m & (p == pp)).sum() >= 3, pp
    assert (m & (alpha == 1e6) & (p > 0.999) & (p < 1)).sum() >= 10 and (m & (alpha == 1e-3) & (p > 0.99) & (p < 1)).sum() >= 5
    assert (m & (k == 3000) & (fx["geq"] == 0)).sum() == 1 and (m & (fx["pmf"] > 0) & (fx["pmf"] < tiny)).sum() >= 1


def test_pair_table_covers_the_orderings_and_edges(fx):
    k1, k2, v1, v2 = fx["pair_k1"], fx["pair_k2"], fx["pair_midp_upper1"], fx["pair_midp_upper2"]
    lp0 = fx["pair_alpha"] * np.log(fx["pair_p"])
    assert (k1 < k2).sum() >= 40 and (k1 == k2).sum() >= 40 and (k1 > k2).sum() >= 40
    for a, b in ((128, 129), (64, 65), (10, 100), (0, 128)):
        assert ((k1 == a) & (k2 == b)).sum() >= 5 and ((k1 == b) & (k2 == a)).sum() >= 5, (a, b)
    assert ((np.minimum(k1, k2) == 10) & (np.maximum(k1, k2) == 100) & (np.abs(lp0 + 300) < 1e-6)).sum() >= 2
    small = np.maximum(k1, k2) <= 128
    c1, c2 = v1 < 1e-6, v2 < 1e-6
    assert (small & (c1 != c2)).sum() >= 20 and (small & c1 & c2).sum() >= 20 and (small & ~c1 & ~c2).sum() >= 40
    assert (fx["pair_path1"] >= 0).all() and (fx["pair_path2"] >= 0).all()
