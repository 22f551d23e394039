"""dig_nb_power on the GPU (engine.nb_power: the device form on CUDA tensors, the `_host` twin on numpy arrays) against the table of
tests/test_nb_power_fixture.py -- the reference's own critical counts, demanded EXACTLY on every row (the table keeps only rows whose
statistic stays 1e-6 clear of the level on either side of the crossing), and its powers inside the project's tolerance contract
(nb_power_statement.check_power) --, the two forms against each other bit for bit, and the counts against the route's own test,
dig_nb_midp_upper, on either side of every crossing."""
import numpy as np
import pytest

import nb_power_statement as S
from test_nb_power_fixture import blocks_of, check_counts, load_fixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


def _run(planes, level, scale, folds, k_max, dev=None):
    """engine.nb_power on host arrays (dev None: the twin) or on their device copies; numpy results either way."""
    import torch
    from digdriver_amd import engine
    if dev is None:
        got = engine.nb_power(*planes, level, scale=scale, folds=folds, k_max=k_max)
        return got["k_crit"], got["power"]
    on = lambda x: None if x is None else torch.as_tensor(np.asarray(x, np.float64), device=dev)
    got = engine.nb_power(*[on(x) for x in planes], on(level), scale=on(scale), folds=folds, k_max=k_max)
    assert got["k_crit"].is_cuda and got["k_crit"].dtype == torch.int32
    return got["k_crit"].cpu().numpy(), None if got["power"] is None else got["power"].cpu().numpy()


@pytest.fixture(scope="module")
def golden_runs(fx, dev):
    """The table block by block, each block a plane [1, n] with its level, scale and k_max: {form: (K [N], power [F, N])}."""
    N, F = len(fx["k_crit"]), len(fx["folds"])
    res = {}
    for form, where in (("device", dev), ("twin", None)):
        K, power = np.full(N, -7, np.int32), np.full((F, N), -7.0)
        for rows, level, cj, k_max in blocks_of(fx):
            k, pw = _run([fx[c][rows][None] for c in ("alpha", "theta", "pi")], [level], [cj], fx["folds"], k_max, where)
            assert k.shape == (1, len(rows)) and pw.shape == (F, 1, len(rows))
            K[rows], power[:, rows] = k[0], pw[:, 0]
        res[form] = (K, power)
    return res


@pytest.mark.parametrize("form", ["device", "twin"])
def test_golden_counts_are_exact_and_powers_within_the_contract(fx, golden_runs, form):
    K, power = golden_runs[form]
    check_counts(K, fx, "dig_nb_power, " + form)
    S.check_power(power, fx["power"], fx["k_crit"], "dig_nb_power, " + form)


def test_device_form_and_twin_agree_bit_for_bit_on_the_golden(golden_runs):
    (Kd, pd_), (Kh, ph) = golden_runs["device"], golden_runs["twin"]
    assert Kd.tobytes() == Kh.tobytes() and pd_.tobytes() == ph.tobytes()


@pytest.mark.parametrize("on_device", [True, False], ids=["device", "twin"])
def test_golden_as_planes_of_three_rows_with_a_level_and_a_scale_per_row(fx, golden_runs, dev, on_device):
    """The fifteen regular blocks as five planes [3, 200]: every row of a plane another level AND another scale."""
    b = blocks_of(fx)[:15]                                               # block 3 l + c: level l, scale c
    for j in range(5):
        pick = [b[((j + c) % 5) * 3 + c] for c in range(3)]
        assert len({l for _, l, _, _ in pick}) == 3 and len({c for _, _, c, _ in pick}) == 3 and len({k for _, _, _, k in pick}) == 1
        K, power = _run([np.stack([fx[c][r] for r, _, _, _ in pick]) for c in ("alpha", "theta", "pi")], [l for _, l, _, _ in pick],
                        [c for _, _, c, _ in pick], fx["folds"], pick[0][3], dev if on_device else None)
        for i, (rows, _, _, _) in enumerate(pick):
            check_counts(K[i], fx, "planes [3, n], plane %d row %d" % (j, i), rows=rows)
            # the same bits as the block alone: a pair's result does not depend on its place in the plane
            assert power[:, i].tobytes() == golden_runs["device"][1][:, rows].tobytes()


def _random_planes(rng, R, n):
    """The bench's parameter ranges with hostile values among them: (alpha, theta, pi) f64 [R, n]."""
    mu = np.exp(rng.uniform(np.log(0.05), np.log(500.0), (R, n)))
    sigma = mu * np.exp(rng.uniform(np.log(0.05), np.log(1.5), (R, n)))
    pi = np.exp(rng.uniform(np.log(1e-5), 0.0, (R, n)))
    alpha, theta = mu ** 2 / sigma ** 2, sigma ** 2 / mu
    for x, v in ((alpha, np.nan), (theta, -1.0), (pi, 0.0), (pi, np.nan), (alpha, np.inf), (theta, 0.0)):
        x[rng.uniform(size=x.shape) < 0.02] = v
    return alpha, theta, pi


def test_device_form_against_twin_bit_for_bit_over_sizes_rows_and_folds(dev):
    rng = np.random.default_rng(20261021)
    levels, scales = np.array([0.05, 1e-6, 1e-12]), np.array([0.7, 3.0, 0.2])
    for n in (0, 1, 63, 64, 65, 257):
        for R in (1, 3):
            planes = _random_planes(rng, R, n)
            for F in (0, 1, 8):
                folds = (2.0, 5.0, 10.0, 100.0, 0.5, 1.0, 3.0, 1.5)[:F]
                Kd, pd_ = _run(planes, levels[:R], scales[:R], folds, 1 << 12, dev)
                Kh, ph = _run(planes, levels[:R], scales[:R], folds, 1 << 12, None)
                assert Kd.shape == (R, n) and Kd.tobytes() == Kh.tobytes(), (n, R, F)
                if F == 0:
                    assert pd_ is None and ph is None
                else:
                    assert pd_.shape == (F, R, n) and pd_.tobytes() == ph.tobytes(), (n, R, F)
                    assert ((Kd >= 0) | (pd_ == 0) | np.isnan(pd_)).all() and (pd_[:, Kd == 0] == 1.0).all()


def test_no_scale_is_a_scale_of_ones_and_a_vector_is_one_row(dev):
    rng = np.random.default_rng(7)
    planes = _random_planes(rng, 3, 257)
    levels, folds = [0.05, 1e-3, 1e-6], (2.0, 10.0)
    for where in (dev, None):
        K0, p0 = _run(planes, levels, None, folds, 1 << 12, where)
        K1, p1 = _run(planes, levels, np.ones(3), folds, 1 << 12, where)
        assert K0.tobytes() == K1.tobytes() and p0.tobytes() == p1.tobytes()
        Kv, pv = _run([x[1] for x in planes], levels[1], None, folds, 1 << 12, where)
        assert Kv.shape == (257,) and pv.shape == (2, 257) and Kv.tobytes() == K0[1].tobytes() and pv.tobytes() == p0[:, 1].tobytes()


def test_counts_are_consistent_with_the_routes_own_test_at_fold_one(fx, golden_runs, dev):
    """For every row with K >= 0: dig_nb_midp_upper at (K, alpha, p(1)) <= level (1 + 1e-6), and at K - 1 (where K > 0) > level
    (1 - 1e-6) -- the statistic the element route tests with, on either side of the crossing the kernel reports."""
    import torch
    from digdriver_amd.sequence_model import nb_model
    K = golden_runs["device"][0]
    at = np.flatnonzero(K >= 0)
    p1 = S.success_prob(fx["theta"][at], fx["pi"][at], 1.0, fx["cj"][at])
    on = lambda x: torch.as_tensor(x, device=dev)
    m_at = nb_model.nb_pvalue_greater_midp(on(K[at].astype(np.float64)), on(fx["alpha"][at]), on(p1)).cpu().numpy()
    level = fx["level"][at]
    print("M(K) / level: largest %.9g" % float((m_at / level).max()))
    assert (m_at <= level * (1 + 1e-6)).all()
    below = K[at] > 0
    m_below = nb_model.nb_pvalue_greater_midp(on(K[at][below] - 1.0), on(fx["alpha"][at][below]), on(p1[below])).cpu().numpy()
    print("M(K - 1) / level: smallest %.9g" % float((m_below / level[below]).min()))
    assert (m_below > level[below] * (1 - 1e-6)).all()
    # ... and the power at fold 1 is the project's own upper tail at K
    g = nb_model.nb_pvalue_greater(on(K[at].astype(np.float64)), on(fx["alpha"][at]), on(p1)).cpu().numpy()
    assert g.tobytes() == golden_runs["device"][1][0, at].tobytes()


def test_nb_critical_count_is_the_one_array_form(dev):
    """nb_model.nb_critical_count(alpha, p, level): engine.nb_power with theta = (1 - p) / p and pi = 1, device tensors and host arrays."""
    import torch
    from digdriver_amd import engine
    from digdriver_amd.sequence_model import nb_model
    rng = np.random.default_rng(3)
    alpha, p = rng.uniform(0.2, 30.0, 300), rng.uniform(0.01, 0.99, 300)
    want = engine.nb_power(alpha, (1.0 - p) / p, np.ones(300), 1e-3, k_max=1 << 16)["k_crit"]
    got = nb_model.nb_critical_count(alpha, p, 1e-3, k_max=1 << 16)
    assert got.dtype == np.int32 and np.array_equal(got, want) and (got > 0).all()
    got_d = nb_model.nb_critical_count(torch.as_tensor(alpha, device=dev), torch.as_tensor(p, device=dev), 1e-3, k_max=1 << 16)
    assert got_d.is_cuda and np.array_equal(got_d.cpu().numpy(), want)
