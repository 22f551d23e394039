"""GPU parity tests: the HIP path (through the C ABI of libdig_hip.so) against
  (a) the committed golden vectors produced by the real reference, and
  (b) the oracle on seeded inputs,
plus size-independent properties at BASELINE-scale sizes.

Tolerance contract (BASELINE.json north_star / SURVEY 8c): p-values and expected counts within
1e-6 relative for p >= 1e-250 (below that scipy itself is not self-consistent: both sides must be
< 1e-250); integer outputs bit-exact.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, rel_close

pytestmark = pytest.mark.gpu

RTOL = 1e-6


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------
# NB family vs reference goldens
# ---------------------------------------------------------------------------------------
def test_nb_midp_upper_golden_host_and_device(torch_dev):
    import torch
    from digdriver_amd.sequence_model import nb_model
    d = np.load(os.path.join(GOLDEN, "nb_midp_golden.npz"))
    got = nb_model.nb_pvalue_greater_midp(d["k"], d["alpha"], d["p"])
    rel_close(got, d["pval"], RTOL)
    # device-pointer entry point on torch tensors: same kernel, no copies
    t = [torch.as_tensor(d[n], device=torch_dev) for n in ("k", "alpha", "p")]
    got_dev = nb_model.nb_pvalue_greater_midp(*t)
    assert got_dev.is_cuda
    assert np.array_equal(got_dev.cpu().numpy(), got, equal_nan=True)
    # SURVEY 8c spot values
    spot = nb_model.nb_pvalue_greater_midp(d["spot_k"], d["spot_alpha"], 1 / (d["spot_theta"] * d["spot_pi"] + 1))
    rel_close(spot, d["spot_pval"], RTOL)
    # edge conventions measured with the reference
    e = nb_model.nb_pvalue_greater_midp(np.array([0., 0., 3., 2., 2., 2.]), np.array([2.5, 4., 4., 4., 0., np.nan]),
                                       np.array([0.3, 1.0, 1.0, 1.2, .5, .5]))
    assert e[0] == pytest.approx(0.5 * 0.3 ** 2.5 + 1 - 0.3 ** 2.5, rel=1e-13)
    assert e[1] == 0.5 and e[2] == 0.0 and np.isnan(e[3]) and np.isnan(e[4]) and np.isnan(e[5])


def test_nb_wide_parameter_sweep_vs_scipy(torch_dev):
    """Far outside the workload's ranges: alpha 1e-3 .. 1e6, p 1e-9 .. 1 - 1e-12, k 0 .. 1e5 (fast recurrence, rescaled
    recurrence, tail series and the lgamma + continued-fraction fallback all get traffic), against the scipy expressions the
    reference evaluates (oracle), under the tolerance contract."""
    from digdriver_amd.sequence_model import nb_model
    from oracle import dig_oracle as O
    rng = np.random.default_rng(77)
    n = 120_000
    alpha = 10.0 ** rng.uniform(-3, 6, n)
    p = np.where(rng.uniform(size=n) < 0.5, 10.0 ** rng.uniform(-9, 0, n), 1.0 - 10.0 ** rng.uniform(-12, 0, n))
    p = np.clip(p, 1e-9, 1.0)
    mean = alpha * (1 - p) / p
    kind = rng.integers(0, 4, n)
    with np.errstate(all="ignore"):
        k = np.where(kind == 0, rng.poisson(np.minimum(mean, 5e4)),                       # near the mean
            np.where(kind == 1, np.floor(np.minimum(mean, 2e4) * rng.uniform(1, 6, n) + rng.integers(0, 30, n)),   # upper tail
            np.where(kind == 2, rng.integers(0, 70, n), rng.integers(0, 100_000, n)))).astype(float)
    with np.errstate(all="ignore"):
        want = O.nb_pvalue_greater_midp(k, alpha, p)
    got = nb_model.nb_pvalue_greater_midp(k, alpha, p)
    rel_close(got, want, RTOL)
    with np.errstate(all="ignore"):
        rel_close(nb_model.nb_pvalue_exact(k, alpha, p), O.nb_pvalue_exact(k, alpha, p), RTOL)
        rel_close(nb_model.nb_pvalue_greater(k, alpha, p), O.nb_pvalue_greater(k, alpha, p), RTOL)


def test_nb_scalar_siblings_golden(torch_dev):
    from digdriver_amd.sequence_model import nb_model
    d = np.load(os.path.join(GOLDEN, "nb_exact_golden.npz"))
    rel_close(nb_model.nb_pvalue_exact(d["k"], d["alpha"], d["p"]), d["pval_exact"], RTOL)
    rel_close(nb_model.nb_pvalue_greater(d["k"], d["alpha"], d["p"]), d["pval_greater"], RTOL)
    rel_close(nb_model.nb_pvalue_midp(d["k"], d["alpha"], d["p"]), d["pval_midp"], RTOL)
    assert nb_model.nb_pvalue_exact(0, 4, .5) == pytest.approx(0.0625, rel=1e-13)
    assert nb_model.nb_pvalue_exact(10, 4, .5) == pytest.approx(0.046142578125, rel=1e-12)
    assert nb_model.nb_pvalue_exact(4, 4, .5) == pytest.approx(0.5, rel=1e-12)
    assert nb_model.nb_pvalue_exact(3000, 4, .5) == 0.0


def test_fisher_and_gamma(torch_dev):
    from digdriver_amd.sequence_model import nb_model
    d = np.load(os.path.join(GOLDEN, "fisher_golden.npz"))
    rel_close(nb_model.fisher_combine(d["p1"], d["p2"]), d["out"], 1e-12)
    assert nb_model.fisher_combine(1e-3, 0.5) == pytest.approx(0.004300451229771043, rel=1e-13)
    e = np.load(os.path.join(GOLDEN, "element_stats_golden.npz"))
    a, t = nb_model.normal_params_to_gamma(e["mu"], e["sigma"])
    assert np.array_equal(a, e["out_ALPHA"], equal_nan=True)         # bit-exact: same IEEE operations
    with np.errstate(all="ignore"):
        assert np.array_equal(t * float(e["cj"]), e["out_THETA"], equal_nan=True)


# ---------------------------------------------------------------------------------------
# element statistics block
# ---------------------------------------------------------------------------------------
def _element_obs(d):
    pres = d["present"]
    return [np.where(pres, d["tab_" + k], 0).astype(np.int32) for k in ("obs_snv", "obs_samples", "obs_indel")]


def test_element_stats_golden(torch_dev):
    import torch
    from digdriver_amd import engine
    d = np.load(os.path.join(GOLDEN, "element_stats_golden.npz"))
    obs = _element_obs(d)
    r = engine.element_stats(d["mu"], d["sigma"], d["pi_sum"], d["pi_indel"], *obs, float(d["cj"]), float(d["cj_indel"]))
    for name in engine.ES_PLANES:
        rel_close(r[name][:, 0], d["out_" + name], RTOL)
    # EXP_SNV / THETA_INDEL / EXP_INDEL are plain products: bit-exact
    for name in ("EXP_SNV", "THETA_INDEL", "EXP_INDEL"):
        assert np.array_equal(r[name][:, 0], d["out_" + name], equal_nan=True), name
    # device path, 3 cohorts with different scale factors == three host calls
    E = len(d["mu"])
    cjs, cjis = np.array([float(d["cj"]), 0.4, 2.2]), np.array([float(d["cj_indel"]), 0.2, 0.01])
    rep = lambda v: torch.as_tensor(np.repeat(np.asarray(v)[:, None], 3, axis=1), device=torch_dev)
    rd = engine.element_stats(rep(d["mu"]), rep(d["sigma"]), rep(d["pi_sum"]), torch.as_tensor(d["pi_indel"], device=torch_dev),
                              rep(obs[0]), rep(obs[1]), rep(obs[2]), torch.as_tensor(cjs, device=torch_dev),
                              torch.as_tensor(cjis, device=torch_dev))
    for c in range(3):
        rh = engine.element_stats(d["mu"], d["sigma"], d["pi_sum"], d["pi_indel"], *obs, cjs[c], cjis[c])
        for name in engine.ES_PLANES:
            assert np.array_equal(rd[name][:, c].cpu().numpy(), rh[name][:, 0], equal_nan=True), (name, c)


def test_element_stats_vs_oracle_random_cohorts(torch_dev):
    from digdriver_amd import engine
    from oracle import dig_oracle as O
    rng = np.random.default_rng(5)
    E, C = 4000, 37
    mu = np.exp(rng.uniform(np.log(0.05), np.log(500.0), (E, C)))
    sigma = mu * np.exp(rng.uniform(np.log(0.05), np.log(1.5), (E, C)))
    pi = np.exp(rng.uniform(np.log(1e-5), np.log(1.0), (E, C)))
    pii = np.exp(rng.uniform(np.log(1e-5), np.log(1.0), E))
    cj, cji = rng.uniform(0.2, 3, C), rng.uniform(0.01, 0.5, C)
    lam = mu * cj * pi
    k1 = rng.poisson(lam * np.exp(rng.normal(0, 1, (E, C)))).astype(np.int32)
    k2 = rng.binomial(k1, 0.9).astype(np.int32)
    k3 = rng.poisson(mu * cji * pii[:, None]).astype(np.int32)
    mui, sgi = mu * rng.uniform(0.5, 2, (E, C)), sigma * rng.uniform(0.5, 2, (E, C))
    got = engine.element_stats(mu, sigma, pi, pii, k1, k2, k3, cj, cji, mu_indel=mui, sigma_indel=sgi)
    want = O.element_stats(mu, sigma, pi, pii[:, None], k1, k2, k3, cj[None, :], cji[None, :], mu_indel=mui, sigma_indel=sgi)
    for name in engine.ES_PLANES:
        rel_close(got[name], want[name], RTOL)
    # worklist (two-pass) and inline (single-pass) modes: identical bits for every test the streaming pass resolves; the
    # tests it leaves open are summed by eight lanes in the compacted pass and by one lane inline -- same value, another
    # order of additions
    import torch
    dev = torch.device("cuda:0")
    tt = lambda v: torch.as_tensor(v, device=dev)
    a = engine.element_stats(tt(mu), tt(sigma), tt(pi), tt(pii), tt(k1), tt(k2), tt(k3), tt(cj), tt(cji))
    b = engine.element_stats(tt(mu), tt(sigma), tt(pi), tt(pii), tt(k1), tt(k2), tt(k3), tt(cj), tt(cji), use_workspace=False)
    n_equal = 0
    for name in engine.ES_PLANES:
        x, y = a[name].cpu().numpy(), b[name].cpu().numpy()
        if name.startswith("PVAL"):
            rel_close(x, y, 1e-6)                               # (the inline form accepts 1 - CDF down to 1e-6: up to 2e-7 of cancellation)
            n_equal += int((x == y).sum())
        else:
            assert np.array_equal(x, y, equal_nan=True), name
    assert n_equal > 0.9 * 4 * E * C                       # (the open tests are a small minority)
    # empty problem is a no-op
    r = engine.element_stats(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), np.zeros((0, 3), np.int32),
                             np.zeros((0, 3), np.int32), np.zeros((0, 3), np.int32), np.ones(3), np.ones(3))
    assert r["EXP_SNV"].shape == (0, 3)


def test_elementwise_entry_points_wide_range_vs_oracle():
    """nb_pvalue_greater_midp / greater / exact / two-sided mid-p far outside the fixtures (tools/stress_elementwise.py is the
    multi-seed form): counts up to 2e6, alpha 1e-2 .. 1e6.  scipy's lgamma expressions for the pmf and for the prefactor of
    the incomplete beta are 2e-6 off at counts of 1e6; the device uses Loader's saddle-point forms."""
    from digdriver_amd.sequence_model import nb_model as M
    from oracle import dig_oracle as O
    rng = np.random.default_rng(5)
    n = 60_000
    mean = 10 ** rng.uniform(-2, 5, n)
    alpha = 10 ** rng.uniform(-2, 6, n)
    p = alpha / (alpha + mean)
    k = np.clip(np.rint(mean + rng.uniform(-4, 14, n) * np.sqrt(mean / p)), 0, 2e6)
    for name in ("nb_pvalue_greater_midp", "nb_pvalue_greater", "nb_pvalue_exact", "nb_pvalue_midp"):
        rel_close(getattr(M, name)(k, alpha, p), getattr(O, name)(k, alpha, p), RTOL)


def test_element_stats_wide_range_vs_oracle():
    """Far outside the fixtures: rates 1e-2 .. 1e5, dispersion alpha 1e-2 .. 1e6, counts from four standard deviations below
    the mean to fourteen above (up to 2e6) -- the compacted pass's series, its saddle-point pmf and the scalar fallbacks
    (heavy tails at alpha << 1, counts beyond the recurrence) all inside the 1e-6 contract (tools/stress_stats.py is the
    multi-seed form of this test; scipy's own lgamma form of the pmf would be off by 2e-6 at counts of 1e6)."""
    from digdriver_amd import engine
    from oracle import dig_oracle as O
    rng = np.random.default_rng(21)
    E, C = 2500, 37
    mean = 10 ** rng.uniform(-2, 5, (E, C))
    alpha = 10 ** rng.uniform(-2, 6, (E, C))
    mu, sigma = mean, mean / np.sqrt(alpha)
    sd = np.sqrt(mean * (1 + mean / alpha))
    k1 = np.clip(np.rint(mean + rng.uniform(-4, 14, (E, C)) * sd), 0, 2e6).astype(np.int32)
    k2 = np.clip(np.rint(k1 * rng.uniform(0.5, 1.0, (E, C))), 0, None).astype(np.int32)
    k3 = np.clip(np.rint(mean + rng.uniform(-3, 8, (E, C)) * sd), 0, 2e6).astype(np.int32)
    one = np.ones((E, C))
    got = engine.element_stats(mu, sigma, one, np.ones(E), k1, k2, k3, np.ones(C), np.ones(C))
    want = O.element_stats(mu, sigma, one, np.ones((E, 1)), k1, k2, k3, np.ones((1, C)), np.ones((1, C)))
    for name in engine.ES_PLANES:
        rel_close(got[name], want[name], RTOL)



# ---------------------------------------------------------------------------------------
# per-element accumulation vs the reference's own loops (goldens)
# ---------------------------------------------------------------------------------------
def _sorted_dpr(freq):
    from oracle import dig_oracle as O
    return freq[O.model_rows_to_sorted_perm()][None, :]


def _csr(ovp):
    ptr = np.concatenate([[0], np.cumsum((ovp >= 0).sum(axis=1))]).astype(np.int64)
    return ptr, ovp[ovp >= 0].astype(np.int32)


def test_accumulate_nonc_model_golden(torch_dev):
    from digdriver_amd import engine
    d = np.load(os.path.join(GOLDEN, "accumulate_golden.npz"))
    ptr, idx = _csr(d["elt_overlap_bins"])
    r = engine.accumulate_elements(d["bin_y_pred"], d["bin_std"], d["bin_y_true"], d["bin_flag"], d["bin_ctx"], ptr, idx,
                                   d["elt_L"].astype(np.int32), (d["elt_strand"] == "-"), _sorted_dpr(d["seq_freq"]))
    col = {c: i for i, c in enumerate(d["out_cols"])}
    v = d["out_vals"]
    rel_close(r["MU"][:, 0], v[:, col["MU"]], 1e-12)
    rel_close(r["SIGMA"][:, 0], v[:, col["SIGMA"]], 1e-12)
    rel_close(r["P"][:, 0, 0], v[:, col["P_SUM"]], 1e-11)
    rel_close(r["P_INDEL"], v[:, col["P_INDEL"]], 1e-15)
    for name in ("R_OBS", "FLAG"):
        assert np.array_equal(r[name][:, 0], v[:, col[name]].astype(np.int32)), name
    for name in ("R_SIZE", "ELT_SIZE"):
        assert np.array_equal(r[name], v[:, col[name]].astype(np.int32)), name


def test_zero_denominators_with_zeros_in_the_frequency_table(torch_dev):
    """The one known output difference of rounds 3-4, closed: a cohort whose FREQ table is exactly zero at
    every context an element's bins hold has sum(region_counts * d_pr) == 0 AND 0 / 0 in t_pi, so the reference's P_SUM is NaN
    whatever L is (genic_driver_tools.py:361-366; rounds 3-4 said inf when L held no zero).  Golden: the reference's own
    nonc_model (accumulate_zero_golden.npz), three tables as three cohorts of ONE call -- general form, the no-workspace form
    and the compact pipeline form (the cohort test runs only on the zero-denominator path)."""
    import torch
    from digdriver_amd import engine
    from oracle import dig_oracle as O
    d = np.load(os.path.join(GOLDEN, "accumulate_zero_golden.npz"))
    ptr, idx = _csr(d["elt_overlap_bins"])
    C = d["seq_freq"].shape[0]
    E = len(d["elt_L"])
    rep = lambda v: np.ascontiguousarray(np.repeat(np.asarray(v)[:, None], C, axis=1))
    d_pr = np.ascontiguousarray(d["seq_freq"][:, O.model_rows_to_sorted_perm()])
    want = d["p_sum"].T                                   # [E, 3 tables]
    assert np.isnan(want[:, 1]).sum() >= 8
    ins = (rep(d["bin_y_pred"]), rep(d["bin_std"]), rep(d["bin_y_true"]).astype(np.int32), rep(d["bin_flag"]).astype(np.uint8),
           d["bin_ctx"].astype(np.int32), ptr, idx, d["elt_L"].astype(np.int32), (d["elt_strand"] == "-"), d_pr)

    def check(P, what):
        P = np.asarray(P)
        assert np.array_equal(np.isnan(P), np.isnan(want)), what
        ok = ~np.isnan(want)
        rel_close(P[ok], want[ok], 1e-11)

    r = engine.accumulate_elements(*ins)
    check(r["P"][:, 0, :], "general form")
    td = [torch.as_tensor(np.ascontiguousarray(x), device=torch_dev) for x in ins]
    zeros = torch.zeros((E, C), dtype=torch.int32, device=torch_dev)
    one = torch.ones(C, dtype=torch.float64, device=torch_dev)
    plan = engine.PipelinePlan(*td, zeros, zeros, zeros)
    assert plan.compact
    acc, _ = plan.run(one, one)
    torch.cuda.synchronize()
    check(acc["P"].cpu().numpy().reshape(E, C), "compact pipeline form")
    plan_g = engine.PipelinePlan(*td, zeros, zeros, zeros, compact=False)
    acc, _ = plan_g.run(one, one)
    torch.cuda.synchronize()
    check(acc["P"].cpu().numpy().reshape(E, C), "general pipeline form")
    # more cohorts than one 16-column tile and the 4-column quads: the three tables cycled over 37 cohorts
    C2 = 37
    cyc = np.arange(C2) % C
    ins2 = (np.ascontiguousarray(ins[0][:, cyc]), np.ascontiguousarray(ins[1][:, cyc]), np.ascontiguousarray(ins[2][:, cyc]),
            np.ascontiguousarray(ins[3][:, cyc]), ins[4], ptr, idx, ins[7], ins[8], np.ascontiguousarray(d_pr[cyc]))
    td2 = [torch.as_tensor(np.ascontiguousarray(x), device=torch_dev) for x in ins2]
    z2 = torch.zeros((E, C2), dtype=torch.int32, device=torch_dev)
    o2 = torch.ones(C2, dtype=torch.float64, device=torch_dev)
    for compact in ("auto", False):
        acc, _ = engine.PipelinePlan(*td2, z2, z2, z2, compact=compact).run(o2, o2)
        torch.cuda.synchronize()
        P = acc["P"].cpu().numpy().reshape(E, C2)
        assert np.array_equal(np.isnan(P), np.isnan(want[:, cyc])), compact
        ok = ~np.isnan(want[:, cyc])
        rel_close(P[ok], want[:, cyc][ok], 1e-11)


def test_accumulate_tiled_and_genic_golden(torch_dev):
    from digdriver_amd import engine
    d = np.load(os.path.join(GOLDEN, "accumulate_golden.npz"))
    window = int(d["window"])
    bin_index = {(int(c), int(s)): i for i, (c, s, _) in enumerate(d["bin_idx"])}
    rows = [bin_index[(int(n.split(":")[0][3:]), int(n.split(":")[1].split("-")[0]) // window * window)]
            for n in d["tile_names"]]
    T = len(rows)
    r = engine.accumulate_elements(d["bin_y_pred"], d["bin_std"], d["bin_y_true"], d["bin_flag"], d["bin_ctx"],
                                   np.arange(T + 1), np.array(rows), d["tile_L"].astype(np.int32), np.zeros(T, bool),
                                   _sorted_dpr(d["seq_freq"]))
    col = {c: i for i, c in enumerate(d["out_cols"])}
    v = d["tile_out_vals"]
    rel_close(r["MU"][:, 0], v[:, col["MU"]], 1e-12)
    rel_close(r["P"][:, 0, 0], v[:, col["P_SUM"]], 1e-11)
    assert np.array_equal(r["ELT_SIZE"], v[:, col["ELT_SIZE"]].astype(np.int32))
    assert np.array_equal(r["FLAG"][:, 0], v[:, col["FLAG"]].astype(np.int32))

    g = np.load(os.path.join(GOLDEN, "genic_golden.npz"))
    ptr, idx = _csr(g["gene_overlap_bins"])
    glen = ((g["cds_ends"] - g["cds_starts"] + 1) * (g["cds_starts"] >= 0)).sum(axis=1)
    G = len(glen)
    r = engine.accumulate_elements(d["bin_y_pred"], d["bin_std"], d["bin_y_true"], d["bin_flag"], d["bin_ctx"], ptr, idx,
                                   g["L_data"].astype(np.int32), np.zeros(G, bool), _sorted_dpr(d["seq_freq"]),
                                   gene_length=glen)
    col = {c: i for i, c in enumerate(g["out_cols"])}
    v = g["out_vals"]
    rel_close(r["MU"][:, 0], v[:, col["MU"]], 1e-12)
    rel_close(r["SIGMA"][:, 0], v[:, col["SIGMA"]], 1e-12)
    for q, name in enumerate(["P_SILENT", "P_MIS", "P_NONS", "P_SPLICE"]):
        rel_close(r["P"][:, q, 0], v[:, col[name]], 1e-11)
    rel_close(r["P_INDEL"], v[:, col["P_INDEL"]], 1e-15)
    assert np.array_equal(r["R_SIZE"], v[:, col["R_SIZE"]].astype(np.int32))
    assert np.array_equal(r["R_OBS"][:, 0], v[:, col["R_OBS"]].astype(np.int32))
    assert np.array_equal(r["FLAG"][:, 0], v[:, col["FLAG"]].astype(np.int32))


def _accumulate_vs_oracle(torch_dev, C, E):
    import torch
    from bench import make_workload
    from digdriver_amd import engine
    from oracle import dig_oracle as O
    w = make_workload(n_bins=900, n_elements=E, n_cohorts=C, seed=11 + C)
    # a few ragged cases: an element with no overlapped bin and one with many
    w["ov_ptr"] = w["ov_ptr"].copy()
    td = {k: torch.as_tensor(v, device=torch_dev) for k, v in w.items() if isinstance(v, np.ndarray)}
    got = engine.accumulate_elements(td["bin_mu"], td["bin_std"], td["bin_y"], td["bin_flag"], td["bin_ctx"], td["ov_ptr"],
                                     td["ov_idx"], td["L"], td["strand_minus"], td["d_pr"])
    want = O.accumulate_elements(w["bin_mu"], w["bin_std"], w["bin_y"], w["bin_flag"], w["bin_ctx"], w["ov_ptr"],
                                 w["ov_idx"], w["L"], w["strand_minus"].astype(bool), w["d_pr"])
    rel_close(got["MU"].cpu().numpy(), want["MU"], 1e-12)
    rel_close(got["SIGMA"].cpu().numpy(), want["SIGMA"], 1e-12)
    rel_close(got["P"].cpu().numpy(), want["P"], 1e-11)
    rel_close(got["P_INDEL"].cpu().numpy(), want["P_INDEL"], 1e-15)
    for name in ("R_OBS", "FLAG", "R_SIZE", "ELT_SIZE"):
        assert np.array_equal(got[name].cpu().numpy(), want[name]), name
    # the no-workspace (single-kernel LDS) variant agrees with the workspace (two-kernel) variant
    v1 = engine.accumulate_elements(td["bin_mu"], td["bin_std"], td["bin_y"], td["bin_flag"], td["bin_ctx"], td["ov_ptr"],
                                    td["ov_idx"], td["L"], td["strand_minus"], td["d_pr"], use_workspace=False)
    for name in ("MU", "SIGMA", "P", "P_INDEL"):
        rel_close(v1[name].cpu().numpy(), got[name].cpu().numpy(), 1e-12)
    for name in ("R_OBS", "FLAG", "R_SIZE", "ELT_SIZE"):
        assert torch.equal(v1[name], got[name]), name
    # host twin == device path bit for bit
    host = engine.accumulate_elements(w["bin_mu"], w["bin_std"], w["bin_y"], w["bin_flag"], w["bin_ctx"], w["ov_ptr"],
                                      w["ov_idx"], w["L"], w["strand_minus"], w["d_pr"])
    for name in got:
        assert np.array_equal(host[name], got[name].cpu().numpy(), equal_nan=True), name
    return w, td, got, want


@pytest.mark.parametrize("C", [1, 5, 12, 20, 33, 37, 48, 64, 70, 104])
def test_accumulate_vs_oracle_multi_cohort(torch_dev, C):
    _accumulate_vs_oracle(torch_dev, C, 700)


@pytest.mark.parametrize("C", [1, 4, 5, 8, 9, 16, 17, 21, 24, 25, 32, 33, 37, 40, 41, 48, 49, 85])
def test_accumulate_and_compact_pipeline_at_every_cohort_cut(torch_dev, C):
    """All nine (tiles, quads) cuts of a 48-cohort chunk, and two chunks, through both dot kernels: dig_accumulate_elements
    (acc_dot_mfma_kernel) as above, and the compact pipeline (acc_dot_ctx_kernel) against it with the comparison of
    test_compact_pipeline_against_general_form_and_oracle.  E = 33: two full 16-row tiles and one row."""
    import torch
    from digdriver_amd import engine
    w, td, got, want = _accumulate_vs_oracle(torch_dev, C, 33)
    plan = engine.PipelinePlan(td["bin_mu"], td["bin_std"], td["bin_y"], td["bin_flag"], td["bin_ctx"], td["ov_ptr"], td["ov_idx"],
                               td["L"], td["strand_minus"], td["d_pr"], td["obs_snv"], td["obs_samples"], td["obs_indel"])
    assert plan.compact, "make_workload repeats every context count three times"
    acc_c, _ = plan.run(td["cj"], td["cj_indel"])
    torch.cuda.synchronize()
    for k in ("MU", "SIGMA", "R_OBS", "FLAG", "R_SIZE", "ELT_SIZE", "P_INDEL"):
        assert torch.equal(torch.nan_to_num(got[k].double(), nan=-7.0), torch.nan_to_num(acc_c[k].double(), nan=-7.0)), k
    pg, pc = got["P"].cpu().numpy(), acc_c["P"].cpu().numpy()
    assert (np.isnan(pg) == np.isnan(pc)).all()
    ok = np.isfinite(pg)
    assert np.array_equal(pc[~ok & ~np.isnan(pg)], pg[~ok & ~np.isnan(pg)])
    assert (np.abs(pc[ok] / pg[ok] - 1) <= 1e-13).all()
    rel_close(pc, want["P"], 1e-11)


def test_scale_suffstats(torch_dev):
    import torch
    from digdriver_amd import engine
    from oracle import dig_oracle as O
    rng = np.random.default_rng(2)
    for N, C in [(1, 1), (1000, 37), (4097, 64), (300, 300), (70000, 3)]:
        mu = rng.gamma(9.0, 3.0, (N, C))
        flag = (rng.uniform(size=(N, C)) < 0.1).astype(np.uint8)
        got = engine.scale_suffstats(mu, flag)
        want = np.array([O.scale_factor_genome(mu[:, c], flag[:, c], 1.0, 1.0)[0] for c in range(C)])
        np.testing.assert_allclose(1.0 / got, want, rtol=1e-12)
        dev = engine.scale_suffstats(torch.as_tensor(mu, device=torch_dev), torch.as_tensor(flag, device=torch_dev))
        assert np.array_equal(dev.cpu().numpy(), got)                    # deterministic order
        again = engine.scale_suffstats(torch.as_tensor(mu, device=torch_dev), torch.as_tensor(flag, device=torch_dev))
        assert torch.equal(dev, again)


# ---------------------------------------------------------------------------------------
# gather and tiles
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", ["f32", "f64", "i16"])
def test_gather_bins(torch_dev, src):
    import torch
    from digdriver_amd import engine
    from oracle import dig_oracle as O
    rng = np.random.default_rng(4)
    N, L, T = 50, 100, 77
    x = np.round(rng.uniform(0, 1, (N, L, T)), 2) * 100
    x = x.astype({"f32": np.float32, "f64": np.float64, "i16": np.int16}[src])
    rows = rng.integers(0, N, 23)
    tracks = np.concatenate([np.arange(3, 40), [1, 70, 76, 5]])
    want = O.gather_bins(x, rows, tracks)
    got = engine.gather_bins(x, rows, tracks)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    got_t = engine.gather_bins(x, rows, tracks, transpose=True)
    assert np.array_equal(got_t, want.transpose(0, 2, 1))
    xd = torch.as_tensor(x, device=torch_dev)
    assert np.array_equal(engine.gather_bins(xd, rows, None).cpu().numpy(), x[rows].astype(np.float32))
    b = engine.gather_bins(xd, rows, tracks, out_dtype="bf16", transpose=True)
    assert b.dtype == torch.bfloat16
    np.testing.assert_allclose(b.float().cpu().numpy(), want.transpose(0, 2, 1), rtol=2 ** -8)
    assert engine.gather_bins(x, np.zeros(0, np.int64), tracks).shape == (0, L, len(tracks))
    # all tracks (tracks=None -> NULL): the contiguous block copy, its bf16 form, the channels-first form, the host twin,
    # and a bin size that is not a multiple of four values (falls back to the row kernel)
    full = x[rows].astype(np.float32)
    assert np.array_equal(engine.gather_bins(x, rows, None), full)
    assert np.array_equal(engine.gather_bins(xd, rows, None, transpose=True).cpu().numpy(), full.transpose(0, 2, 1))
    bf = engine.gather_bins(xd, rows, None, out_dtype="bf16")
    assert bf.dtype == torch.bfloat16 and torch.equal(bf, torch.as_tensor(full, device=torch_dev).to(torch.bfloat16))
    xo = np.ascontiguousarray(x[:, :99, :])
    assert np.array_equal(engine.gather_bins(torch.as_tensor(xo, device=torch_dev), rows, None).cpu().numpy(),
                          xo[rows].astype(np.float32))
    big = rng.integers(0, N, 700)                      # many bins; still inside one pass of the block kernel's grid (65 535 bins
                                                       # in y): test_gpu_grid_wrap.py goes past it
    assert np.array_equal(engine.gather_bins(xd, big, None).cpu().numpy(), x[big].astype(np.float32))


@pytest.mark.parametrize("src", ["i16", "f32", "f64"])
def test_gather_track_subset_wide_and_row_forms(torch_dev, src):
    """A track-selection file (dataset_generator.py:57-80) with a multiple of four tracks: the wide subset kernel (groups of
    rows as 8-byte aligned blocks through LDS) for every source type, odd and even track counts, f32 and bf16 outputs; shapes
    it does not take (L not a multiple of the group, T beyond its LDS block) go through the row kernel -- all against the
    oracle's x_data[rows][:, :, tracks]."""
    import torch
    from digdriver_amd import engine
    from oracle import dig_oracle as O
    rng = np.random.default_rng(9)
    dt = {"f32": np.float32, "f64": np.float64, "i16": np.int16}[src]
    for (N, L, T, n_sel) in ((37, 100, 77, 44), (20, 100, 735, 512), (11, 100, 64, 64), (9, 99, 77, 40), (5, 100, 1100, 16), (3, 4, 8, 8)):
        x = (np.round(rng.uniform(0, 1, (N, L, T)), 2) * 100).astype(dt)
        rows = rng.integers(0, N, 19)
        tracks = np.sort(rng.permutation(T)[:n_sel]).astype(np.int32)
        tracks[:2] = tracks[:2][::-1]                       # not sorted everywhere: the order of the list is the order of the output
        want = O.gather_bins(x, rows, tracks)
        xd = torch.as_tensor(x, device=torch_dev)
        got = engine.gather_bins(xd, rows, tracks)
        assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want), (N, L, T, n_sel)
        if n_sel % 8 == 0:
            b = engine.gather_bins(xd, rows, tracks, out_dtype="bf16")
            assert torch.equal(b, torch.as_tensor(want, device=torch_dev).to(torch.bfloat16)), (N, L, T, n_sel)


def test_tiled_nb_test_vs_oracle(torch_dev):
    from digdriver_amd import engine
    from oracle import dig_oracle as O
    rng = np.random.default_rng(8)
    C, nb, nt = 3, 40, 200
    mu = rng.gamma(9.0, 3.0, (C, nb))
    sigma = rng.gamma(4.0, 1.0, (C, nb))
    pt = rng.dirichlet(np.ones(nt), size=nb)
    pt[0, :5] = 0.0                                    # N-masked positions: pt = 0 -> p = 1
    k = rng.poisson(mu[:, :, None] * pt[None] * 1.5).astype(np.int32)
    k[1, 3, 7] = 40                                    # a hotspot
    pval, ex = engine.tiled_nb_test(pt, k, mu, sigma)
    for c in range(C):
        wp, we = O.tiled_nb_test(pt, k[c], mu[c], sigma[c])
        rel_close(pval[c], wp, RTOL)
        assert np.array_equal(ex[c], we)
    pt3 = np.stack([pt, pt * 0.5, pt * 0.25])
    pval3, _ = engine.tiled_nb_test(pt3, k, mu, sigma)
    assert np.array_equal(pval3[0], pval[0], equal_nan=True)
    # other shapes: few tiles per bin (generic kernel), one bin per cohort, the reference's default 50-position tiles
    for C, nb, nt in ((2, 7, 5), (2, 1, 17), (1, 300, 50), (5, 33, 1)):
        mu = rng.gamma(9.0, 3.0, (C, nb))
        sigma = rng.gamma(4.0, 1.0, (C, nb))
        pt = rng.dirichlet(np.ones(nt), size=nb)
        k = rng.poisson(mu[:, :, None] * pt[None] * 1.5).astype(np.int32)
        pval, ex = engine.tiled_nb_test(pt, k, mu, sigma)
        for c in range(C):
            wp, we = O.tiled_nb_test(pt, k[c], mu[c], sigma[c])
            rel_close(pval[c], wp, RTOL)
            assert np.array_equal(ex[c], we)


# ---------------------------------------------------------------------------------------
# size-independent properties at BASELINE scale (full 288k-bin x 37-cohort problem)
# ---------------------------------------------------------------------------------------
def test_properties_at_baseline_size(torch_dev):
    import torch
    from bench import make_workload
    from digdriver_amd import engine
    from digdriver_amd.sequence_model import nb_model
    w = make_workload(n_bins=288_000, n_elements=120_091, n_cohorts=37, seed=3)
    td = {k: torch.as_tensor(v, device=torch_dev) for k, v in w.items() if isinstance(v, np.ndarray)}
    acc = engine.accumulate_elements(td["bin_mu"], td["bin_std"], td["bin_y"], td["bin_flag"], td["bin_ctx"], td["ov_ptr"],
                                     td["ov_idx"], td["L"], td["strand_minus"], td["d_pr"])
    E, C = acc["MU"].shape
    # (1) checksum of checksums: sum over elements of MU == sum over CSR entries of bin_mu (linearity)
    want = td["bin_mu"][td["ov_idx"].long()].sum(dim=0)
    assert torch.allclose(acc["MU"].sum(dim=0), want, rtol=1e-10)
    assert torch.equal(acc["R_OBS"].sum(dim=0, dtype=torch.int64), td["bin_y"][td["ov_idx"].long()].sum(dim=0, dtype=torch.int64))
    # (2) strand symmetry: flipping every strand while reverse-complementing both L and d_pr leaves P unchanged
    from oracle import dig_oracle as O
    g = torch.as_tensor(O.minus_strand_gather192(), device=torch_dev)
    flipped = engine.accumulate_elements(td["bin_mu"], td["bin_std"], td["bin_y"], td["bin_flag"], td["bin_ctx"],
                                         td["ov_ptr"], td["ov_idx"], td["L"][:, :, g].contiguous(), 1 - td["strand_minus"],
                                         td["d_pr"][:, g].contiguous())
    assert torch.equal(flipped["MU"], acc["MU"]) and torch.equal(flipped["R_SIZE"], acc["R_SIZE"])
    assert torch.allclose(flipped["P"], acc["P"], rtol=1e-10, atol=0)
    # (3) element statistics: p-values in [0, 1], mid-p identity and monotonicity in k
    st = engine.element_stats(acc["MU"], acc["SIGMA"], acc["P"].view(E, C), acc["P_INDEL"], td["obs_snv"], td["obs_samples"],
                              td["obs_indel"], td["cj"], td["cj_indel"])
    for name in ("PVAL_SNV_BURDEN", "PVAL_SAMPLE_BURDEN", "PVAL_INDEL_BURDEN", "PVAL_MUT_BURDEN"):
        v = st[name]
        assert bool(torch.isfinite(v).all()) and float(v.min()) >= 0.0 and float(v.max()) <= 1.0, name
    # samples <= mutations => sample p-value >= SNV p-value
    assert bool((st["PVAL_SAMPLE_BURDEN"] >= st["PVAL_SNV_BURDEN"] * (1 - 1e-12)).all())
    # Fisher of the two planes recomputed from the outputs
    f = nb_model.fisher_combine(st["PVAL_SNV_BURDEN"], st["PVAL_INDEL_BURDEN"])
    assert torch.allclose(f, st["PVAL_MUT_BURDEN"], rtol=1e-12, atol=0)
    # mid-p telescoping identity: midp(k) - midp(k+1) = (pmf(k) + pmf(k+1)) / 2 > 0, and
    # midp(k) + lower-mid-p(k) = 1, on one million (alpha, p, k) triples taken from the run
    alpha, theta = nb_model.normal_params_to_gamma(acc["MU"], acc["SIGMA"])
    p = 1 / (theta * td["cj"] * acc["P"].view(E, C) + 1)
    sel = torch.randperm(E * C, device=torch_dev)[:1_000_000]
    a_s, p_s = alpha.view(-1)[sel].contiguous(), p.view(-1)[sel].contiguous()
    k_s = td["obs_snv"].view(-1)[sel].double()
    m0 = nb_model.nb_pvalue_greater_midp(k_s, a_s, p_s)
    m1 = nb_model.nb_pvalue_greater_midp(k_s + 1, a_s, p_s)
    assert bool((m0 >= m1).all()) and bool((m0 > m1).float().mean() > 0.9)
    two = nb_model.nb_pvalue_midp(k_s, a_s, p_s)          # lower or upper mid-p by side of the mean
    mean = a_s * (1 - p_s) / p_s
    lower = k_s < mean
    assert torch.allclose(torch.where(lower & (k_s > 0), two + m0, torch.ones_like(m0)), torch.ones_like(m0), rtol=1e-9)
    assert torch.allclose(two[~lower], m0[~lower], rtol=1e-12)
    # (4) the fused operation bench.py runs (dig_element_pipeline) at full size against the oracle on a random subsample:
    # 3 000 whole elements through the accumulation, their 111 000 (element, cohort) pairs through the statistics
    acc2, st2 = engine.element_pipeline(td["bin_mu"], td["bin_std"], td["bin_y"], td["bin_flag"], td["bin_ctx"], td["ov_ptr"],
                                        td["ov_idx"], td["L"], td["strand_minus"], td["d_pr"], td["obs_snv"],
                                        td["obs_samples"], td["obs_indel"], td["cj"], td["cj_indel"])
    rng = np.random.default_rng(11)
    es = np.sort(rng.choice(E, 3000, replace=False))
    lens = (w["ov_ptr"][es + 1] - w["ov_ptr"][es]).astype(np.int64)
    sub_ptr = np.concatenate([[0], np.cumsum(lens)])
    sub_idx = np.concatenate([w["ov_idx"][w["ov_ptr"][e]:w["ov_ptr"][e + 1]] for e in es])
    ref = O.accumulate_elements(w["bin_mu"], w["bin_std"], w["bin_y"], w["bin_flag"], w["bin_ctx"], sub_ptr, sub_idx,
                                w["L"][es], w["strand_minus"][es].astype(bool), w["d_pr"])
    est = torch.as_tensor(es, device=torch_dev)
    np.testing.assert_allclose(acc2["MU"][est].cpu().numpy(), ref["MU"], rtol=1e-12)
    np.testing.assert_allclose(acc2["SIGMA"][est].cpu().numpy(), ref["SIGMA"], rtol=1e-12)
    np.testing.assert_allclose(acc2["P"][est].cpu().numpy(), ref["P"], rtol=1e-11)
    np.testing.assert_allclose(acc2["P_INDEL"][est].cpu().numpy(), ref["P_INDEL"], rtol=1e-15)
    for name in ("R_OBS", "FLAG", "R_SIZE", "ELT_SIZE"):
        assert np.array_equal(acc2[name][est].cpu().numpy(), ref[name]), name
    ref_st = O.element_stats(ref["MU"], ref["SIGMA"], ref["P"][:, 0, :], ref["P_INDEL"][:, None], w["obs_snv"][es],
                             w["obs_samples"][es], w["obs_indel"][es], w["cj"][None, :], w["cj_indel"][None, :])
    for j, name in enumerate(engine.ES_PLANES):
        got, want_ = st2[j][est].cpu().numpy(), ref_st[name]
        assert (np.isnan(got) == np.isnan(want_)).all(), name
        m = np.isfinite(want_) & (np.abs(want_) >= 1e-250)
        rel = np.abs(got[m] - want_[m]) / np.abs(want_[m])
        assert rel.max() <= 1e-6, (name, rel.max())           # tolerance contract of DESIGN 5
        assert (np.abs(got[~m & np.isfinite(want_)]) < 1e-250).all(), name


def test_genic_accumulation_at_gene_set_size(torch_dev):
    """genic_model's four mutation classes (n_class = 4, P_INDEL from the gene length) at the size of the reference's gene
    list (20 091 genes x 37 cohorts on the 288 000-bin grid) against the oracle on a random subsample."""
    import torch
    from bench import make_workload
    from digdriver_amd import engine
    from oracle import dig_oracle as O
    E, C = 20091, 37
    w = make_workload(288_000, E, C, seed=5)
    rng = np.random.default_rng(1)
    L1 = w["L"].reshape(E, -1)[:, :192]
    L4 = np.ascontiguousarray(np.stack([L1] + [rng.poisson(L1 * f).astype(np.int32) for f in (0.7, 0.2, 0.1)], axis=1))
    glen = rng.integers(300, 9000, E).astype(np.int32)
    td = {k: torch.as_tensor(v, device=torch_dev) for k, v in w.items() if isinstance(v, np.ndarray)}
    acc = engine.accumulate_elements(td["bin_mu"], td["bin_std"], td["bin_y"], td["bin_flag"], td["bin_ctx"], td["ov_ptr"],
                                     td["ov_idx"], torch.as_tensor(L4, device=torch_dev), td["strand_minus"], td["d_pr"],
                                     gene_length=torch.as_tensor(glen, device=torch_dev))
    es = np.sort(rng.choice(E, 800, replace=False))
    lens = (w["ov_ptr"][es + 1] - w["ov_ptr"][es]).astype(np.int64)
    sub_ptr = np.concatenate([[0], np.cumsum(lens)])
    sub_idx = np.concatenate([w["ov_idx"][w["ov_ptr"][e]:w["ov_ptr"][e + 1]] for e in es])
    ref = O.accumulate_elements(w["bin_mu"], w["bin_std"], w["bin_y"], w["bin_flag"], w["bin_ctx"], sub_ptr, sub_idx, L4[es],
                                w["strand_minus"][es].astype(bool), w["d_pr"], gene_length=glen[es])
    est = torch.as_tensor(es, device=torch_dev)
    assert acc["P"].shape == (E, 4, C)
    np.testing.assert_allclose(acc["P"][est].cpu().numpy(), ref["P"], rtol=1e-11)
    np.testing.assert_allclose(acc["MU"][est].cpu().numpy(), ref["MU"], rtol=1e-12)
    np.testing.assert_allclose(acc["P_INDEL"][est].cpu().numpy(), ref["P_INDEL"], rtol=1e-15)
    for name in ("ELT_SIZE", "R_SIZE", "R_OBS", "FLAG"):
        assert np.array_equal(acc[name][est].cpu().numpy(), ref[name]), name


def test_context_counting_matches_reference_golden_and_oracle():
    """dig_count_contexts (device-resident and host twin) against the reference's own counts on the golden genome and
    against the oracle on a larger random genome (bit-exact)."""
    import json
    import torch
    from digdriver_amd import engine
    from digdriver_amd.data_tools.genome import PackedGenome
    from oracle import dig_oracle as O
    g = json.load(open(os.path.join(GOLDEN, "contexts_golden.json")))
    genome = PackedGenome.from_sequences(g["genome"])
    chroms, starts, ends = zip(*g["regions"])
    got = engine.count_contexts(genome, chroms, starts, ends, device=0)
    assert np.array_equal(got.cpu().numpy(), np.array(g["counts64"]))
    minus = [s in ("-", "-1") for s in g["strands"]]
    got_m = engine.count_contexts(genome, [c[3:] for c in chroms], starts, ends, minus, on_device=False)
    want192 = np.array(g["counts192"])
    got192, keys = O.expand_contexts_192(got_m)
    assert keys == g["columns192"] and np.array_equal(got192, want192)
    # larger random genome: 10-kb windows and short blocks, N runs across word boundaries
    rng = np.random.default_rng(9)
    seqs = {}
    for name, n in (("1", 250_003), ("2", 99_999)):
        s = rng.choice(np.frombuffer(b"ACGTacgtN", np.uint8), n, p=[.24, .24, .24, .24, .005, .005, .005, .005, .02])
        a = int(rng.integers(0, n - 5000))
        s[a:a + 3000] = ord("N")
        seqs[name] = s.tobytes().decode()
    seqs["3"] = rng.choice(np.frombuffer(b"ACGT", np.uint8), 70_001).tobytes().decode()      # N-free: the unchecked path
    genome = PackedGenome.from_sequences(seqs)
    regs = [("1", 10000 * i, 10000 * (i + 1)) for i in range(26)] + [("2", 10000 * i, 10000 * (i + 1)) for i in range(10)]
    regs += [("3", 10000 * i, 10000 * (i + 1)) for i in range(8)] + [("3", 0, 70_001), ("3", 69_990, 70_500), ("3", 5, 5)]
    for _ in range(300):
        c = "123"[int(rng.integers(0, 3))]
        a = int(rng.integers(0, len(seqs[c])))
        regs.append((c, a, a + int(rng.integers(0, 3000))))
    for _ in range(400):   # every alignment of short regions against the 8-base words and 32-base groups
        a = int(rng.integers(0, 69_000))
        regs.append(("3", a, a + int(rng.integers(0, 140))))
    chroms, starts, ends = zip(*regs)
    minus = rng.uniform(size=len(regs)) < 0.5
    got = engine.count_contexts(genome, chroms, starts, ends, minus, device=0).cpu().numpy()
    want = O.count_contexts_regions(seqs, chroms, starts, ends, minus)
    assert np.array_equal(got, want)
    assert got.sum() > 0
    # the first (4-bit) form and the 2-bit form's host twin: the same counts
    assert np.array_equal(engine.count_contexts(genome, chroms, starts, ends, minus, device=0, form="4bit").cpu().numpy(), want)
    assert np.array_equal(engine.count_contexts(genome, chroms[:50], starts[:50], ends[:50], minus[:50], on_device=False), want[:50])


def test_context_counting_2bit_form_on_letter_runs_and_every_alignment():
    """dig_count_contexts2 (2 bits per base + the list of non-ACGT runs; 4-mers at even bases, counters that are never
    cleared, take-backs at the group ends, single centres, interval corrections) against the oracle: genomes from N-free to
    90 % N, runs that start / end at every offset of a region and of a 64-base group, adjacent runs one base apart, regions
    of 0 ... 3 000 centres at every alignment, chromosome starts and ends, both strands.  A lane takes one region and the
    grid holds a lane per region here: every lane's running totals start from zero.  Their carry from region to region, over
    more than two passes of the grid, is in test_gpu_grid_wrap.py."""
    import torch
    from digdriver_amd import engine
    from digdriver_amd.data_tools.genome import PackedGenome
    from oracle import dig_oracle as O
    rng = np.random.default_rng(41)
    for p_n in (0.0, 0.01, 0.2, 0.9):
        seqs = {"chr1": "".join(rng.choice(list("ACGTN"), 30_011, p=[(1 - p_n) / 4] * 4 + [p_n])),
                "chr2": "".join(rng.choice(list("ACGT"), 5_003)),
                "chr3": "N" * 10 + "".join(rng.choice(list("ACGT"), 300)) + "N" * 700 + "ACGNAC" + "".join(rng.choice(list("ACGT"), 4000))}
        genome = PackedGenome.from_sequences(seqs)
        names = list(seqs)
        regs = []
        for _ in range(6000):
            c = names[int(rng.integers(0, 3))]
            n = len(seqs[c])
            a = int(rng.integers(0, n))
            e = a + int(rng.integers(0, (5, 70, 300, 3000)[int(rng.integers(0, 4))]))
            u = rng.uniform()
            regs.append((c, 0 if u < 0.03 else a, n + 5 if u > 0.95 else e))
        regs += [("chr3", 300 + k, 1020 + k) for k in range(70)] + [("chr3", k, k + 1) for k in range(40)]
        chroms, starts, ends = zip(*regs)
        minus = rng.uniform(size=len(regs)) < 0.5
        got = engine.count_contexts(genome, chroms, starts, ends, minus, device=0).cpu().numpy()
        want = O.count_contexts_regions(seqs, chroms, starts, ends, minus)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert len(bad) == 0, (p_n, len(bad), regs[bad[0]], bool(minus[bad[0]]), (got - want)[bad[0]].tolist())


def test_element_pipeline_equals_separate_calls(torch_dev):
    """dig_element_pipeline (rate sums fused into the statistics kernel) against dig_accumulate_elements followed by
    dig_element_stats on the same inputs: every output of both operations bit-identical."""
    import torch
    from bench import make_workload
    from digdriver_amd import engine
    # cohort counts on both sides of the dot kernel's 16-column tiles and 48-cohort chunks
    for (nb, E, C, seed) in ((3000, 2500, 5, 1), (900, 700, 37, 2), (400, 333, 1, 3), (1200, 1000, 49, 4), (500, 450, 17, 5),
                             (300, 260, 100, 6), (200, 7, 48, 7)):
        w = make_workload(n_bins=nb, n_elements=E, n_cohorts=C, seed=seed)
        td = {k: torch.as_tensor(v, device=torch_dev) for k, v in w.items() if isinstance(v, np.ndarray)}
        # make a few pairs take the compacted pass and a few be degenerate
        td["obs_snv"][::97] += 90
        td["bin_std"][5] = 0.0
        acc = engine.accumulate_elements(td["bin_mu"], td["bin_std"], td["bin_y"], td["bin_flag"], td["bin_ctx"], td["ov_ptr"],
                                         td["ov_idx"], td["L"], td["strand_minus"], td["d_pr"])
        st = engine.element_stats(acc["MU"], acc["SIGMA"], acc["P"].view(E, C), acc["P_INDEL"], td["obs_snv"], td["obs_samples"],
                                  td["obs_indel"], td["cj"], td["cj_indel"])
        acc2, st2 = engine.element_pipeline(td["bin_mu"], td["bin_std"], td["bin_y"], td["bin_flag"], td["bin_ctx"],
                                            td["ov_ptr"], td["ov_idx"], td["L"], td["strand_minus"], td["d_pr"], td["obs_snv"],
                                            td["obs_samples"], td["obs_indel"], td["cj"], td["cj_indel"])
        for k in acc:
            a, b = acc[k], acc2[k]
            assert torch.equal(torch.nan_to_num(a.double(), nan=-7.0), torch.nan_to_num(b.double(), nan=-7.0)), k
        for j, name in enumerate(engine.ES_PLANES):
            a, b = st[name], st2[j]
            assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)), name


def test_compact_pipeline_against_general_form_and_oracle(torch_dev):
    """Context-repeated L (sequence_tools.py:560-564: every element / tile / on-the-fly set): dig_element_pipeline_prepare +
    DIG_PIPE_COMPACT_L run contexts + dot as ONE kernel over the 64 per-context sums of d_pr (acc_dot_ctx_kernel).  Against
    the general 192-substitution form: integer outputs, MU, SIGMA and P_INDEL bit-identical, P within 1e-13 (same
    denominators, regrouped numerator sum), statistics within the contract; against the oracle: P within 1e-11.  Cohort
    counts on both sides of the 16-column tiles / 4-column quads / 48-cohort chunks, elements over 0 ... many bins, both
    strands, E not a multiple of 16, stages as separate calls."""
    import torch
    from bench import make_workload
    from digdriver_amd import _lib, engine
    from oracle import dig_oracle as O
    for (nb, E, C, seed, mb) in ((3000, 2500, 5, 1, 3), (900, 700, 37, 2, 3), (400, 333, 1, 3, 9), (1200, 1000, 49, 4, 3),
                                 (500, 450, 17, 5, 6), (300, 260, 104, 6, 3), (200, 7, 48, 7, 3), (64, 1, 37, 8, 1),
                                 (700, 1601, 40, 9, 12), (50, 16, 8, 10, 2)):
        w = make_workload(n_bins=nb, n_elements=E, n_cohorts=C, seed=seed, max_blocks=mb)
        if E > 20:                                        # a few elements without any bin: rates 0, P = 0 / 0
            ptr = w["ov_ptr"].copy()
            keep = np.ones(len(w["ov_idx"]), bool)
            for e in (3, 11, E - 1):
                keep[ptr[e]:ptr[e + 1]] = False
            cnt = np.diff(ptr)
            cnt[[3, 11, E - 1]] = 0
            w["ov_idx"] = w["ov_idx"][keep]
            w["ov_ptr"] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        td = {k: torch.as_tensor(v, device=torch_dev) for k, v in w.items() if isinstance(v, np.ndarray)}
        args = (td["bin_mu"], td["bin_std"], td["bin_y"], td["bin_flag"], td["bin_ctx"], td["ov_ptr"], td["ov_idx"], td["L"],
                td["strand_minus"], td["d_pr"], td["obs_snv"], td["obs_samples"], td["obs_indel"])
        acc_g, st_g = engine.element_pipeline(*args, td["cj"], td["cj_indel"])
        plan = engine.PipelinePlan(*args)
        assert plan.compact, "make_workload repeats every context count three times"
        acc_c, st_c = plan.run(td["cj"], td["cj_indel"])
        torch.cuda.synchronize()
        for k in ("MU", "SIGMA", "R_OBS", "FLAG", "R_SIZE", "ELT_SIZE", "P_INDEL"):
            assert torch.equal(torch.nan_to_num(acc_g[k].double(), nan=-7.0), torch.nan_to_num(acc_c[k].double(), nan=-7.0)), (k, C)
        pg, pc = acc_g["P"].cpu().numpy(), acc_c["P"].cpu().numpy()
        assert (np.isnan(pg) == np.isnan(pc)).all()
        ok = np.isfinite(pg)
        assert np.array_equal(pc[~ok & ~np.isnan(pg)], pg[~ok & ~np.isnan(pg)])
        assert (np.abs(pc[ok] / pg[ok] - 1) <= 1e-13).all(), C
        sg, sc = st_g.cpu().numpy(), st_c.cpu().numpy()
        def close(got, ref, tol):                          # rel_close, with infinities (an element without bins) in the same places
            fin = ~np.isinf(ref)
            assert np.array_equal(got[~fin], ref[~fin])
            rel_close(got[fin], ref[fin], tol)
        for j, name in enumerate(engine.ES_PLANES):
            # (an ulp of P moves a p-value that the stream pass takes as 1 - CDF just above its 1e-6 acceptance edge by up to
            #  ~1e-8: the cancellation the tolerance contract of 1e-6 against scipy already budgets for)
            close(sc[j], sg[j], 2e-7 if name.startswith("PVAL") else 1e-12)
        want = O.accumulate_elements(w["bin_mu"], w["bin_std"], w["bin_y"], w["bin_flag"], w["bin_ctx"], w["ov_ptr"], w["ov_idx"],
                                     w["L"], w["strand_minus"].astype(bool), w["d_pr"])
        close(pc, want["P"], 1e-11)
        assert np.array_equal(acc_c["R_SIZE"].cpu().numpy(), want["R_SIZE"])
        assert np.array_equal(acc_c["ELT_SIZE"].cpu().numpy(), want["ELT_SIZE"])
        # the stages as separate calls (contexts: nothing to do; dot: the fused kernel; statistics) == one call
        keep_p, keep_s = acc_c["P"].clone(), st_c.clone()
        acc_c["P"].fill_(-3.0)
        st_c.fill_(-3.0)
        plan.run(td["cj"], td["cj_indel"], stages=1)
        plan.run(td["cj"], td["cj_indel"], stages=2)
        plan.run(td["cj"], td["cj_indel"], stages=4 | 8)
        torch.cuda.synchronize()
        assert torch.equal(torch.nan_to_num(acc_c["P"], nan=-7.0), torch.nan_to_num(keep_p, nan=-7.0))
        assert torch.equal(torch.nan_to_num(st_c, nan=-7.0), torch.nan_to_num(keep_s, nan=-7.0))
        # new scale factors on the same accumulation: statistics only (clears the worklist header itself)
        plan.run(td["cj"] * 2.0, td["cj_indel"] * 0.5, stages=4)
        _, st_2 = engine.element_pipeline(*args, td["cj"] * 2.0, td["cj_indel"] * 0.5, compact="auto")
        torch.cuda.synchronize()
        assert torch.equal(torch.nan_to_num(st_c, nan=-7.0), torch.nan_to_num(st_2, nan=-7.0))
    # an L that does NOT repeat (genic class columns, --f-sites sets): prepare says so and the general form runs, same bits as before
    w = make_workload(n_bins=500, n_elements=400, n_cohorts=37, seed=12)
    w["L"][17, 0, 5] += 1
    td = {k: torch.as_tensor(v, device=torch_dev) for k, v in w.items() if isinstance(v, np.ndarray)}
    args = (td["bin_mu"], td["bin_std"], td["bin_y"], td["bin_flag"], td["bin_ctx"], td["ov_ptr"], td["ov_idx"], td["L"],
            td["strand_minus"], td["d_pr"], td["obs_snv"], td["obs_samples"], td["obs_indel"])
    plan = engine.PipelinePlan(*args)
    assert not plan.compact
    acc_p, st_p = plan.run(td["cj"], td["cj_indel"])
    acc_g, st_g = engine.element_pipeline(*args, td["cj"], td["cj_indel"])
    assert torch.equal(acc_p["P"], acc_g["P"]) and torch.equal(torch.nan_to_num(st_p, nan=-7.0), torch.nan_to_num(st_g, nan=-7.0))


def test_packed_bin_records_give_the_same_bits(torch_dev):
    """dig_bin_records_pack (plan time: {Y_PRED, STD^2} pairs + Y_TRUE | FLAG << 31 per (bin, cohort)) feeds the statistics
    stage two gathers per bin instead of four.  Every output of a plan WITH the records equals the plan WITHOUT them bit
    for bit -- general and compact accumulation, elements over 0 ... 12 bins (the first three travel in registers, the rest
    in a loop), C on both sides of 37 -- a table changed in place needs repack_bins(), plans over the same tables share
    one set of records, and a negative count is refused (the record keeps Y_TRUE in 31 bits)."""
    import torch
    from bench import make_workload
    from digdriver_amd import _lib, engine
    for (nb, E, C, seed, mb) in ((900, 700, 37, 2, 3), (400, 333, 1, 3, 9), (700, 1601, 40, 9, 12), (300, 260, 104, 6, 3), (64, 1, 37, 8, 1)):
        w = make_workload(n_bins=nb, n_elements=E, n_cohorts=C, seed=seed, max_blocks=mb)
        w["bin_flag"][::7] = 1
        w["bin_y"][3, 0] = 2 ** 31 - 1                       # the largest count a record holds
        td = {k: torch.as_tensor(v, device=torch_dev) for k, v in w.items() if isinstance(v, np.ndarray)}
        args = (td["bin_mu"], td["bin_std"], td["bin_y"], td["bin_flag"], td["bin_ctx"], td["ov_ptr"], td["ov_idx"], td["L"],
                td["strand_minus"], td["d_pr"], td["obs_snv"], td["obs_samples"], td["obs_indel"])
        for compact in ("auto", False):
            plain = engine.PipelinePlan(*args, compact=compact, pack_bins=False)
            packed = engine.PipelinePlan(*args, compact=compact)
            shared = engine.PipelinePlan(*args, compact=compact, pack_bins=packed)
            assert plain.records is None and packed.records is not None and shared.records is packed.records
            a0, s0 = plain.run(td["cj"], td["cj_indel"])
            for plan in (packed, shared):
                a1, s1 = plan.run(td["cj"], td["cj_indel"])
                torch.cuda.synchronize()
                for k in a0:
                    assert torch.equal(torch.nan_to_num(a0[k].double(), nan=-7.0), torch.nan_to_num(a1[k].double(), nan=-7.0)), (k, C, compact)
                assert torch.equal(torch.nan_to_num(s0, nan=-7.0), torch.nan_to_num(s1, nan=-7.0)), (C, compact)
        # a table changed in place: the plan reads its records until they are rebuilt
        td["bin_mu"][: nb // 2] *= 1.5
        td["bin_flag"][1::3] ^= 1
        stale = packed.run(td["cj"], td["cj_indel"])[0]["MU"].clone()
        packed.repack_bins()
        a1, s1 = packed.run(td["cj"], td["cj_indel"])
        a0, s0 = plain.run(td["cj"], td["cj_indel"])
        torch.cuda.synchronize()
        assert not torch.equal(stale, a0["MU"]) or nb < 4
        for k in a0:
            assert torch.equal(torch.nan_to_num(a0[k].double(), nan=-7.0), torch.nan_to_num(a1[k].double(), nan=-7.0)), k
        assert torch.equal(torch.nan_to_num(s0, nan=-7.0), torch.nan_to_num(s1, nan=-7.0))
    td["bin_y"][5, 0] = -1
    with pytest.raises(_lib.DigHipError, match="negative count"):
        engine.PipelinePlan(*args)


def test_record_major_outputs_give_the_same_bits(torch_dev):
    """DIG_PIPE_RECORDS (ABI 9): the statistics stage writes the ten outputs of a pair -- the seven statistics, MU, SIGMA,
    R_OBS | FLAG -- as tile-blocked records, one aligned 5 120-byte run per 64-pair tile instead of eleven store streams.
    Unpacked (dig_element_records_unpack, both orders) they are the planes of the plane form bit for bit: shapes whose
    pair count is and is not a multiple of 64, C on both sides of 37, elements over 0 ... 12 bins, a workload in which
    most pairs take the queue and the overflow segment behind it."""
    import torch
    from bench import make_workload
    from digdriver_amd import engine
    cases = ((900, 700, 37, 2, 3, 0), (400, 333, 1, 3, 9, 0), (700, 1601, 40, 9, 12, 0), (300, 260, 104, 6, 3, 0), (64, 1, 37, 8, 1, 0),
             (512, 64, 64, 4, 2, 0), (20000, 20000, 37, 31, 3, 300), (9000, 12000, 37, 32, 3, 0))
    for (nb, E, C, seed, mb, bump) in cases:
        w = make_workload(n_bins=nb, n_elements=E, n_cohorts=C, seed=seed, max_blocks=mb)
        w["bin_flag"][::7] = 1
        td = {k: torch.as_tensor(v, device=torch_dev) for k, v in w.items() if isinstance(v, np.ndarray)}
        td["obs_snv"] += bump
        td["obs_samples"] += bump // 2
        args = (td["bin_mu"], td["bin_std"], td["bin_y"], td["bin_flag"], td["bin_ctx"], td["ov_ptr"], td["ov_idx"], td["L"],
                td["strand_minus"], td["d_pr"], td["obs_snv"], td["obs_samples"], td["obs_indel"])
        planes = engine.PipelinePlan(*args)
        recs = engine.PipelinePlan(*args, records_out=True, pack_bins=planes)
        assert recs.out_records.shape == ((E * C + 63) // 64, 5, 64, 2)
        recs.out_records.fill_(float("nan"))
        a0, s0 = planes.run(td["cj"], td["cj_indel"])
        recs.run(td["cj"], td["cj_indel"])
        a1, s1 = recs.unpack()
        sc = recs.unpack(cohort_major=True, stats=torch.empty((7, C, E), dtype=torch.float64, device=torch_dev))
        torch.cuda.synchronize()
        for k in a0:
            assert torch.equal(torch.nan_to_num(a0[k].double(), nan=-7.0), torch.nan_to_num(a1[k].double(), nan=-7.0)), (k, E, C)
        assert torch.equal(torch.nan_to_num(s0, nan=-7.0), torch.nan_to_num(s1, nan=-7.0)), (E, C)
        assert torch.equal(torch.nan_to_num(s0, nan=-7.0).transpose(1, 2), torch.nan_to_num(sc, nan=-7.0)), (E, C)
        if bump:
            assert torch.isfinite(s1[1]).all() and (s1[1] >= 0).all() and (s1[6] >= 0).all()      # no marker left behind
    with pytest.raises(ValueError, match="packed bin records"):
        engine.PipelinePlan(*args, records_out=True, pack_bins=False)


def test_pipeline_when_most_pairs_need_the_second_pass(torch_dev):
    """The fused stream pass finishes its unfinished pairs itself: through the workgroup's LDS queue (1024 records) and, beyond
    that, through the workgroup's own segment of the worklist.  With every SNV count raised past the recurrence's range
    almost every pair takes that route and every workgroup overflows its queue; the result must still be the bits of the
    two separate calls (whose statistics kernel is the two-kernel form)."""
    import torch
    from bench import make_workload
    from digdriver_amd import engine
    for (nb, E, C, seed, bump) in ((20000, 20000, 37, 31, 300), (9000, 12000, 37, 32, 0)):
        w = make_workload(n_bins=nb, n_elements=E, n_cohorts=C, seed=seed)
        td = {k: torch.as_tensor(v, device=torch_dev) for k, v in w.items() if isinstance(v, np.ndarray)}
        td["obs_snv"] += bump
        td["obs_samples"] += bump // 2
        acc = engine.accumulate_elements(td["bin_mu"], td["bin_std"], td["bin_y"], td["bin_flag"], td["bin_ctx"], td["ov_ptr"],
                                         td["ov_idx"], td["L"], td["strand_minus"], td["d_pr"])
        st = engine.element_stats(acc["MU"], acc["SIGMA"], acc["P"].view(E, C), acc["P_INDEL"], td["obs_snv"], td["obs_samples"],
                                  td["obs_indel"], td["cj"], td["cj_indel"])
        acc2, st2 = engine.element_pipeline(td["bin_mu"], td["bin_std"], td["bin_y"], td["bin_flag"], td["bin_ctx"],
                                            td["ov_ptr"], td["ov_idx"], td["L"], td["strand_minus"], td["d_pr"], td["obs_snv"],
                                            td["obs_samples"], td["obs_indel"], td["cj"], td["cj_indel"])
        for j, name in enumerate(engine.ES_PLANES):
            a, b = st[name], st2[j]
            assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)), (name, bump)
        assert torch.isfinite(st2[1]).all() and (st2[1] >= 0).all() and (st2[6] >= 0).all()      # no marker left behind


def test_one_kernel_statistics_equal_round_one_two_kernel_form():
    """The pipelined statistics kernel (stream pass + the workgroup's own second pass) against round 1's two-stage kernel +
    compacted kernel, which DIG_ES_GIVEN_FORM=0 keeps behind dig_element_stats: random shapes and parking rates, bit for
    bit (tools/fuzz_pipeline.py in a process of its own: the switch is read once per process)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DIG_ES_GIVEN_FORM="0")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_pipeline.py"), "80", "7"], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "mismatches 0" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_pipeline_with_more_than_2_to_24_bins(torch_dev):
    """Bin rows beyond 2^24: the statistics stream pass then leaves its 24-bit multiply-add for 64-bit offsets.  Pipeline
    against the two separate calls (bit-identical) and against the oracle on the bins the elements touch."""
    import torch
    from digdriver_amd import engine
    from oracle import dig_oracle as O
    dev = torch_dev
    N, C, E = (1 << 24) + 4096, 2, 1500
    g = torch.Generator(device=dev).manual_seed(3)
    bin_mu = torch.empty((N, C), dtype=torch.float64, device=dev).uniform_(5.0, 60.0, generator=g)
    bin_std = torch.empty((N, C), dtype=torch.float64, device=dev).uniform_(1.0, 8.0, generator=g)
    bin_y = torch.randint(0, 60, (N, C), dtype=torch.int32, device=dev, generator=g)
    bin_flag = (torch.rand((N, C), device=dev, generator=g) < 0.1).to(torch.uint8)
    bin_ctx = torch.randint(0, 400, (N, 64), dtype=torch.int32, device=dev, generator=g)
    rng = np.random.default_rng(8)
    n_ov = rng.integers(1, 4, E)
    first = np.where(rng.uniform(size=E) < 0.5, rng.integers(N - 5000, N - 3, E), rng.integers(0, N - 3, E))
    ov_ptr = np.concatenate([[0], np.cumsum(n_ov)]).astype(np.int64)
    ov_idx = np.concatenate([np.arange(f, f + k) for f, k in zip(first, n_ov)]).astype(np.int32)
    L = rng.integers(0, 40, (E, 1, 192)).astype(np.int32)
    strand = rng.integers(0, 2, E).astype(np.uint8)
    d_pr = rng.dirichlet(np.ones(192), size=C) * 1e-6
    obs = [rng.poisson(3.0, (E, C)).astype(np.int32) for _ in range(3)]
    obs[1] = np.minimum(obs[1], obs[0])
    obs[0][::50] += 80                                              # some pairs for the compacted pass
    cj, cji = np.array([0.7, 1.9]), np.array([0.3, 0.2])
    t = lambda a: torch.as_tensor(a, device=dev)
    args = (bin_mu, bin_std, bin_y, bin_flag, bin_ctx, t(ov_ptr), t(ov_idx), t(L), t(strand), t(d_pr))
    acc = engine.accumulate_elements(*args)
    st = engine.element_stats(acc["MU"], acc["SIGMA"], acc["P"].view(E, C), acc["P_INDEL"], t(obs[0]), t(obs[1]), t(obs[2]), t(cj), t(cji))
    acc2, st2 = engine.element_pipeline(*args, t(obs[0]), t(obs[1]), t(obs[2]), t(cj), t(cji))
    for k in acc:
        assert torch.equal(acc[k], acc2[k]), k
    for j, name in enumerate(engine.ES_PLANES):
        assert torch.equal(torch.nan_to_num(st[name], nan=-7.0), torch.nan_to_num(st2[j], nan=-7.0)), name
    # oracle on the touched bins only (re-indexed compactly)
    used, inv = np.unique(ov_idx, return_inverse=True)
    ui = t(used.astype(np.int64))
    ref = O.accumulate_elements(bin_mu[ui].cpu().numpy(), bin_std[ui].cpu().numpy(), bin_y[ui].cpu().numpy(),
                                bin_flag[ui].cpu().numpy(), bin_ctx[ui].cpu().numpy(), ov_ptr, inv.astype(np.int32), L,
                                strand.astype(bool), d_pr)
    np.testing.assert_allclose(acc2["MU"].cpu().numpy(), ref["MU"], rtol=1e-12)
    np.testing.assert_allclose(acc2["P"].cpu().numpy(), ref["P"], rtol=1e-11)
    assert np.array_equal(acc2["R_OBS"].cpu().numpy(), ref["R_OBS"]) and np.array_equal(acc2["R_SIZE"].cpu().numpy(), ref["R_SIZE"])


def test_degenerate_shapes_do_not_crash(torch_dev):
    """Empty and ragged inputs through every entry point: zero elements / cohorts / regions / rows, an element without
    bins (MU = 0, SIGMA = 0 -> NaN statistics, as numpy gives), one-pair problems."""
    import torch
    from bench import make_workload
    from digdriver_amd import engine
    from digdriver_amd.data_tools.genome import PackedGenome
    from digdriver_amd.sequence_model import nb_model
    dev = torch_dev
    z64 = torch.zeros(0, dtype=torch.float64, device=dev)
    assert nb_model.nb_pvalue_greater_midp(z64, z64, z64).numel() == 0
    st = engine.element_stats(torch.zeros((0, 3), dtype=torch.float64, device=dev), torch.zeros((0, 3), dtype=torch.float64, device=dev),
                              torch.zeros((0, 3), dtype=torch.float64, device=dev), z64, torch.zeros((0, 3), dtype=torch.int32, device=dev),
                              torch.zeros((0, 3), dtype=torch.int32, device=dev), torch.zeros((0, 3), dtype=torch.int32, device=dev),
                              torch.ones(3, dtype=torch.float64, device=dev), torch.ones(3, dtype=torch.float64, device=dev))
    assert st["PVAL_SNV_BURDEN"].shape == (0, 3)
    # ragged CSR: element 1 has no bins at all, element 2 has five
    w = make_workload(n_bins=300, n_elements=4, n_cohorts=2, seed=8)
    td = {k: torch.as_tensor(v, device=dev) for k, v in w.items() if isinstance(v, np.ndarray)}
    ov_ptr = torch.tensor([0, 1, 1, 6, 7], dtype=torch.int64, device=dev)
    ov_idx = torch.tensor([3, 10, 11, 12, 13, 14, 299], dtype=torch.int32, device=dev)
    acc = engine.accumulate_elements(td["bin_mu"], td["bin_std"], td["bin_y"], td["bin_flag"], td["bin_ctx"], ov_ptr, ov_idx,
                                     td["L"], td["strand_minus"], td["d_pr"])
    assert float(acc["MU"][1].abs().sum()) == 0.0 and int(acc["R_SIZE"][1]) == 0 and int(acc["R_OBS"][1].sum()) == 0
    want = td["bin_mu"][10:15].sum(dim=0)
    assert torch.allclose(acc["MU"][2], want, rtol=1e-14)
    acc2, st2 = engine.element_pipeline(td["bin_mu"], td["bin_std"], td["bin_y"], td["bin_flag"], td["bin_ctx"], ov_ptr, ov_idx,
                                        td["L"], td["strand_minus"], td["d_pr"], td["obs_snv"], td["obs_samples"], td["obs_indel"],
                                        td["cj"], td["cj_indel"])
    assert torch.equal(acc2["MU"], acc["MU"]) and torch.equal(acc2["FLAG"], acc["FLAG"])
    assert bool(torch.isnan(st2[1][1]).all())                      # mu = sigma = 0 -> alpha = 0/0 -> NaN p-values (numpy semantics)
    assert bool(torch.isfinite(st2[1][[0, 2, 3]]).all())
    # zero regions / rows / mutations
    g = PackedGenome.from_sequences({"1": "ACGTACGTNNACGT"})
    assert engine.count_contexts(g, [], [], [], device=0).shape == (0, 64)
    one = engine.count_contexts(g, ["1"], [0], [14], device=0).cpu().numpy()
    assert one.sum() == 8                                           # centres 1..12 minus the five windows touching N
    x = torch.zeros((5, 100, 4), dtype=torch.float32, device=dev)
    assert engine.gather_bins(x, torch.zeros(0, dtype=torch.int64, device=dev), torch.arange(4, device=dev)).shape == (0, 100, 4)


def test_configs0_chr21_every_element_against_the_oracle(torch_dev):
    """BASELINE configs[0] (SURVEY 8d cfg 1): chr21 only -- N = 4 812 10-kb bins, ONE cohort, E = 2 000 elements, seed 21 --
    through dig_element_pipeline (both forms of the accumulation) with EVERY element and every output checked against the
    oracle: integers bit-exact, rates and P to 1e-12 / 1e-11, the seven statistics planes within the 1e-6 contract."""
    import torch
    from bench import make_workload
    from digdriver_amd import engine
    from oracle import dig_oracle as O
    w = make_workload(n_bins=4812, n_elements=2000, n_cohorts=1, seed=21)
    td = {k: torch.as_tensor(v, device=torch_dev) for k, v in w.items() if isinstance(v, np.ndarray)}
    args = (td["bin_mu"], td["bin_std"], td["bin_y"], td["bin_flag"], td["bin_ctx"], td["ov_ptr"], td["ov_idx"], td["L"],
            td["strand_minus"], td["d_pr"], td["obs_snv"], td["obs_samples"], td["obs_indel"], td["cj"], td["cj_indel"])
    want = O.accumulate_elements(w["bin_mu"], w["bin_std"], w["bin_y"], w["bin_flag"], w["bin_ctx"], w["ov_ptr"], w["ov_idx"], w["L"],
                                 w["strand_minus"].astype(bool), w["d_pr"])
    want_st = O.element_stats(want["MU"], want["SIGMA"], want["P"][:, 0, :], want["P_INDEL"][:, None], w["obs_snv"], w["obs_samples"],
                              w["obs_indel"], w["cj"][None, :], w["cj_indel"][None, :])
    for compact in (False, "auto"):
        acc, st = engine.element_pipeline(*args, compact=compact)
        torch.cuda.synchronize()
        for k in ("R_OBS", "FLAG", "R_SIZE", "ELT_SIZE"):
            assert np.array_equal(acc[k].cpu().numpy(), want[k]), (k, compact)
        for k, tol in (("MU", 1e-12), ("SIGMA", 1e-12), ("P_INDEL", 1e-12), ("P", 1e-11)):
            rel_close(acc[k].cpu().numpy(), want[k], tol)
        for j, name in enumerate(engine.ES_PLANES):
            rel_close(st[j].cpu().numpy(), want_st[name], RTOL)
    assert (w["obs_snv"] > 0).any() and np.isfinite(want_st["PVAL_MUT_BURDEN"]).all()


def test_host_twins_of_pipeline_tiles_and_join(torch_dev):
    """The `_host` twins added in ABI 4 (dig_element_pipeline_host, dig_base_tile_probs_host, dig_tile_mut_counts_host,
    dig_overlap_join_count_host / _fill_host): host pointers in, host arrays out, the same bits as the device entry points."""
    import torch
    from bench import make_workload
    from digdriver_amd import _lib, engine
    from digdriver_amd.data_tools import tabulate_gpu
    from digdriver_amd.data_tools.genome import PackedGenome
    hp = _lib.host_ptr
    # ---- pipeline ----
    w = make_workload(n_bins=700, n_elements=533, n_cohorts=5, seed=77)
    E, C, N = 533, 5, 700
    td = {k: torch.as_tensor(v, device=torch_dev) for k, v in w.items() if isinstance(v, np.ndarray)}
    acc_d, st_d = engine.element_pipeline(td["bin_mu"], td["bin_std"], td["bin_y"], td["bin_flag"], td["bin_ctx"], td["ov_ptr"], td["ov_idx"],
                                          td["L"], td["strand_minus"], td["d_pr"], td["obs_snv"], td["obs_samples"], td["obs_indel"],
                                          td["cj"], td["cj_indel"], compact="auto")
    o = dict(MU=np.empty((E, C)), SIGMA=np.empty((E, C)), R_OBS=np.empty((E, C), np.int32), FLAG=np.empty((E, C), np.int32),
             P=np.empty((E, 1, C)), R_SIZE=np.empty(E, np.int32), ELT_SIZE=np.empty(E, np.int32), P_INDEL=np.empty(E))
    st_h = np.empty((7, E, C))
    c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)
    ins = [c(w["bin_mu"], np.float64), c(w["bin_std"], np.float64), c(w["bin_y"], np.int32), c(w["bin_flag"], np.uint8),
           c(w["bin_ctx"], np.int32), c(w["ov_ptr"], np.int64), c(w["ov_idx"], np.int32), c(w["L"], np.int32),
           c(w["strand_minus"], np.uint8), None, c(w["d_pr"], np.float64), c(w["obs_snv"], np.int32), c(w["obs_samples"], np.int32),
           c(w["obs_indel"], np.int32), c(w["cj"], np.float64), c(w["cj_indel"], np.float64)]
    _lib.call("dig_element_pipeline_host", *[hp(a) for a in ins], hp(o["MU"]), hp(o["SIGMA"]), hp(o["R_OBS"]), hp(o["FLAG"]), hp(o["P"]),
              hp(o["R_SIZE"]), hp(o["ELT_SIZE"]), hp(o["P_INDEL"]), hp(st_h), N, E, C, 0)
    for k in o:
        assert np.array_equal(o[k], acc_d[k].cpu().numpy(), equal_nan=True), k
    assert np.array_equal(st_h, st_d.cpu().numpy(), equal_nan=True)
    # ---- tiles ----
    rng = np.random.default_rng(3)
    seqs = {"chr1": "".join(rng.choice(list("ACGTN"), 7013, p=[.24, .25, .25, .24, .02])), "chr2": "".join(rng.choice(list("ACGT"), 2500))}
    genome = PackedGenome.from_sequences(seqs)
    chroms = ["chr1"] * 7 + ["chr2"] * 3
    starts = np.array([0, 1000, 2000, 3000, 4000, 5000, 6000, 0, 1000, 2000], np.int64)
    ends = starts + 1000
    S = rng.uniform(1e-3, 1e-2, (3, 64))
    pt_d, first_d, nval_d = engine.base_tile_probs(genome, chroms, starts, ends, S, 50, device=0)
    R, T = len(chroms), pt_d.shape[2]
    pt_h, first_h, nval_h = np.empty((3, R, T)), np.empty(R, np.int64), np.empty(R, np.int32)
    ci = genome.chrom_index(chroms)
    _lib.call("dig_base_tile_probs_host", hp(genome.words), genome.words.size, hp(genome.offsets), hp(genome.lengths), len(genome.names),
              hp(ci), hp(starts), hp(ends), R, hp(np.ascontiguousarray(S)), 3, 50, T, hp(pt_h), hp(first_h), hp(nval_h), 0)
    assert np.array_equal(pt_h, pt_d.cpu().numpy(), equal_nan=True) and np.array_equal(first_h, first_d.cpu().numpy())
    assert np.array_equal(nval_h, nval_d.cpu().numpy())
    # ---- join + tile counts ----
    M = 4000
    mci = rng.integers(0, 2, M)
    ms = np.array([rng.integers(0, len(seqs["chr%d" % (i + 1)])) for i in mci], np.int64)
    me = ms + 1
    co = rng.integers(-1, 4, M).astype(np.int32)                       # ids -1 and 3 are outside [0, C): skipped, not counted
    blocks = tabulate_gpu.ElementBlocks(ci, starts, ends, np.arange(R), R, torch_dev)
    mc_t = torch.as_tensor(mci, device=torch_dev).to(torch.int64)
    pm_d, pb_d = tabulate_gpu.overlap_pairs(blocks, mc_t, torch.as_tensor(ms, device=torch_dev), torch.as_tensor(me, device=torch_dev))
    keys = [blocks.start_key.cpu().numpy(), blocks.runmax_key.cpu().numpy(), blocks.end.cpu().numpy()]
    counts = np.empty(M, np.int32)
    mch = mci.astype(np.int64)
    _lib.call("dig_overlap_join_count_host", hp(keys[0]), hp(keys[1]), hp(keys[2]), R, hp(mch), hp(ms), hp(me), M, hp(counts), 0)
    offs = (np.cumsum(counts) - counts).astype(np.int64)
    n_pairs = int(counts.sum())
    pm_h, pb_h = np.empty(n_pairs, np.int32), np.empty(n_pairs, np.int32)
    _lib.call("dig_overlap_join_fill_host", hp(keys[0]), hp(keys[1]), hp(keys[2]), R, hp(mch), hp(ms), hp(me), M, hp(offs), n_pairs,
              hp(pm_h), hp(pb_h), 0)
    assert n_pairs == pm_d.numel() and np.array_equal(pm_h, pm_d.cpu().numpy()) and np.array_equal(pb_h, pb_d.cpu().numpy())
    k_d = engine.tile_mut_counts(genome, chroms, starts, ends, first_d, nval_d, ["chr%d" % (i + 1) for i in mci], ms, me, co, 3, 50, T)
    pr_h = blocks.elt.cpu().numpy()[pb_h].astype(np.int32)
    k_h = np.empty((3, R, T), np.int32)
    _lib.call("dig_tile_mut_counts_host", hp(pm_h), hp(pr_h), n_pairs, hp(ms), M, hp(co), hp(first_h), hp(nval_h), 50, T, R, 3, hp(k_h), 0)
    assert np.array_equal(k_h, k_d.cpu().numpy())
    inside = (co >= 0) & (co < 3)
    assert 0 < int(k_h.sum()) <= int(inside.sum())
    # ---- general-context tile probabilities (penta-nucleotide tables) ----
    S5 = rng.uniform(1e-4, 1e-2, (3, 1024))
    pt5_d, f5_d, n5_d = engine.base_tile_probs(genome, chroms, starts, ends, S5, 50, device=0)
    pt5_h, f5_h, n5_h = np.empty((3, R, T)), np.empty(R, np.int64), np.empty(R, np.int32)
    _lib.call("dig_base_tile_probs_ctx_host", hp(genome.words), genome.words.size, hp(genome.offsets), hp(genome.lengths),
              len(genome.names), hp(ci), hp(starts), hp(ends), R, hp(np.ascontiguousarray(S5)), 3, 2, 50, T, hp(pt5_h), hp(f5_h), hp(n5_h), 0)
    assert np.array_equal(pt5_h, pt5_d.cpu().numpy(), equal_nan=True) and np.array_equal(f5_h, f5_d.cpu().numpy())
    assert np.array_equal(n5_h, n5_d.cpu().numpy()) and f5_h[0] == 2
    # ---- gene pipeline ----
    G = 61
    wg = make_workload(n_bins=300, n_elements=G, n_cohorts=4, seed=78)
    Lg = np.repeat(rng.poisson(5.0, (G, 4, 64)), 3, axis=2).astype(np.int32)
    glen = rng.integers(300, 9000, G).astype(np.int32)
    obs5 = rng.poisson(3.0, (G, 5, 4)).astype(np.int32)
    ns6 = rng.poisson(2.0, (G, 6, 4)).astype(np.int32)
    ti = rng.uniform(0.05, 0.3, 4)
    tg = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=torch_dev)
    acc_g, st_g = engine.gene_pipeline(tg(wg["bin_mu"]), tg(wg["bin_std"]), tg(wg["bin_y"]), tg(wg["bin_flag"]), tg(wg["bin_ctx"]),
                                       tg(wg["ov_ptr"]), tg(wg["ov_idx"]), tg(Lg), tg(wg["strand_minus"]), tg(glen), tg(wg["d_pr"]), tg(obs5),
                                       tg(ns6), tg(wg["cj"]), tg(ti))
    og = dict(MU=np.empty((G, 4)), SIGMA=np.empty((G, 4)), R_OBS=np.empty((G, 4), np.int32), FLAG=np.empty((G, 4), np.int32),
              P=np.empty((G, 4, 4)), R_SIZE=np.empty(G, np.int32), ELT_SIZE=np.empty(G, np.int32), P_INDEL=np.empty(G))
    out_h = np.empty((22, G, 4))
    ins = [c(wg["bin_mu"], np.float64), c(wg["bin_std"], np.float64), c(wg["bin_y"], np.int32), c(wg["bin_flag"], np.uint8),
           c(wg["bin_ctx"], np.int32), c(wg["ov_ptr"], np.int64), c(wg["ov_idx"], np.int32), Lg, c(wg["strand_minus"], np.uint8), glen,
           c(wg["d_pr"], np.float64), obs5, ns6, c(wg["cj"], np.float64), c(ti, np.float64)]
    _lib.call("dig_gene_pipeline_host", *[hp(a) for a in ins], 1, hp(og["MU"]), hp(og["SIGMA"]), hp(og["R_OBS"]), hp(og["FLAG"]),
              hp(og["P"]), hp(og["R_SIZE"]), hp(og["ELT_SIZE"]), hp(og["P_INDEL"]), hp(out_h), 300, G, 4, 0)
    for k in og:
        assert np.array_equal(og[k], acc_g[k].cpu().numpy(), equal_nan=True), k
    for j, name in enumerate(engine.GS_PLANES):
        assert np.array_equal(out_h[j], st_g[name].cpu().numpy(), equal_nan=True), name


def _twin_agrees_with_device(dev, name, args, ws_bytes=None):
    """`name`_host on the numpy arrays of `args` and `name` on device copies of them (None stays NULL, scalars pass as they
    are, a workspace of ws_bytes goes in front of the stream): every array comes back with the same bits.  Returns the
    host twin's arrays."""
    import torch
    from digdriver_amd import _lib
    is_arr = lambda a: isinstance(a, np.ndarray)
    host = [a.copy() if is_arr(a) else a for a in args]
    _lib.call(name + "_host", *[_lib.host_ptr(a) if is_arr(a) else a for a in host], 0)
    devs = [torch.as_tensor(a, device=dev) if is_arr(a) else a for a in args]
    ws = [] if ws_bytes is None else [torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev), ws_bytes]
    _lib.call(name, *[_lib.dev_ptr(t) if isinstance(t, torch.Tensor) else t for t in devs + ws], _lib.stream_ptr())
    torch.cuda.synchronize()
    for j, (h, d) in enumerate(zip(host, devs)):
        if is_arr(h):
            assert np.array_equal(h, d.cpu().numpy(), equal_nan=True), (name, j)
    return host


def test_staged_host_twins_match_their_device_entry_points(torch_dev):
    """The `_host` twins not covered above against their device entry points on small inputs, bit for bit, through their
    optional inputs: the NB tails, Fisher, gamma; accumulation with one and four classes, with and without gene_length;
    element statistics with and without indel parameters, pi_indel per element and per cohort; gene statistics with and
    without the indel block; tiled tests with a shared and a per-cohort pt; scale sums with N > 0 and N == 0; gathers with
    and without a track list; both context-count forms on genomes with and without runs of N."""
    from bench import make_workload
    from digdriver_amd import _lib, engine
    from digdriver_amd.data_tools.genome import PackedGenome
    agree = lambda name, *args, ws=None: _twin_agrees_with_device(torch_dev, name, list(args), ws)
    rng = np.random.default_rng(12)
    nan = lambda *shape: np.full(shape, np.nan)
    neg = lambda *shape: np.full(shape, -7, np.int32)
    # ---- elementwise ----
    n = 3001
    k, alpha, p = rng.poisson(4.0, n).astype(np.float64), rng.gamma(2.0, 3.0, n), rng.uniform(0.05, 0.95, n)
    for tail in ("dig_nb_midp_upper", "dig_nb_exact", "dig_nb_greater", "dig_nb_midp_twosided"):
        agree(tail, k, alpha, p, nan(n), n)
    agree("dig_fisher", rng.uniform(1e-9, 1.0, n), rng.uniform(1e-9, 1.0, n), nan(n), n)
    agree("dig_normal_params_to_gamma", rng.gamma(3.0, 2.0, n), rng.uniform(0.1, 5.0, n), nan(n), nan(n), n)
    # ---- accumulation ----
    E, C, N = 300, 3, 400
    w = make_workload(n_bins=N, n_elements=E, n_cohorts=C, seed=13)
    c = lambda key, dt: np.ascontiguousarray(w[key], dtype=dt)
    bins = [c("bin_mu", np.float64), c("bin_std", np.float64), c("bin_y", np.int32), c("bin_flag", np.uint8), c("bin_ctx", np.int32),
            c("ov_ptr", np.int64), c("ov_idx", np.int32)]
    L4 = np.repeat(rng.poisson(5.0, (E, 4, 64)), 3, axis=2).astype(np.int32)
    glen = rng.integers(300, 9000, E).astype(np.int32)
    acc = {}
    for n_class, L in ((1, c("L", np.int32)), (4, L4)):
        for gl in (None, glen):
            res = agree("dig_accumulate_elements", *bins, L, n_class, c("strand_minus", np.uint8), gl, c("d_pr", np.float64),
                        nan(E, C), nan(E, C), neg(E, C), neg(E, C), nan(E, n_class, C), neg(E), neg(E), nan(E), N, E, C,
                        ws=_lib.workspace_bytes("accumulate", E, C))
            acc[n_class, gl is not None] = res[12:20]
    # ---- element statistics ----
    MU, SIGMA, _, _, P, _, _, P_INDEL = acc[1, False]
    obs = [c("obs_snv", np.int32), c("obs_samples", np.int32), c("obs_indel", np.int32), c("cj", np.float64), c("cj_indel", np.float64)]
    pi_cohort = np.ascontiguousarray(P_INDEL[:, None] * rng.uniform(0.5, 2.0, (E, C)))
    for mu_i, sg_i in ((None, None), (MU * 0.3, SIGMA * 0.5)):
        for per_cohort, pi_i in ((0, P_INDEL), (1, pi_cohort)):
            agree("dig_element_stats", MU, SIGMA, mu_i, sg_i, np.ascontiguousarray(P[:, 0, :]), pi_i, per_cohort, *obs, nan(7, E, C), E, C,
                  ws=_lib.workspace_bytes("element_stats", E, C))
    # ---- gene statistics ----
    MUg, SIGMAg, _, _, Pg, _, _, PIg = acc[4, True]
    obs5, ns6 = rng.poisson(3.0, (E, 5, C)).astype(np.int32), rng.poisson(2.0, (E, 6, C)).astype(np.int32)
    ti = rng.uniform(0.05, 0.3, C)
    agree("dig_gene_stats", MUg, SIGMAg, None, None, Pg, 4, PIg, 0, obs5, ns6, obs[3], ti, 1, nan(22, E, C), E, C)
    agree("dig_gene_stats", MUg, SIGMAg, MUg * 0.3, SIGMAg * 0.5, Pg, 4, PIg, 0, obs5, ns6, obs[3], ti, 1, nan(22, E, C), E, C)
    agree("dig_gene_stats", MUg, SIGMAg, None, None, Pg, 4, None, 0, obs5, ns6, obs[3], None, 0, nan(22, E, C), E, C)
    # ---- tiled tests ----
    nb, nt = 40, 20
    kt = rng.poisson(1.0, (C, nb, nt)).astype(np.int32)
    mut = rng.uniform(5.0, 40.0, (C, nb))
    sgt = mut * rng.uniform(0.2, 0.8, (C, nb))
    for per_cohort, pt in ((0, rng.dirichlet(np.ones(nt), nb)), (1, rng.dirichlet(np.ones(nt), (C, nb)))):
        agree("dig_tiled_nb_test", pt, per_cohort, kt, mut, sgt, nan(C, nb, nt), nan(C, nb, nt), C, nb, nt)
    # ---- scale sums ----
    agree("dig_scale_suffstats", bins[0], bins[3], N, C, nan(C), ws=_lib.workspace_bytes("suffstats", N, C))
    agree("dig_scale_suffstats", None, None, 0, C, nan(C), ws=_lib.workspace_bytes("suffstats", 0, C))
    # ---- gathers ----
    Nx, Lx, Tx, B = 50, 7, 6, 33
    rows = rng.integers(0, Nx, B).astype(np.int64)
    agree("dig_gather_bins", rng.normal(size=(Nx, Lx, Tx)), 1, Nx, Lx, Tx, rows, B, np.array([5, 0, 3], np.int32), 3,
          np.full((B, Lx, 3), np.nan, np.float32), 0, 0)                                  # f64 -> f32, three tracks
    agree("dig_gather_bins", rng.integers(-3000, 3000, (Nx, Lx, Tx)).astype(np.int16), 2, Nx, Lx, Tx, rows, B, None, Tx,
          np.zeros((B, Tx, Lx), np.int16), 3, 1)                                          # i16 -> bf16, every track, transposed
    # ---- context counts: n_int == 0 and n_int > 0 ----
    for p_n, n1, n2 in ((0.0, 6000, 2000), (0.05, 6007, 2003)):      # whole words of ACGT: no run of other letters, no padding
        seqs = {"c1": "".join(rng.choice(list("ACGTN"), n1, p=[(1 - p_n) / 4] * 4 + [p_n])), "c2": "".join(rng.choice(list("ACGT"), n2))}
        genome = PackedGenome.from_sequences(seqs)
        assert (genome.two_bit()[1].size > 0) == (p_n > 0)
        chroms = ["c1"] * 40 + ["c2"] * 10
        starts = np.array([int(rng.integers(0, len(seqs[ch]))) for ch in chroms], np.int64)
        ends = np.minimum(starts + rng.integers(0, 700, len(chroms)), [len(seqs[ch]) for ch in chroms])
        minus = rng.uniform(size=len(chroms)) < 0.5
        for form in ("2bit", "4bit"):
            dv = engine.count_contexts(genome, chroms, starts, ends, minus, device=0, form=form).cpu().numpy()
            assert np.array_equal(engine.count_contexts(genome, chroms, starts, ends, minus, on_device=False, form=form), dv), form
            assert dv.sum() > 0


def test_gene_pipeline_all_cohorts_against_oracle(torch_dev):
    """dig_gene_pipeline: genic_model's accumulation (four class columns of L, P_INDEL = GENE_LENGTH / R_SIZE) + the gene
    statistics block (six classes x count / sample tests, indel test, Fisher on TRUNC + INDEL) for G genes x C cohorts in one
    call, against the oracle's gene_stats on the oracle's accumulation; integer planes exact, p-values within the contract;
    and dig_gene_stats through its host twin gives the same bits."""
    import torch
    from bench import make_workload
    from digdriver_amd import engine
    from oracle import dig_oracle as O
    G, C, N = 417, 5, 900
    w = make_workload(n_bins=N, n_elements=G, n_cohorts=C, seed=41, max_blocks=8)
    rng = np.random.default_rng(42)
    L64 = rng.poisson(6.0, (G, 4, 64))
    L = np.repeat(L64, 3, axis=2).astype(np.int32)
    L[:, :, ::7] += rng.integers(0, 3, (G, 4, 28))                   # class columns do not repeat per context (no compact form)
    gene_length = rng.integers(300, 9000, G).astype(np.int32)
    acc_w = O.accumulate_elements(w["bin_mu"], w["bin_std"], w["bin_y"], w["bin_flag"], w["bin_ctx"], w["ov_ptr"], w["ov_idx"], L,
                                  w["strand_minus"].astype(bool), w["d_pr"], gene_length=gene_length)
    alpha = acc_w["MU"] ** 2 / acc_w["SIGMA"] ** 2
    theta = acc_w["SIGMA"] ** 2 / acc_w["MU"] * w["cj"][None, :]
    P4 = acc_w["P"]                                                 # [G, 4, C]
    pi = {"SYN": P4[:, 0], "MIS": P4[:, 1], "NONS": P4[:, 2], "SPL": P4[:, 3]}
    pi["TRUNC"] = pi["NONS"] + pi["SPL"]
    pi["NONSYN"] = pi["MIS"] + pi["TRUNC"]
    obs5 = np.stack([rng.poisson(alpha * theta * pi[c] * 1.2) for c in ("SYN", "MIS", "NONS", "SPL")] +
                    [rng.poisson(alpha * theta * acc_w["P_INDEL"][:, None] * 0.1)], axis=1).astype(np.int32)
    obs5[::50, 1] += 400                                             # a few counts beyond the recurrence's table
    obs = {"SYN": obs5[:, 0], "MIS": obs5[:, 1], "NONS": obs5[:, 2], "SPL": obs5[:, 3]}
    obs["TRUNC"] = obs["NONS"] + obs["SPL"]
    obs["NONSYN"] = obs["MIS"] + obs["TRUNC"]
    ns = {c: rng.binomial(obs[c], 0.9) for c in O.GENE_CLASSES}
    n_samp = np.stack([ns[c] for c in O.GENE_CLASSES], axis=1).astype(np.int32)
    t_indel = rng.uniform(0.05, 0.3, C)
    want = O.gene_stats(acc_w["MU"], acc_w["SIGMA"], pi, obs, ns, w["cj"][None, :], pi_indel=acc_w["P_INDEL"][:, None],
                        obs_indel=obs5[:, 4], t_indel=t_indel[None, :])
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=torch_dev)
    acc, st = engine.gene_pipeline(t(w["bin_mu"]), t(w["bin_std"]), t(w["bin_y"]), t(w["bin_flag"]), t(w["bin_ctx"]), t(w["ov_ptr"]),
                                   t(w["ov_idx"]), t(L), t(w["strand_minus"]), t(gene_length), t(w["d_pr"]), t(obs5), t(n_samp),
                                   t(w["cj"]), t(t_indel))
    torch.cuda.synchronize()
    rel_close(acc["P"].cpu().numpy(), acc_w["P"], 1e-11)
    rel_close(acc["P_INDEL"].cpu().numpy(), acc_w["P_INDEL"], 1e-12)
    assert np.array_equal(acc["R_SIZE"].cpu().numpy(), acc_w["R_SIZE"])
    for name in engine.GS_PLANES:
        rel_close(st[name].cpu().numpy(), want[name], 1e-12 if name.startswith(("EXP", "THETA")) else RTOL)
    assert (want["PVAL_MIS_BURDEN"][::50] < 1e-20).any()
    # the statistics alone, through the host twin, on the device's own accumulation: the same bits
    host = engine.gene_stats(acc["MU"].cpu().numpy(), acc["SIGMA"].cpu().numpy(), acc["P"].cpu().numpy(), acc["P_INDEL"].cpu().numpy(),
                             obs5, n_samp, w["cj"], t_indel)
    for name in engine.GS_PLANES:
        assert np.array_equal(host[name], st[name].cpu().numpy(), equal_nan=True), name
    # without the indel block those four planes are NaN and nothing else moves
    no_ind = engine.gene_stats(acc["MU"], acc["SIGMA"], acc["P"], acc["P_INDEL"], t(obs5), t(n_samp), t(w["cj"]))
    assert torch.isnan(no_ind["PVAL_MUT_BURDEN"]).all() and torch.equal(no_ind["PVAL_TRUNC_BURDEN"], st["PVAL_TRUNC_BURDEN"])
