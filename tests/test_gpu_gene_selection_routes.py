"""dig_gene_selection where its formulas are delicate, and Fisher's method around its switch of form, against the 80-digit
references of tests/golden/gene_selection_routes_golden.npz (tests/golden/make_gene_selection_routes_golden.py;
tests/test_gene_selection_routes_fixture.py holds the checker, the bounds M and M_F and how they were set, and shows that
subtly wrong formulas are rejected).  One launch per form: device tensors, the _host twin, n_pi = 4.  Every check prints one line
per plane and group; DESIGN.md 5.2 records the figures of the MI355X run."""
import numpy as np
import pytest

from test_gene_selection_routes_fixture import check_fisher, check_planes, load_fixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    from digdriver_amd import _lib
    _lib.require_device()
    return load_fixture()


@pytest.fixture(scope="module")
def device_planes(fx):
    import torch
    from digdriver_amd import engine
    dev = torch.device("cuda:0")
    res = engine.gene_selection(*[torch.as_tensor(fx[k], device=dev) for k in ("alpha", "theta", "pi", "obs")])
    assert all(v.is_cuda for v in res.values())
    return np.stack([res[name].cpu().numpy() for name in engine.SEL_PLANES])


def test_device_planes_against_the_80_digit_reference(fx, device_planes):
    check_planes(device_planes, fx, "device")


def test_host_twin_gives_the_bits_of_the_device_entry(fx, device_planes):
    from digdriver_amd import engine
    res = engine.gene_selection(fx["alpha"], fx["theta"], fx["pi"], fx["obs"])
    for i, name in enumerate(engine.SEL_PLANES):
        assert isinstance(res[name], np.ndarray) and np.array_equal(res[name], device_planes[i], equal_nan=True), name


def test_four_class_probabilities_against_the_80_digit_reference(fx, device_planes):
    """n_pi = 4: TRUNC and NONSYN are formed in the kernel; every pair of the fixture has pi[4], pi[5] as those sums."""
    import torch
    from digdriver_amd import engine
    assert bool(fx["pi_sums"][0])
    dev = torch.device("cuda:0")
    res = engine.gene_selection(torch.as_tensor(fx["alpha"], device=dev), torch.as_tensor(fx["theta"], device=dev),
                                torch.as_tensor(fx["pi"][:, :4, :].copy(), device=dev), torch.as_tensor(fx["obs"], device=dev))
    got = np.stack([res[name].cpu().numpy() for name in engine.SEL_PLANES])
    check_planes(got, fx, "n_pi=4")
    assert np.array_equal(got, device_planes, equal_nan=True)


def test_fisher_elementwise_against_the_80_digit_table(fx):
    import torch
    from digdriver_amd.sequence_model import nb_model
    got = nb_model.fisher_combine(fx["fisher_p1"], fx["fisher_p2"])
    dev = nb_model.fisher_combine(torch.as_tensor(fx["fisher_p1"], device="cuda:0"), torch.as_tensor(fx["fisher_p2"], device="cuda:0"))
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), got, equal_nan=True)
    check_fisher(got, fx, "dig_fisher")


def test_fused_statistics_combine_as_the_elementwise_entry_point(fx):
    """The fused statistics form their two p-values themselves, so the table cannot be fed to them: their combined plane has to
    be, bit for bit, dig_fisher of their own two planes -- on the pair table of nb_routes_golden.npz, whose values reach 1e-291 and
    put products on both sides of 1e-290 and a few results below 1e-305."""
    import os
    import torch
    from conftest import GOLDEN
    from digdriver_amd import engine
    from digdriver_amd.sequence_model import nb_model
    r = dict(np.load(os.path.join(GOLDEN, "nb_routes_golden.npz")))
    dev = torch.device("cuda:0")
    C = 5
    n_pair, singles = len(r["pair_k1"]), np.flatnonzero(np.isfinite(r["mu"]))
    order = singles[np.argsort(r["midp_upper"][singles])]                       # small indel values beside small SNV values
    by_pair = np.argsort(np.minimum(r["pair_midp_upper1"], r["pair_midp_upper2"]))
    E = -(-n_pair // C)
    pi = by_pair[np.arange(E * C) % n_pair].reshape(E, C)
    si = order[(np.arange(E * C) * len(order) // (E * C))].reshape(E, C)
    t = lambda v, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(v), dtype=dt, device=dev)
    es = engine.element_stats(t(r["pair_mu"][pi]), t(r["pair_sigma"][pi]), t(np.ones((E, C))), t(np.ones(E)), t(r["pair_k1"][pi], torch.int32),
                              t(r["pair_k2"][pi], torch.int32), t(r["k"][si], torch.int32), t(np.ones(C)), t(np.ones(C)),
                              mu_indel=t(r["mu"][si]), sigma_indel=t(r["sigma"][si]))
    zero = np.zeros((E, C))
    obs = np.stack([zero, zero, r["pair_k1"][pi], zero, r["k"][si]], axis=1)     # TRUNC = NONS + SPL carries k1
    gs = engine.gene_stats(t(r["pair_mu"][pi]), t(r["pair_sigma"][pi]), t(np.ones((E, 6, C))), t(np.ones(E)), t(obs, torch.int32),
                           t(np.zeros((E, 6, C)), torch.int32), t(np.ones(C)), t_indel=t(np.ones(C)), mu_indel=t(r["mu"][si]),
                           sigma_indel=t(r["sigma"][si]))
    torch.cuda.synchronize()
    for what, res, a in (("element_stats", es, "PVAL_SNV_BURDEN"), ("gene_stats", gs, "PVAL_TRUNC_BURDEN")):
        p1, p2, mut = (res[n].cpu().numpy() for n in (a, "PVAL_INDEL_BURDEN", "PVAL_MUT_BURDEN"))
        q = p1 * p2
        above, below = int(((q > 1e-290) & (q < 1e-200)).sum()), int(((q <= 1e-290) & (q > 0)).sum())
        deep = int(((mut > 0) & (mut < 1e-305)).sum())          # where fisher_combine takes one exponential of log1p(h) - h
        print("%s: %d products in 1e-290 .. 1e-200, %d in (0, 1e-290]; %d results in (0, 1e-305)" % (what, above, below, deep))
        assert above >= 5 and below >= 5 and deep >= 3, what
        assert np.array_equal(mut, nb_model.fisher_combine(p1, p2), equal_nan=True), what
