"""Every route of the negative-binomial p-value dispatch (csrc/dig_math.hpp) at its switch points, against the 80-digit
reference of tests/golden/nb_routes_golden.npz (tests/golden/make_nb_routes_golden.py; tests/test_nb_routes_fixture.py checks the
fixture itself on the CPU).  The random sweeps of test_gpu_parity.py compare with scipy at 1e-6 and put a handful of rows, or
none, next to a threshold; here the rows sit ON the thresholds and every route is asserted under its own name, against

  the contract   1e-6 relative for reference values >= 1e-250, both sides below 1e-250 otherwise (conftest.rel_close), and
  STRICT = 1e-7  relative for reference values >= 1e-250: the sum of the bounds dig_math.hpp states for its own routes, rounded up
                 (5e-8 from the incremental u += x of the fast recurrence + 7e-9 at its acceptance edge; 2e-9 for the rescaled
                 recurrence; ~(number of terms) ulp for the series; 3e-10 for the saddle-point pmf).

Each check prints one line per route (rows, worst relative error at >= 1e-250 and in 1e-290 .. 1e-250, which is reported and not
asserted); DESIGN.md section 5.1 records the figures of the MI355X run.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, rel_close

pytestmark = pytest.mark.gpu

CONTRACT = 1e-6
STRICT = 1e-7
DIRECT_MIN = 1e-6          # kDirectMin


@pytest.fixture(scope="module")
def fx():
    d = dict(np.load(os.path.join(GOLDEN, "nb_routes_golden.npz")))
    k, geq, pmf = d["k"], d["geq"], d["pmf"]
    d["greater"] = np.where(k == 0, 1.0, np.where(geq == 0, pmf, geq))          # nb_model.py:243-256 on the stored doubles
    d["fused"] = np.isfinite(d["mu"])                                            # rows the parameter transform reaches
    return d


@pytest.fixture(scope="module")
def dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def worst_rel(got, want, lo, hi=np.inf):
    m = (np.abs(want) >= lo) & (np.abs(want) < hi)
    if not m.any():
        return 0.0
    with np.errstate(all="ignore"):
        return float(np.nanmax(np.abs(got[m] - want[m]) / np.abs(want[m])))


def check_by_label(what, got, want, label, names):
    """The two bounds per label; prints the figures and returns the list of failures (label named in each)."""
    got, want, label = np.asarray(got, float).ravel(), np.asarray(want, float).ravel(), np.asarray(label).ravel()
    failures = []
    for r, name in enumerate(names):
        m = label == r
        if not m.any():
            continue
        print("%-40s %-20s rows %5d  worst rel %.3g  (1e-290..1e-250: %.3g)" %
              (what, name, int(m.sum()), worst_rel(got[m], want[m], 1e-250), worst_rel(got[m], want[m], 1e-290, 1e-250)))
        for bound, title in ((CONTRACT, "contract 1e-6"), (STRICT, "strict 1e-7")):
            try:
                rel_close(got[m], want[m], bound)
            except AssertionError as exc:
                rows = np.flatnonzero(m)
                failures.append("%s, route %s, %s: %s (first row of the route: %d)" % (what, name, title, exc, int(rows[0])))
                break
    return failures


ENTRY_POINTS = [("nb_pvalue_greater_midp", "midp_upper"), ("nb_pvalue_greater", "greater"), ("nb_pvalue_exact", "exact"),
                ("nb_pvalue_midp", "midp")]


@pytest.mark.parametrize("entry,ref", ENTRY_POINTS)
def test_elementwise_entry_point_by_route(fx, dev, entry, ref):
    import torch
    from digdriver_amd.sequence_model import nb_model
    fn = getattr(nb_model, entry)
    got = fn(fx["k"], fx["alpha"], fx["p"])
    got_dev = fn(*[torch.as_tensor(fx[n], device=dev) for n in ("k", "alpha", "p")])
    assert got_dev.is_cuda
    assert np.array_equal(got_dev.cpu().numpy(), got, equal_nan=True), "host arrays and device tensors differ"
    failures = check_by_label(entry, got, fx[ref], fx["route"], list(fx["route_names"]))
    assert not failures, "\n".join(failures)


# ---- fused kernels: the pair table (one recurrence per pair) and the single-count table as the indel test ------------------
def pair_labels(fx):
    """Per count of a pair: its own path; and whether BOTH counts are accepted by the shared fast recurrence (with a margin
    at the two thresholds, where the last bit decides)."""
    k1, k2, v1, v2 = fx["pair_k1"], fx["pair_k2"], fx["pair_midp_upper1"], fx["pair_midp_upper2"]
    lp0 = fx["pair_alpha"] * np.log(fx["pair_p"])
    kmax = np.maximum(k1, k2)
    lp0_min = np.where(kmax <= 64, -400.0, -200.0)
    both_fast = (kmax <= 128) & (lp0 > lp0_min + 1e-6) & (v1 >= DIRECT_MIN * 1.00001) & (v2 >= DIRECT_MIN * 1.00001)
    return both_fast


def layout(fx, C):
    """Row indices [E, C] into the pair table and into the fused-reachable singles, E the smallest that holds both."""
    n_pair = len(fx["pair_k1"])
    singles = np.flatnonzero(fx["fused"])
    E = -(-max(n_pair, len(singles)) // C)
    pi = (np.arange(E * C) % n_pair).reshape(E, C)
    si = singles[np.arange(E * C) % len(singles)].reshape(E, C)
    return E, pi, si


@pytest.fixture(scope="module")
def elementwise_midp(fx, dev):
    """nb_pvalue_greater_midp on the pair table's counts and on the singles: what the fused planes must equal bit for bit where
    the fast recurrence accepts."""
    from digdriver_amd.sequence_model import nb_model
    f = nb_model.nb_pvalue_greater_midp
    return dict(pair1=f(fx["pair_k1"], fx["pair_alpha"], fx["pair_p"]), pair2=f(fx["pair_k2"], fx["pair_alpha"], fx["pair_p"]),
                single=f(fx["k"], fx["alpha"], fx["p"]))


def check_fused(what, fx, ew, pi, si, snv, smp, ind):
    names, paths = list(fx["route_names"]), list(fx["path_names"])
    failures = []
    failures += check_by_label(what + " k1", snv, fx["pair_midp_upper1"][pi], fx["pair_path1"][pi], paths)
    failures += check_by_label(what + " k2", smp, fx["pair_midp_upper2"][pi], fx["pair_path2"][pi], paths)
    failures += check_by_label(what + " indel", ind, fx["midp_upper"][si], fx["route"][si], names)
    both = pair_labels(fx)[pi]
    assert both.sum() >= 40
    if not np.array_equal(snv[both], ew["pair1"][pi][both]) or not np.array_equal(smp[both], ew["pair2"][pi][both]):
        failures.append("%s: pairs accepted by the fast recurrence differ from nb_pvalue_greater_midp in their bits" % what)
    acc = ((fx["path"] == 0) & (fx["midp_upper"] >= DIRECT_MIN * 1.00001) &
           (fx["alpha"] * np.log(np.where(fx["p"] < 1, fx["p"], 0.5)) > np.where(fx["k"] <= 64, -400.0, -200.0) + 1e-6))[si]
    assert acc.sum() >= 40
    if not np.array_equal(ind[acc], ew["single"][si][acc]):
        failures.append("%s: single counts accepted by the fast recurrence differ from nb_pvalue_greater_midp in their bits" % what)
    return failures


@pytest.mark.parametrize("C", [5, 37])
@pytest.mark.parametrize("use_workspace", [True, False], ids=["compacted", "inline"])
def test_element_stats_pairs_by_route(fx, dev, elementwise_midp, C, use_workspace):
    import torch
    from digdriver_amd import engine
    from oracle import dig_oracle as O
    E, pi, si = layout(fx, C)
    t = lambda v, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(v), dtype=dt, device=dev)
    one = np.ones((E, C))
    r = engine.element_stats(t(fx["pair_mu"][pi]), t(fx["pair_sigma"][pi]), t(one), t(np.ones(E)), t(fx["pair_k1"][pi], torch.int32),
                             t(fx["pair_k2"][pi], torch.int32), t(fx["k"][si], torch.int32), t(np.ones(C)), t(np.ones(C)),
                             mu_indel=t(fx["mu"][si]), sigma_indel=t(fx["sigma"][si]), use_workspace=use_workspace)
    torch.cuda.synchronize()
    snv, smp, ind = (r[n].cpu().numpy() for n in ("PVAL_SNV_BURDEN", "PVAL_SAMPLE_BURDEN", "PVAL_INDEL_BURDEN"))
    what = "element_stats C=%d %s" % (C, "compacted" if use_workspace else "inline")
    failures = check_fused(what, fx, elementwise_midp, pi, si, snv, smp, ind)
    with np.errstate(all="ignore"):                              # the combination of two checked planes: the contract
        rel_close(r["PVAL_MUT_BURDEN"].cpu().numpy(), O.fisher_combine(fx["pair_midp_upper1"][pi], fx["midp_upper"][si]), CONTRACT)
    assert not failures, "\n".join(failures)


def test_gene_stats_pairs_by_route(fx, dev, elementwise_midp):
    """dig_gene_stats: nb_midp_upper_fast2<1>(k1, k2, 3u, ...) + nb_midp_upper_unresolved.  SYN carries (k1, k2) as (count,
    samples), MIS the same pair the other way round, the indel block the single-count table."""
    import torch
    from digdriver_amd import engine
    C = 5
    G, pi, si = layout(fx, C)
    t = lambda v, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(v), dtype=dt, device=dev)
    k1, k2, k3 = fx["pair_k1"][pi], fx["pair_k2"][pi], fx["k"][si]
    zero = np.zeros((G, C))
    obs = np.stack([k1, k2, zero, zero, k3], axis=1)                       # SYN, MIS, NONS, SPL, INDEL
    n_samp = np.stack([k2, k1, zero, zero, zero, k1], axis=1)              # ... TRUNC, NONSYN (= MIS here: the pair again)
    r = engine.gene_stats(t(fx["pair_mu"][pi]), t(fx["pair_sigma"][pi]), t(np.ones((G, 6, C))), t(np.ones(G)), t(obs, torch.int32),
                          t(n_samp, torch.int32), t(np.ones(C)), t_indel=t(np.ones(C)), mu_indel=t(fx["mu"][si]),
                          sigma_indel=t(fx["sigma"][si]))
    torch.cuda.synchronize()
    g = lambda n: r[n].cpu().numpy()
    failures = check_fused("gene_stats SYN", fx, elementwise_midp, pi, si, g("PVAL_SYN_BURDEN"), g("PVAL_SYN_BURDEN_SAMPLE"),
                           g("PVAL_INDEL_BURDEN"))
    failures += check_fused("gene_stats MIS", fx, elementwise_midp, pi, si, g("PVAL_MIS_BURDEN_SAMPLE"), g("PVAL_MIS_BURDEN"),
                            g("PVAL_INDEL_BURDEN"))
    # OBS_NONSYN = MIS + TRUNC = k2, with k1 samples (all six class probabilities are given as 1, so every class shares p)
    failures += check_by_label("gene_stats NONSYN k2", g("PVAL_NONSYN_BURDEN"), fx["pair_midp_upper2"][pi], fx["pair_path2"][pi],
                               list(fx["path_names"]))
    assert not failures, "\n".join(failures)


def test_tiled_nb_test_by_route(fx, dev):
    """dig_tiled_nb_test (nb_exact) on the single-count table: one cohort, one tile per bin, tile probability 1."""
    import torch
    from digdriver_amd import engine
    rows = np.flatnonzero(fx["fused"])
    t = lambda v, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(v), dtype=dt, device=dev)
    pval, _ = engine.tiled_nb_test(t(np.ones((len(rows), 1))), t(fx["k"][rows][None, :, None], torch.int32), t(fx["mu"][rows][None, :]),
                                   t(fx["sigma"][rows][None, :]))
    torch.cuda.synchronize()
    failures = check_by_label("tiled_nb_test", pval.cpu().numpy().ravel(), fx["exact"][rows], fx["route"][rows],
                              list(fx["route_names"]))
    assert not failures, "\n".join(failures)
