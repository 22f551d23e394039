"""The fixture of tests/test_gpu_gene_selection_routes.py checked on its own (no GPU), and the proof that its checker has teeth:
tests/golden/gene_selection_routes_golden.npz (tests/golden/make_gene_selection_routes_golden.py) holds the inputs, the 14
arithmetic planes of dig_gene_selection as numpy forms them one operation at a time, and 80-digit references of its 20 p-value
planes.  check_planes() is the one checker of both tests:

  arithmetic planes (T_SYN, MRFOLD, EXP_c_ML, SEL_c)   bit for bit
  likelihood-ratio planes                               |got / want - 1| <= M 2^-53 (1 + A S) per pair, + 4 x 2^-1074 absolute where
                                                        the reference is subnormal; 0 where it is 0; NaN where it is NaN
  burden planes                                         STRICT of test_gpu_nb_routes.py (1e-7, floor 1e-250)

M = 16: the worst ratio of the double restatement on this machine's C library against the 80-digit values is 3.27 (the maker
prints it per group), times 4 for a device library specified to a few ulp, rounded up to a power of two.  M_F = 8 for Fisher's
method (1.76 the same way, bound M_F 2^-53 (1 + h)).  DESIGN.md 5.2 has the figures of the MI355X run.

The mutants of restate() below are each rejected under the name of a plane and a group.  Two of the list the fixture was written
for cannot be rejected by any test, because they compute the same function: `x <= 0 -> 1` for `x < 0 -> 1` (erfc(0) = exp(0) = 1)
and fmax(1e-10, r) for Python's max(1e-10, r) (both give 1e-10 for a NaN r; they differ only with NaN as the FIRST argument).
The test asserts that they give the same bits on all pairs -- which include x = 0 exactly and a NaN ratio -- and rejects the
nearest form that does differ, numpy's NaN-propagating maximum.  fma_sel_denominator is a contraction the compiler could make
without the pragma: ex + 1e-16 as fma(rate, Pi_c, 1e-16), emulated with Fraction.  (The other product-plus-add of the kernel,
kt - lam + k of pois_llr, would move a likelihood-ratio plane by at most half an ulp of lam, far inside M: no test at this bound
sees it.)  fma_ex_ml and fma_t_syn round once where the kernel rounds twice or more: rate Pi_c MRFOLD as one product, and T_SYN's
quotient with 1 + 1 / tps kept exact.
"""
import importlib.util
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, rel_close
from test_gpu_nb_routes import STRICT

M = 16.0
M_F = 8.0


def load_maker():
    name = "make_gene_selection_routes_golden"
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_fixture():
    d = dict(np.load(os.path.join(GOLDEN, "gene_selection_routes_golden.npz"), allow_pickle=False))
    d["maker"] = load_maker()
    return d


def check_planes(got, fx, what="", burden=True):
    """got [34, G, C] against the fixture; prints the worst figure per plane and group and raises with every (plane, group) that
    misses its bound."""
    mk = fx["maker"]
    names, groups = [str(s) for s in fx["plane_names"]], [str(s) for s in fx["group_names"]]
    got = np.asarray(got, np.float64)
    want, check, group = fx["want"], fx["check"] == 1, fx["group"]
    assert got.shape == want.shape
    failures = []
    lr_at = {q: j for j, q in enumerate(mk.LR)}
    for q, name in enumerate(names):
        for gi, gname in enumerate(groups):
            m = (group == gi) & check[q]
            if not m.any():
                continue
            g, w = got[q][m], want[q][m]
            if q in mk.ARITH:
                bad = ~((g == w) | (np.isnan(g) & np.isnan(w)))
                print("%s %-22s %-16s pairs %4d  differing in their bits %d" % (what, name, gname, int(m.sum()), int(bad.sum())))
                if bad.any():
                    i = int(np.flatnonzero(bad)[0])
                    failures.append("%s, group %s: %d of %d pairs differ in their bits (first: got %r, want %r)" %
                                    (name, gname, int(bad.sum()), int(m.sum()), float(g[i]), float(w[i])))
            elif q in lr_at:
                r = mk.ratios(g, w, fx["AS"][lr_at[q]][m])
                worst = float(r.max())
                print("%s %-22s %-16s pairs %4d  worst ratio %.3g of M = %g" % (what, name, gname, int(m.sum()), worst, M))
                if not worst <= M:
                    i = int(np.argmax(r))
                    failures.append("%s, group %s: ratio %.3g > M = %g (got %r, want %r, 1 + A S = %.3g)" %
                                    (name, gname, worst, M, float(g[i]), float(w[i]), 1.0 + float(fx["AS"][lr_at[q]][m][i])))
            elif burden:
                big = np.abs(w) >= 1e-250
                with np.errstate(all="ignore"):
                    worst = float(np.nanmax(np.abs(g[big] - w[big]) / np.abs(w[big]))) if big.any() else 0.0
                print("%s %-22s %-16s pairs %4d  worst rel %.3g (STRICT %g)" % (what, name, gname, int(m.sum()), worst, STRICT))
                try:
                    rel_close(g, w, STRICT)
                except AssertionError as exc:
                    failures.append("%s, group %s: %s" % (name, gname, exc))
    if failures:                                   # (raised by hand: pytest truncates the message of a rewritten assert)
        raise AssertionError("\n".join(failures))


def check_fisher(got, fx, what=""):
    mk = fx["maker"]
    h = np.where(np.isfinite(fx["fisher_h"]), fx["fisher_h"], 0.0)
    r = mk.ratios(got, fx["fisher_want"], h)
    print("%s Fisher rows %d  worst ratio %.3g of M_f = %g" % (what, len(r), float(r.max()), M_F))
    bad = np.flatnonzero(~(r <= M_F))
    if len(bad):
        raise AssertionError("\n".join("Fisher(%r, %r): got %r, want %r, ratio %.3g > M_f = %g" % (
        float(fx["fisher_p1"][i]), float(fx["fisher_p2"][i]), float(np.asarray(got)[i]), float(fx["fisher_want"][i]), float(r[i]), M_F)
        for i in bad[:10]))


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.fixture(scope="module")
def restated(fx):
    return fx["maker"].restate(fx["alpha"], fx["theta"], fx["pi"], fx["obs"])


def test_fixture_shape_counts_and_intermediates(fx, restated):
    mk = fx["maker"]
    G, C = fx["alpha"].shape
    assert C == 3 and (G * C) % 256 != 0 and G * C >= 1000
    assert [str(s) for s in fx["group_names"]] == mk.GROUPS and [str(s) for s in fx["plane_names"]] == list(mk.PLANES)
    from digdriver_amd import _lib
    assert list(mk.PLANES) == list(_lib.SEL_PLANES)
    assert os.path.getsize(os.path.join(GOLDEN, "gene_selection_routes_golden.npz")) <= 571160
    # group counts as the maker printed them
    want = dict(regular=(450, 450, 450), ratio_near_zero=(162, 162, 162), deep_tail=(90, 90, 90), small_theta_pi=(90, 90, 90),
                alpha_le_1=(80, 80, 80), mrfold_floor=(72, 72, 72), near_poisson=(72, 72, 72), gamma_poisson=(84, 83, 83),
                burden=(133, 133, 131))
    for gi, name in enumerate(mk.GROUPS):
        got = (int(fx["candidates_per_group"][gi]), int(fx["drawn_per_group"][gi]), int(fx["kept_per_group"][gi]))
        assert got == want[name], (name, got)
        assert int((fx["group"] == gi).sum()) == got[2]
        assert got[0] - got[1] <= 0.02 * got[0], name          # the cap on uninformative pairs
    # no pair that is kept has a bound above 1e-9 at the M the maker capped with, and M is within it
    assert M <= mk.M_CAP
    zero = fx["want"][mk.LR] == 0
    assert ((mk.M_CAP * mk.U * (1.0 + fx["AS"].astype(np.float64)) <= mk.BOUND_CAP * (1 + 1e-6)) | zero).all()
    # Pi differs between the cohorts of a gene; the sums are the sums everywhere (so n_pi = 4 serves every pair)
    assert (fx["pi"][:, :4, 0] != fx["pi"][:, :4, 1]).any(axis=1).mean() > 0.9
    assert bool(fx["pi_sums"][0])
    # the doubles at which the 80-digit part started are the ones numpy forms here
    for n in mk.SUMMED:
        assert mk.sum64(restated[n]) == fx["sum64_" + n], n
    # what the groups are for
    grp = lambda n: fx["group"] == mk.GROUPS.index(n)
    w = fx["want"]
    lr = w[mk.LR]
    assert ((lr > 0) & (lr < 2.3e-308))[:, grp("deep_tail")].sum() >= 10 and (lr == 0)[:, grp("deep_tail")].sum() >= 10
    for lo, hi in ((1e-101, 1e-99), (1e-250, 1e-248), (1e-252, 1e-250), (1e-301, 1e-299)):
        assert ((lr > lo) & (lr < hi))[:, grp("deep_tail")].sum() >= 3, lo
    assert fx["obs"].max() == 9000
    assert (w[1] == 1e-10)[grp("mrfold_floor")].sum() >= 20 and ((w[1] > 1e-10) & (w[1] < 1.002e-10))[grp("mrfold_floor")].sum() >= 20
    assert (lr == 1.0)[:, grp("ratio_near_zero")].sum() >= 12          # x = 0 exactly
    assert np.isnan(w[18:22][:, grp("gamma_poisson")]).any() and not np.isnan(w[18:22][:, ~grp("gamma_poisson")]).any()
    with np.errstate(all="ignore"):
        assert np.isnan(restated["t_syn"] / (restated["rate"] * fx["pi"][:, 0])).any()              # a NaN ratio under the max
    tp = restated["tp"][:, grp("small_theta_pi")]
    assert tp.min() < 2e-15 and ((restated["p0_sel"] < 1) | (restated["k"] == 0)).all()
    a = fx["alpha"][grp("alpha_le_1")]
    assert set(np.unique(a)) == {0.25, 1.0 - 2.0 ** -53, 1.0, 1.0 + 2.0 ** -52, 1.5}
    kb = fx["obs"][:, 1, :][grp("burden")]
    assert {0, 1, 64, 65, 128, 129, 2048, 2049, 5000} <= set(kb.tolist())
    with np.errstate(all="ignore"):
        lp0 = (fx["alpha"] * np.log(restated["p"][1]))[grp("burden")]
    for centre in (-200.0, -400.0, -500.0):
        assert ((lp0 > centre) & (lp0 < 0.99 * centre)).sum() >= 3 and ((lp0 <= centre) & (lp0 > 1.01 * centre)).sum() >= 3, centre
    v = w[9][grp("burden")]
    assert ((v > 5e-7) & (v < 1e-6)).sum() >= 3 and ((v >= 1e-6) & (v < 2e-6)).sum() >= 3


def test_double_restatement_passes_and_matches_the_recorded_figures(fx, restated):
    from oracle import dig_oracle as O
    mk = fx["maker"]
    planes = restated["planes"].copy()
    with np.errstate(all="ignore"):
        planes[mk.BURDEN] = O.nb_pvalue_greater_midp(restated["k"], fx["alpha"][None], restated["p"])
    check_planes(planes, fx, "restatement")
    r = mk.ratios(planes[mk.LR], fx["want"][mk.LR], fx["AS"])
    r = np.where(fx["check"][mk.LR] == 1, r, 0.0)
    for gi, name in enumerate(mk.GROUPS):
        worst = float(r[:, fx["group"] == gi].max())
        assert worst <= 1.0001 * float(fx["cpu_worst_ratio_per_group"][gi]) + 0.5, (name, worst)     # (+ 0.5: another C library's last bits)
    assert mk.pow2_ceil(4 * float(fx["cpu_worst_ratio_per_group"].max())) == M
    assert mk.pow2_ceil(4 * float(fx["fisher_cpu_worst_ratio"].max())) == M_F
    check_fisher(mk.fisher_restate(fx["fisher_p1"], fx["fisher_p2"]), fx, "restatement")


MUTANTS = [("fma_sel_denominator", "SEL_"), ("fma_ex_ml", "EXP_"), ("fma_t_syn", "T_SYN"), ("log1p_theta", "PVAL_"), ("erfc_1e-9", "PVAL_"), ("pi_next_cohort", "EXP_"),
           ("maximum_mrfold", "MRFOLD")]


@pytest.mark.parametrize("mutant,plane", MUTANTS, ids=[m for m, _ in MUTANTS])
def test_mutant_is_rejected_under_a_plane_and_group(fx, mutant, plane):
    mk = fx["maker"]
    planes = mk.restate(fx["alpha"], fx["theta"], fx["pi"], fx["obs"], mutant=mutant)["planes"]
    with pytest.raises(AssertionError) as exc:
        check_planes(planes, fx, mutant, burden=False)
    lines = str(exc.value).split("\n")
    assert any(ln.startswith(plane) and ", group " in ln for ln in lines), lines[:5]
    groups = [str(s) for s in fx["group_names"]]
    assert all(ln.split(", group ")[1].split(":")[0] in groups for ln in lines)


@pytest.mark.parametrize("mutant", ["x_le_0", "fmax_mrfold"])
def test_equivalent_mutant_gives_the_same_bits(fx, restated, mutant):
    """Not rejected, and not rejectable: see the module docstring."""
    planes = fx["maker"].restate(fx["alpha"], fx["theta"], fx["pi"], fx["obs"], mutant=mutant)["planes"]
    assert np.array_equal(planes, restated["planes"], equal_nan=True)
    with np.errstate(all="ignore"):
        assert (restated["planes"][fx["maker"].LR] == 1.0).sum() >= 12 and np.isnan(restated["t_syn"] / (restated["rate"] * fx["pi"][:, 0])).any()


def test_fisher_table_covers_the_switch(fx):
    p1, p2, want = fx["fisher_p1"], fx["fisher_p2"], fx["fisher_want"]
    with np.errstate(all="ignore"):
        q = p1 * p2
    assert ((q > 1e-290) & (q < 2.1e-290)).sum() >= 10 and ((q <= 1e-290) & (q > 0.49e-290)).sum() >= 10
    assert ((p1 == 1) | (p2 == 1)).sum() >= 5 and ((p1 > 1) | (p2 > 1)).sum() >= 5 and np.isnan(want).sum() == 3
    assert ((q == 0) & (p1 > 0) & (p2 > 0)).sum() >= 4 and ((want > 0) & (want < 2.3e-308)).sum() >= 8 and (want == 0).sum() >= 4
    # a 1e-9 error on the logarithm of the fast form, and the product form the kernel had below 1e-305, are both rejected
    mk = fx["maker"]
    with np.errstate(all="ignore"):
        h = -(np.log(p1) + np.log(p2))
        old = np.where(np.isnan(h), np.nan, np.where(h < 0, 1.0, np.where(np.isinf(h), 0.0, np.exp(-h) * (1.0 + h))))
    with pytest.raises(AssertionError):
        check_fisher(old, fx, "exp(-h) (1 + h)")
    with pytest.raises(AssertionError):
        check_fisher(mk.fisher_restate(p1, p2) * (1 + 1e-9), fx, "1e-9")
