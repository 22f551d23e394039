"""The 80-digit table of Fisher's method over m = 3 .. 64 members (tests/golden/group_fisher_golden.npz, written by
tests/golden/make_group_fisher_golden.py) checked on its own, without a GPU, and the proof that its checker has teeth.

check_group_fisher() is the one checker of this test and of tests/test_gpu_group_fisher.py.  Every row of the table falls under one
of three clauses, none is left out:

    want = 0                     got = 0 exactly
    want subnormal               |got - want| <= 4 x 2^-1074 + M_G 2^-53 (1 + s) want
    otherwise                    |got / want - 1| <= M_G 2^-53 (1 + s)

M_G = 32: the worst ratio of the double restatement of the rule (the sum of -ln p in ascending order, Horner, one exponential of
log(r) - s; make_group_fisher_golden.restate) on this machine's C library against the 80-digit values is 6.35 (group one_extreme; the
maker prints it per group: uniform 1.26, log12 3.91, log300 3.71, one_extreme 6.35, subnormal_in 4.33, subnormal_out 1.43), times 4
for a device library specified to a few ulp, rounded up to a power of two.  DESIGN.md, section Meta-cohorts of the element route, has
the figure of the MI355X run.

Three mutants of the restatement are each rejected under their name: exp(-s) r in place of exp(log(r) - s) (a subnormal exp(-s) times
a large r), m counted with the NaN members, and a Horner recursion one term short."""
import importlib.util
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

M_G = 32.0


def load_maker():
    name = "make_group_fisher_golden"
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_fixture():
    mk = load_maker()
    d = mk.load()
    d["maker"] = mk
    return d


def check_group_fisher(got, fx, what=""):
    """got [N] against the table; prints the worst ratio per group and raises, under the name `what`, with the rows that miss M_G."""
    mk = fx["maker"]
    got = np.asarray(got, np.float64)
    assert got.shape == fx["want"].shape
    r = mk.ratios(got, fx["want"], fx["s"])
    for gi, name in enumerate(fx["group_names"]):
        k = fx["group"] == gi
        print("%s %-14s rows %4d  worst ratio %.3g of M_G = %g" % (what, name, int(k.sum()), float(r[k].max()), M_G))
    bad = np.flatnonzero(~(r <= M_G))
    if len(bad):
        raise AssertionError("%s: %d rows miss M_G\n" % (what, len(bad)) + "\n".join(
            "%s: row %d (group %s, m = %d, s = %r): got %r, want %r, ratio %.3g > M_G = %g" % (
                what, i, fx["group_names"][fx["group"][i]], int(fx["m"][i]), float(fx["s"][i]), float(got[i]), float(fx["want"][i]),
                float(r[i]), M_G) for i in bad[:10]))


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


def test_table_covers_what_it_was_written_for(fx):
    mk = fx["maker"]
    assert [str(s) for s in fx["group_names"]] == mk.GROUPS
    assert os.path.getsize(os.path.join(GOLDEN, "group_fisher_golden.npz")) <= 256 * 1024
    m, want, p, group = fx["m"], fx["want"], fx["p"], fx["group"]
    for gi in range(len(mk.GROUPS)):
        assert sorted(set(m[group == gi].tolist())) == list(range(3, 65)), mk.GROUPS[gi]
    assert ((~np.isnan(p)).sum(axis=1) == m).all() and np.isnan(p[np.arange(64)[None, :] >= m[:, None]]).all()
    grp = lambda n: group == mk.GROUPS.index(n)
    sub_in = (p > 0) & (p < mk.TINY)
    assert sub_in[grp("subnormal_in")].any(axis=1).all() and (np.nanmin(p[grp("log300")], axis=1) < 1e-100).mean() > 0.4
    assert ((want > 0) & (want < mk.TINY))[grp("subnormal_out")].all()
    assert (want == 0).sum() >= 50 and ((want > 0) & (want < 1e-250)).sum() >= 50 and (fx["s"] > 600).sum() >= 100
    assert (np.nanmin(p[grp("one_extreme")], axis=1) < 1e-200).all()
    # s is the sum of the logarithms rounded once: the doubles' own sequential sum lies within m ulp of it
    _, _, s = mk.restate(p)
    assert (np.abs(s - fx["s"]) <= m * 2.0 ** -52 * fx["s"]).all()


def test_double_restatement_passes_and_m_g_is_derived_from_it(fx):
    mk = fx["maker"]
    got, m, _ = mk.restate(fx["p"])
    assert np.array_equal(m, fx["m"])
    check_group_fisher(got, fx, "restatement")
    r = mk.ratios(got, fx["want"], fx["s"])
    for gi, name in enumerate(mk.GROUPS):
        worst = float(r[fx["group"] == gi].max())
        assert worst <= 1.0001 * float(fx["cpu_worst_ratio_per_group"][gi]) + 0.5, (name, worst)    # (+ 0.5: another C library's last bits)
    assert mk.pow2_ceil(4 * float(fx["cpu_worst_ratio_per_group"].max())) == M_G
    # got = 0 only where the reference rounds to 0
    assert np.array_equal(got == 0, fx["want"] == 0)


@pytest.mark.parametrize("mutant", ["exp_times_r", "m_with_nan", "horner_short"])
def test_mutant_of_the_restatement_is_rejected_by_name(fx, mutant):
    got, _, _ = fx["maker"].restate(fx["p"], mutant=mutant)
    with pytest.raises(AssertionError, match="^" + mutant + ": "):
        check_group_fisher(got, fx, mutant)


def test_checker_rejects_a_zero_for_a_subnormal_and_a_number_for_a_zero(fx):
    mk = fx["maker"]
    got, _, _ = mk.restate(fx["p"])
    sub = np.flatnonzero((fx["want"] > 8 * 2.0 ** -1074) & (fx["want"] < mk.TINY))
    zero = np.flatnonzero(fx["want"] == 0)
    assert len(sub) and len(zero)
    for i, v in ((sub[0], 0.0), (zero[0], 2.0 ** -1074), (0, np.nan)):
        bad = got.copy()
        bad[i] = v
        with pytest.raises(AssertionError, match="row %d " % i):
            check_group_fisher(bad, fx, "edge")
