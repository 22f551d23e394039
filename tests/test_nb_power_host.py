"""The power of the element route, the parts that need no GPU: the binding of dig_nb_power and its `_host` twin, every refusal of the
contract (include/dig_hip.h) before a device is touched, the ValueErrors of engine.nb_power, and the refusals of
cohort_batch.run_element_power and of `DigDriver.py elementCohorts --power` before a file is read."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
from digdriver_amd import _lib, engine
from test_row_select_host import _cli

NAME = "dig_nb_power"


def test_binding_facts():
    """The entry point and its twin are exported, declared and bound; the twin's signature is the entry point's with `device` for
    `stream`; the ABI version is the one of before."""
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dig_hip.h")).read()
    for sym in (NAME, NAME + "_host"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym) and sym + "(" in header
    assert _lib._SIGNATURES[NAME][-1] is ctypes.c_void_p and _lib._SIGNATURES[NAME + "_host"][-1] is ctypes.c_int
    assert _lib._SIGNATURES[NAME + "_host"][:-1] == _lib._SIGNATURES[NAME][:-1] and len(_lib._SIGNATURES[NAME]) == 13
    assert _lib._SIGNATURES[NAME][9] is ctypes.c_int32
    assert lib.dig_abi_version() == 12 and "#define DIG_ABI_VERSION 12" in header and _lib.ABI_VERSION == 12
    assert engine.NB_POWER_MAX_FOLDS == 8 and "#define DIG_NB_POWER_MAX_FOLDS 8" in header


def _call(suffix, alpha="x", theta="x", pi="x", scale=None, level="x", rows=1, n=1, folds="f", n_folds=1, k_max=5, k_crit="k", power="x"):
    """The entry point (suffix "") or its twin ("_host") on one-element host arrays ("x", "f", "k") or NULL (None): its status."""
    arrays = dict(x=np.full(1, 0.5), f=np.full(8, 2.0), k=np.zeros(1, np.int32))
    p = lambda v: None if v is None else _lib.host_ptr(arrays[v])
    return getattr(_lib.load(), NAME + suffix)(p(alpha), p(theta), p(pi), p(scale), p(level), rows, n, p(folds), n_folds, k_max, p(k_crit),
                                               p(power), None if suffix == "" else 0)


REFUSALS = [(dict(rows=-1), "rows, n >= 0"), (dict(n=-1), "rows, n >= 0"), (dict(n_folds=-1), "0 <= n_folds <= 8"),
            (dict(n_folds=9), "0 <= n_folds <= 8"), (dict(k_max=-1), "0 <= k_max <= 2^30"), (dict(k_max=(1 << 30) + 1), "0 <= k_max <= 2^30"),
            (dict(folds=None), "non-null folds"), (dict(power=None), "power non-null with n_folds > 0"),
            (dict(n_folds=0, folds=None), "NULL with n_folds = 0"), (dict(n=1 << 31), "fewer than 2^31 elements per row"),
            (dict(rows=1 << 31), "rows * chunks below 2^31"), (dict(rows=(1 << 31) // 4 + 1, n=3 * 256 + 1), "rows * chunks below 2^31"),
            (dict(alpha=None), "non-null alpha"), (dict(theta=None), "non-null alpha"), (dict(pi=None), "non-null alpha"),
            (dict(level=None), "non-null alpha"), (dict(k_crit=None), "non-null alpha")]


@pytest.mark.parametrize("suffix", ["", "_host"])
def test_every_refusal_comes_before_a_device_is_touched(suffix):
    """(Neither form gets as far as a launch or a staging copy: the pointers are host arrays, and this test runs without a GPU.)"""
    for kw, fragment in REFUSALS:
        assert _call(suffix, **kw) == -1, kw
        assert fragment in _lib.last_error() and _lib.last_error().startswith(NAME + suffix + ":"), (kw, _lib.last_error())
    # nothing to do: success on an empty problem, whatever the pointers
    for kw in (dict(rows=0), dict(n=0), dict(rows=0, n=0, n_folds=0, folds=None, power=None, k_max=0)):
        assert _call(suffix, **kw) == 0, kw
    lib = _lib.load()
    assert getattr(lib, NAME + suffix)(None, None, None, None, None, 0, 0, None, 0, 0, None, None, None if suffix == "" else 0) == 0


def test_the_twin_refuses_a_fold_that_is_not_finite_and_positive():
    lib = _lib.load()
    x, k = np.full(1, 0.5), np.zeros(1, np.int32)
    p = _lib.host_ptr
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        folds = np.array([2.0, bad, 5.0])
        assert lib.dig_nb_power_host(p(x), p(x), p(x), None, p(x), 1, 1, p(folds), 3, 5, p(k), p(np.zeros(3)), 0) == -1
        assert "dig_nb_power_host: requirement failed: folds finite and > 0" in _lib.last_error()
        assert lib.dig_nb_power_host(p(x), p(x), p(x), None, p(x), 0, 1, p(folds), 3, 5, p(k), p(np.zeros(3)), 0) == -1    # (empty or not)


def test_engine_raises_value_errors_without_a_device():
    a = np.full((2, 3), 0.5)
    for kw, match in ((dict(folds=(2.0, 0.0)), "folds: at most 8 finite numbers > 0"), (dict(folds=(float("nan"),)), "folds: at most 8"),
                      (dict(folds=tuple(range(1, 10))), "folds: at most 8"), (dict(k_max=-1), "k_max must be an integer"),
                      (dict(k_max=(1 << 30) + 1), "k_max must be an integer"), (dict(k_max=2.5), "k_max must be an integer")):
        with pytest.raises(ValueError, match=match):
            engine.nb_power(a, a, a, [0.1, 0.2], **kw)
    with pytest.raises(ValueError, match=r"alpha must be \[n\] or \[R, n\]"):
        engine.nb_power(a[None], a[None], a[None], 0.1)
    # no element: empty results of the right shapes, no device needed
    e = np.zeros((2, 0))
    got = engine.nb_power(e, e, e, [0.1, 0.2], scale=[1.0, 2.0], folds=(2.0, 5.0))
    assert got["k_crit"].shape == (2, 0) and got["k_crit"].dtype == np.int32 and got["power"].shape == (2, 2, 0)
    got = engine.nb_power(e[0], e[0], e[0], 0.1)
    assert got["k_crit"].shape == (0,) and got["power"] is None
    from digdriver_amd.sequence_model import nb_model
    assert nb_model.nb_critical_count(e[0], e[0], 0.05).shape == (0,)


def test_run_element_power_refuses_its_arguments_before_a_file_is_read():
    from digdriver_amd.driver_model import cohort_batch
    args = (["/nonexistent/a.txt", "/nonexistent/b.txt"], ["/nonexistent/a.h5", "/nonexistent/b.h5"], "/nonexistent/ed.h5", "elts")
    run = cohort_batch.run_element_power
    for kw in ({}, dict(pval_max=0.1, fdr=0.1), dict(fdr=0.1, bonferroni=0.05), dict(pval_max=1e-3, fdr=0.1, bonferroni=0.05)):
        with pytest.raises(ValueError, match="exactly one of pval_max, fdr and bonferroni"):
            run(*args, **kw)
    with pytest.raises(ValueError, match="PVAL_MUT_BURDEN has no critical count"):
        run(*args, fdr=0.1, cut_on="PVAL_MUT_BURDEN")
    with pytest.raises(ValueError, match="cut_on: one of PVAL_SNV_BURDEN, PVAL_SAMPLE_BURDEN, PVAL_INDEL_BURDEN"):
        run(*args, fdr=0.1, cut_on="PVAL")
    for folds in ((), (2.0, -1.0), (0.0,), (float("inf"),), tuple(range(1, 10)), (2.0, 2.0)):
        with pytest.raises(ValueError, match="folds: one to 8 different folds"):
            run(*args, fdr=0.1, folds=folds)
    for power_min in (0.0, 1.5, -0.1):
        with pytest.raises(ValueError, match="power_min: a power within"):
            run(*args, bonferroni=0.05, power_min=power_min)
    with pytest.raises(ValueError, match="labels: one label per cohort"):
        run(*args, pval_max=1e-3, labels=["A"])


def test_element_cohorts_power_is_refused_before_a_cohort_file_is_read():
    cli = _cli()
    base = "elementCohorts /nonexistent/ed.h5 elts --outdir /nonexistent/out --mutation-files a.txt b.txt --maps a.h5 b.h5 --outpfx A B "
    a = cli.parse_args(base + "--power --fdr 0.1 --power-folds 2 3.5 --power-min 0.9")
    assert a.power and a.power_folds == [2.0, 3.5] and a.power_min == 0.9 and a.bonferroni is None
    assert cli._power_options(a) == dict(pval_max=None, fdr=0.1, bonferroni=None, cut_on="PVAL_SNV_BURDEN", folds=(2.0, 3.5), power_min=0.9)
    a = cli.parse_args(base + "--power --bonferroni 0.05 --cut-on PVAL_SAMPLE_BURDEN")
    assert cli._power_options(a) == dict(pval_max=None, fdr=None, bonferroni=0.05, cut_on="PVAL_SAMPLE_BURDEN", folds=(2.0, 5.0, 10.0),
                                         power_min=0.8)
    b = cli.parse_args(base)
    assert not b.power and cli._power_options(b) is None
    for extra, match in (("--power", "--power needs exactly one of"), ("--power --fdr 0.1 --bonferroni 0.05", "--power needs exactly one of"),
                         ("--power --pval-max 1e-3 --bonferroni 0.05", "--power needs exactly one of"),
                         ("--power --pval-max 1e-3 --fdr 0.1", "at most one of --pval-max and --fdr"),
                         ("--bonferroni 0.05", "need --power"), ("--fdr 0.1 --power-folds 2", "need --power"), ("--power-min 0.5", "need --power"),
                         ("--power --bonferroni 0", "--bonferroni takes a level"), ("--power --bonferroni 1.5", "--bonferroni takes a level"),
                         ("--power --fdr 0.1 --power-folds 2 0", "--power-folds takes one to eight"),
                         ("--power --fdr 0.1 --power-folds -3", "--power-folds takes one to eight"),
                         ("--power --fdr 0.1 --power-folds 1 2 3 4 5 6 7 8 9", "--power-folds takes one to eight"),
                         ("--power --fdr 0.1 --power-min 0", "--power-min takes a power"), ("--power --fdr 0.1 --power-min 1.2", "--power-min takes a power"),
                         ("--power --fdr 0.1 --cut-on PVAL_MUT_BURDEN", "no critical count for --cut-on PVAL_MUT_BURDEN"),
                         ("--cut-on PVAL_SNV_BURDEN", "--cut-on needs --fdr or --pval-max")):
        with pytest.raises(SystemExit, match=match):
            cli.main(base + extra)
    assert not os.path.exists("/nonexistent/out")
