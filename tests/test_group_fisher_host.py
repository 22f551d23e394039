"""The meta-cohorts of the element route, the parts that need no GPU: the binding of dig_group_fisher / dig_group_sums, the refusals of
their `_host` twins before a device is touched, the ValueErrors of engine.group_fisher / group_sums, the refusals of
cohort_batch.run_element_meta / run_element_meta_calls and of `DigDriver.py elementCohorts --groups` before a cohort's file is read,
and the numpy statements of tests/group_fisher_statement.py against each other."""
import ctypes
import os

import numpy as np
import pytest

import group_fisher_statement as S
from conftest import ROOT
from digdriver_amd import _lib
from test_row_select_host import _cli

NAMES = ("dig_group_fisher", "dig_group_sums")


def test_binding_facts():
    """Both entry points and their twins are exported and declared; a twin's signature is its entry point's with `device` for
    `stream`; the ABI version is the one of before."""
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dig_hip.h")).read()
    for name in NAMES:
        for sym in (name, name + "_host"):
            assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym) and sym + "(" in header
        assert _lib._SIGNATURES[name][-1] is ctypes.c_void_p and _lib._SIGNATURES[name + "_host"][-1] is ctypes.c_int
        assert _lib._SIGNATURES[name + "_host"][:-1] == _lib._SIGNATURES[name][:-1]
    assert [len(_lib._SIGNATURES[n]) for n in NAMES] == [9, 9]
    assert lib.dig_abi_version() == 12 and "#define DIG_ABI_VERSION 12" in header and _lib.ABI_VERSION == 12
    from digdriver_amd import engine
    assert engine.GROUPS_PER_LAUNCH == 32 and "M <= 32" in header and "C <= 64" in header


def test_host_twins_refuse_bad_sizes_and_missing_pointers_before_touching_a_device():
    lib = _lib.load()
    one, n1, m1 = np.full(1, 0.5), np.zeros(1, np.int32), np.ones(1, np.uint8)
    p = _lib.host_ptr
    big = (1 << 31) // 4 + 1                                             # R rows of four chunks: R * chunks = 2^31 + 4
    for (R, C, E, M), fragment in (((-1, 1, 1, 1), "R, C, E, M >= 0"), ((1, -1, 1, 1), "R, C, E, M >= 0"), ((1, 1, -1, 1), "R, C, E, M >= 0"),
                                   ((1, 1, 1, -1), "R, C, E, M >= 0"), ((1, 65, 1, 1), "C <= 64"), ((1, 1, 1, 33), "M <= 32"),
                                   ((1, 1, 1 << 31, 1), "fewer than 2^31 elements per row"), ((big, 1, 3 * 128 + 1, 1), "R * chunks below 2^31"),
                                   ((1 << 31, 1, 1, 1), "R * chunks below 2^31")):
        assert lib.dig_group_fisher_host(p(one), p(m1), R, C, E, M, p(one), p(n1), 0) == -1
        assert fragment in _lib.last_error() and "dig_group_fisher_host" in _lib.last_error(), _lib.last_error()
        assert lib.dig_group_sums_host(p(one), None, p(m1), R, C, E, M, p(one), 0) == -1
        assert fragment in _lib.last_error() and "dig_group_sums_host" in _lib.last_error(), _lib.last_error()
    for args in ((None, p(m1), p(one)), (p(one), None, p(one)), (p(one), p(m1), None)):
        assert lib.dig_group_fisher_host(args[0], args[1], 1, 1, 1, 1, args[2], p(n1), 0) == -1
        assert "non-null" in _lib.last_error() and "dig_group_fisher_host" in _lib.last_error()
        assert lib.dig_group_sums_host(args[0], None, args[1], 1, 1, 1, 1, args[2], 0) == -1
        assert "non-null" in _lib.last_error() and "dig_group_sums_host" in _lib.last_error()
    for R, C, E, M in ((0, 3, 5, 2), (2, 3, 0, 2), (2, 3, 5, 0)):        # nothing to do
        assert lib.dig_group_fisher_host(None, None, R, C, E, M, None, None, 0) == 0
        assert lib.dig_group_sums_host(None, None, None, R, C, E, M, None, 0) == 0


def test_engine_raises_value_errors_without_a_device():
    from digdriver_amd import engine
    p = np.full((65, 3), 0.5)
    with pytest.raises(ValueError, match="C <= 64"):
        engine.group_fisher(p, np.ones((1, 65)))
    with pytest.raises(ValueError, match="C <= 64"):
        engine.group_sums(p, np.ones((1, 65)))
    with pytest.raises(ValueError, match=r"member must be \[M, C\]"):
        engine.group_fisher(p[:3], np.ones((2, 4)))
    with pytest.raises(ValueError, match=r"\[C, E\] or \[R, C, E\]"):
        engine.group_sums(p[0], np.ones((1, 3)))
    with pytest.raises(ValueError, match="gate must have the shape of x"):
        engine.group_sums(p[:3], np.ones((1, 3)), gate=p[:2])
    # no group, no element: empty results of the right shapes, no device needed
    got = engine.group_fisher(p[:3], np.zeros((0, 3)))
    assert got["pval"].shape == (0, 3) and got["n_used"].shape == (0, 3) and got["n_used"].dtype == np.int32
    assert engine.group_sums(np.zeros((2, 3, 0)), np.ones((40, 3))).shape == (2, 40, 0)
    assert engine.group_fisher(np.zeros((3, 0)), np.ones((1, 3)), counts=False)["n_used"] is None


def test_run_element_meta_refuses_its_groups_before_a_file_is_read():
    from digdriver_amd.driver_model import cohort_batch
    args = (["/nonexistent/a.txt", "/nonexistent/b.txt"], ["/nonexistent/a.h5", "/nonexistent/b.h5"], "/nonexistent/ed.h5", "elts")
    for run, kw in ((cohort_batch.run_element_meta, {}), (cohort_batch.run_element_meta_calls, dict(fdr=0.1))):
        with pytest.raises(ValueError, match="at least one group"):
            run(*args, {}, **kw)
        with pytest.raises(ValueError, match="group 'g' is empty"):
            run(*args, {"g": []}, **kw)
        with pytest.raises(ValueError, match="unknown cohort label 'C'"):
            run(*args, {"g": ["A", "C"]}, labels=["A", "B"], **kw)
        with pytest.raises(ValueError, match="unknown cohort label 'A'"):
            run(*args, {"g": ["A"]}, **kw)
        with pytest.raises(ValueError, match="more than once"):
            run(*args, {"g": ["A", 0]}, labels=["A", "B"], **kw)
        with pytest.raises(ValueError, match=r"cohort index 2 outside \[0, 2\)"):
            run(*args, {"g": [0, 2]}, **kw)
        with pytest.raises(ValueError, match="one label per cohort"):
            run(*args, {"g": [0]}, labels=["A"], **kw)
    with pytest.raises(ValueError, match="exactly one of pval_max and fdr"):
        cohort_batch.run_element_meta_calls(*args, {"g": [0]})
    with pytest.raises(ValueError, match="cut_on: one of"):
        cohort_batch.run_element_meta_calls(*args, {"g": [0]}, fdr=0.1, cut_on="PVAL")
    with pytest.raises(ValueError, match="best_on: one of"):
        cohort_batch.run_element_meta(*args, {"g": [0]}, best_on="PVAL")


def test_element_cohorts_groups_are_refused_before_a_cohort_file_is_read(tmp_path):
    cli = _cli()
    base = "elementCohorts /nonexistent/ed.h5 elts --outdir /nonexistent/out --mutation-files a.txt b.txt --maps a.h5 b.h5 --outpfx A B "
    f = tmp_path / "groups.tsv"

    def run(text, extra=""):
        f.write_text(text)
        cli.main(base + "--groups %s %s" % (f, extra))

    a = cli.parse_args(base + "--groups g.tsv --fdr 0.1")
    assert a.groups == "g.tsv" and cli.parse_args(base).groups is None
    with pytest.raises(SystemExit, match="names no group"):
        run("")
    with pytest.raises(SystemExit, match="names no group"):
        run("# pan\tA\n\n")
    with pytest.raises(SystemExit, match="line 2: C is not one of --outpfx"):
        run("pan\tA\npan\tC\n")
    with pytest.raises(SystemExit, match="the group name B repeats a cohort prefix"):
        run("pan\tA\nB\tA\n", "--fdr 0.1")
    with pytest.raises(SystemExit, match="A is in group pan already"):
        run("pan\tA\npan\tA\n")
    with pytest.raises(SystemExit, match="two tab-separated columns"):
        run("pan A\n")
    f.write_text("pan\tA\n")
    with pytest.raises(SystemExit, match="must then differ"):
        cli.main(base.replace("--outpfx A B", "--outpfx A A") + "--groups %s" % f)
    assert cli._read_groups(str(f), ["A", "B"]) == {"pan": ["A"]}
    f.write_text("pan\tA\r\npan\tB\nsq\tB\n")
    assert list(cli._read_groups(str(f), ["A", "B"]).items()) == [("pan", ["A", "B"]), ("sq", ["B"])]
    assert not os.path.exists("/nonexistent/out")


def test_statements_agree_with_each_other():
    rng = np.random.default_rng(4)
    p = rng.uniform(size=(2, 5, 9))
    p[:, 1] = np.nan
    p[0, :, 3] = np.nan
    p[1, 2, 4] = np.nan
    member = np.array([[1, 1, 1, 1, 1], [0, 0, 0, 0, 0], [0, 0, 1, 0, 0], [1, 0, 0, 2, 0], [0, 1, 0, 0, 0], [1, 0, 0, 2, 0]])
    n = S.n_used(p, member)
    assert n.shape == (2, 6, 9) and n.dtype == np.int32 and (n[:, 1] == 0).all() and (n[:, 4] == 0).all() and n[0, 0, 3] == 0
    assert n[0, 0, 0] == 4 and n[1, 2, 4] == 0 and n[1, 2, 0] == 1 and np.array_equal(n[:, 3], n[:, 5])
    val, known = S.small_groups(p, member, lambda a, b: a * 100 + b)
    assert np.array_equal(known, n <= 2) and np.isnan(val[:, 1]).all() and np.isnan(val[~known]).all()
    assert val[1, 2, 0] == p[1, 2, 0] and np.isnan(val[1, 2, 4]) and val[0, 3, 0] == p[0, 0, 0] * 100 + p[0, 3, 0]
    assert np.isnan(val[0, 3, 3])
    x = rng.integers(0, 9, size=(2, 5, 9)).astype(float)
    sums = S.group_sums(x, member)
    assert np.array_equal(sums[:, 0], x.sum(axis=1)) and (sums[:, 1] == 0).all() and np.array_equal(sums[:, 3], x[:, 0] + x[:, 3])
    gated = S.group_sums(x, member, gate=p)
    assert np.array_equal(gated[:, 0], np.where(np.isnan(p), 0.0, x).sum(axis=1)) and (gated[0, :, 3] == 0).all()
    assert S.group_sums(x[0], member).shape == (1, 6, 9) and S.n_used(p, np.zeros((0, 5))).shape == (2, 0, 9)
