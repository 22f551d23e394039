"""The calls of the element route, the parts that need no GPU: the binding of dig_row_select_count / dig_row_select_fill /
dig_row_scatter and their size queries, the refusals of the three `_host` twins before a device is touched, the refusals of
`DigDriver.py elementCohorts` before a file is read, those of cohort_batch.run_element_calls before any work, and the numpy statements
of tests/row_select_statement.py against each other."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import row_select_statement as S
from conftest import ROOT
from digdriver_amd import _lib
from test_tile_hits_host import _random_list

NAMES = ("dig_row_select_count", "dig_row_select_fill", "dig_row_scatter")


def _cli():
    spec = importlib.util.spec_from_file_location("dig_driver_cli_element_cohorts", os.path.join(ROOT, "scripts", "DigDriver.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_binding_facts():
    """Every entry point, twin and size query is exported and declared; a twin's signature is its entry point's with `device` for
    `stream`; the chunk is a whole number of 16-byte pairs and the counts' size follows from it."""
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dig_hip.h")).read()
    for name in NAMES:
        for sym in (name, name + "_host"):
            assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym) and sym + "(" in header
        assert _lib._SIGNATURES[name][-1] is ctypes.c_void_p and _lib._SIGNATURES[name + "_host"][-1] is ctypes.c_int
        assert _lib._SIGNATURES[name + "_host"][:-1] == _lib._SIGNATURES[name][:-1]
    assert [len(_lib._SIGNATURES[n]) for n in NAMES] == [6, 9, 10]
    for sym in ("dig_row_select_chunk", "dig_row_select_counts_size"):
        assert sym in _lib._SIZE_QUERIES and hasattr(lib, sym) and sym + "(" in header
    K = int(lib.dig_row_select_chunk())
    assert K >= 128 and K % 2 == 0
    size = lib.dig_row_select_counts_size
    assert [int(size(r, n)) for r, n in ((0, 5), (3, 0), (1, 1), (3, K), (3, K + 1), (148, 120_091))] == \
        [0, 0, 1, 3, 6, 148 * -(-120_091 // K)]
    assert lib.dig_abi_version() == 12 and "#define DIG_ABI_VERSION 12" in header


def test_host_twins_refuse_bad_sizes_before_touching_a_device():
    """rows, n >= 0, n < 2^31, rows * chunks < 2^31 and total >= 0 are refused on the sizes alone; a missing pointer and offsets
    that are no prefix sum as well; empty inputs are nothing to do."""
    lib = _lib.load()
    K = int(lib.dig_row_select_chunk())
    one, i1, o1 = np.zeros(1), np.zeros(1, np.int32), np.zeros(1, np.int64)
    p = _lib.host_ptr
    many = (1 << 31) // 4 + 1                                         # rows of four chunks: rows * chunks = 2^31 + 4
    for rows, n, fragment in ((-1, 1, "rows, n >= 0"), (1, -1, "rows, n >= 0"), (1, 1 << 31, "fewer than 2^31 elements per row"),
                              (many, 3 * K + 1, "rows * chunks below 2^31"), (1 << 31, 1, "rows * chunks below 2^31")):
        assert lib.dig_row_select_count_host(p(one), p(one), rows, n, p(i1), 0) == -1
        assert fragment in _lib.last_error() and "dig_row_select_count_host" in _lib.last_error()
        assert lib.dig_row_select_fill_host(p(one), p(one), rows, n, p(o1), 1, p(i1), p(one), 0) == -1
        assert fragment in _lib.last_error() and "dig_row_select_fill_host" in _lib.last_error()
        assert lib.dig_row_scatter_host(p(one), p(one), rows, n, p(o1), 1, p(one), 0.0, p(one), 0) == -1
        assert fragment in _lib.last_error() and "dig_row_scatter_host" in _lib.last_error()
        assert int(lib.dig_row_select_counts_size(rows, n)) == -1
    assert lib.dig_row_select_fill_host(p(one), p(one), 1, 1, p(o1), -1, p(i1), p(one), 0) == -1 and "total >= 0" in _lib.last_error()
    assert lib.dig_row_scatter_host(p(one), p(one), 1, 1, p(o1), -1, p(one), 0.0, p(one), 0) == -1 and "total >= 0" in _lib.last_error()
    assert lib.dig_row_select_count_host(None, p(one), 1, 1, p(i1), 0) == -1 and "non-null" in _lib.last_error()
    assert lib.dig_row_select_fill_host(p(one), None, 1, 1, p(o1), 1, p(i1), p(one), 0) == -1 and "non-null" in _lib.last_error()
    assert lib.dig_row_scatter_host(p(one), p(one), 1, 1, p(o1), 1, p(one), 0.0, None, 0) == -1 and "non-null" in _lib.last_error()
    bad = np.array([0, 3, 2], np.int64)
    assert lib.dig_row_select_fill_host(p(np.zeros(3)), p(np.ones(3)), 3, 1, p(bad), 4, p(np.zeros(4, np.int32)), p(np.zeros(4)), 0) == -1
    assert "exclusive prefix sum" in _lib.last_error()
    assert lib.dig_row_scatter_host(p(np.zeros(3)), p(np.ones(3)), 3, 1, p(bad), 4, p(np.zeros(4)), 0.0, p(np.zeros(3)), 0) == -1
    assert "exclusive prefix sum" in _lib.last_error()
    assert lib.dig_row_select_count_host(None, None, 0, 7, None, 0) == 0                       # nothing to do
    assert lib.dig_row_select_count_host(None, None, 5, 0, None, 0) == 0
    assert lib.dig_row_select_fill_host(None, None, 2, 2, None, 0, None, None, 0) == 0
    assert lib.dig_row_scatter_host(None, None, 0, 2, None, 0, None, 0.0, None, 0) == 0


def test_element_cohorts_parses_and_refuses_before_reading_a_file():
    cli = _cli()
    a = cli.parse_args("elementCohorts ed.h5 elts --mutation-files a.txt b.txt --maps a.h5 b.h5 --outdir o --outpfx A B --fdr 0.1 "
                       "--cut-on PVAL_SAMPLE_BURDEN --scale-factor-manual 1 2 --scale-factor-indel-manual 3 4")
    assert a.func is cli.cmd_element_cohorts and (a.f_element_data, a.save_key) == ("ed.h5", "elts")
    assert a.mutation_files == ["a.txt", "b.txt"] and a.maps == ["a.h5", "b.h5"] and a.outpfx == ["A", "B"]
    assert (a.fdr, a.pval_max, a.cut_on, a.qvalues) == (0.1, None, "PVAL_SAMPLE_BURDEN", False)
    assert (a.scale_factor_manual, a.scale_factor_indel_manual) == ([1.0, 2.0], [3.0, 4.0])
    a = cli.parse_args("elementCohorts ed.h5 elts --mutation-files a.txt --maps a.h5 --outdir o --outpfx A --qvalues")
    assert (a.fdr, a.pval_max, a.cut_on, a.qvalues) == (None, None, None, True)
    assert (a.max_muts_per_sample, a.max_muts_per_elt_per_sample) == (3e9, 3e9)
    base = "elementCohorts /nonexistent/ed.h5 elts --outdir /nonexistent/out "
    one = base + "--mutation-files a.txt --maps a.h5 --outpfx A "
    with pytest.raises(SystemExit, match="same number of cohorts"):
        cli.main(base + "--mutation-files a.txt b.txt --maps a.h5 --outpfx A B --fdr 0.1")
    with pytest.raises(SystemExit, match="same number of cohorts"):
        cli.main(base + "--mutation-files a.txt b.txt --maps a.h5 b.h5 --outpfx A")
    with pytest.raises(SystemExit, match="one value per cohort"):
        cli.main(base + "--mutation-files a.txt b.txt --maps a.h5 b.h5 --outpfx A B --scale-factor-manual 1 --scale-factor-indel-manual 1 2")
    with pytest.raises(SystemExit, match="must specify both"):
        cli.main(one + "--scale-factor-manual 1")
    with pytest.raises(SystemExit, match="at most one of --pval-max and --fdr"):
        cli.main(one + "--pval-max 1e-3 --fdr 0.1")
    with pytest.raises(SystemExit, match="--cut-on needs --fdr or --pval-max"):
        cli.main(one + "--cut-on PVAL_SNV_BURDEN")
    for level in ("--fdr 0", "--fdr 1.5", "--pval-max 0", "--pval-max -0.1", "--pval-max 2"):
        with pytest.raises(SystemExit, match=r"a level within \(0, 1\]"):
            cli.main(one + level)
    with pytest.raises(SystemExit):                                                           # (argparse: not one of the four columns)
        cli.parse_args(one + "--fdr 0.1 --cut-on PVAL")
    assert not os.path.exists("/nonexistent/out")


def test_run_element_calls_refuses_both_cuts_and_no_cut_before_any_work():
    """No file exists and no device is needed: the cut is checked first."""
    from digdriver_amd.driver_model import cohort_batch
    args = (["/nonexistent/muts.txt"], ["/nonexistent/map.h5"], "/nonexistent/ed.h5", "elts")
    with pytest.raises(ValueError, match="exactly one of pval_max and fdr"):
        cohort_batch.run_element_calls(*args)
    with pytest.raises(ValueError, match="exactly one of pval_max and fdr"):
        cohort_batch.run_element_calls(*args, pval_max=1e-3, fdr=0.1)
    with pytest.raises(ValueError, match="cut_on: one of"):
        cohort_batch.run_element_calls(*args, fdr=0.1, cut_on="PVAL")


def test_statements_agree_with_each_other():
    """fill's lists have the lengths of counts, scatter undoes fill, and plane_qvalues of a row is get_q_vals of its NaN-dropped list."""
    from digdriver_amd.sequence_model import nb_model
    rng = np.random.default_rng(2)
    K = 16
    score = np.stack([_random_list(rng, 53) for _ in range(4)])
    score[2] = np.nan
    cut = np.array([np.inf, 0.3, np.inf, np.nan])
    index, vals, ptr = S.fill(score, cut)
    assert np.array_equal(S.counts(score, cut, K).reshape(4, -1).sum(axis=1), np.diff(ptr)) and ptr[-1] == len(index)
    assert ptr[3] == ptr[2] == ptr[4] and ptr[1] == (~np.isnan(score[0])).sum()
    back = S.scatter(score, cut, vals, -7.0)
    sel = S.selected(score, cut)
    assert np.array_equal(back[sel], score[sel]) and (back[~sel] == -7.0).all()
    q = S.plane_qvalues(score.reshape(2, 2, 53))
    assert np.isnan(q[1, 0]).all() and np.array_equal(np.isnan(q), np.isnan(score).reshape(2, 2, 53))
    ok = ~np.isnan(score[1])
    assert q[0, 1][ok].tobytes() == nb_model.get_q_vals(score[1][ok]).tobytes()
