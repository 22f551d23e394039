"""The map report, the parts that need no GPU: the binding of dig_map_windows / dig_map_scores and their `_host` twins, every refusal of
the contract (include/dig_hip.h) before a device is touched, the refusals of map_report.evaluate_maps and of `DigPretrain.py
evaluateMaps` before a file is written, and the numpy statement (map_report_statement.py, p-values by the test-side functions)
against the fixture made with the reference's own functions."""
import ctypes
import os

import numpy as np
import pandas as pd
import pytest

import map_report_cases as MC
import map_report_statement as S
from conftest import ROOT, rel_close
from digdriver_amd import _lib, engine
from digdriver_amd.io import mapfile
from test_sequence_models_host import _cli

WIN, SCO = "dig_map_windows", "dig_map_scores"


def test_binding_facts():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dig_hip.h")).read()
    for sym in (WIN, WIN + "_host", SCO, SCO + "_host", SCO + "_workspace"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym) and sym + "(" in header
    sig = _lib._SIGNATURES
    assert sig[WIN][-1] is ctypes.c_void_p and sig[WIN + "_host"][-1] is ctypes.c_int and sig[WIN + "_host"][:-1] == sig[WIN][:-1]
    assert len(sig[WIN]) == 16 and sig[WIN][8] is ctypes.c_int and sig[WIN][9] is ctypes.c_int
    assert len(sig[SCO]) == 11 and sig[SCO + "_host"] == sig[SCO][:8] + [ctypes.c_int]
    assert _lib._SIZE_QUERIES[SCO + "_workspace"] == [ctypes.c_int64, ctypes.c_int64]
    assert lib.dig_abi_version() == 12 and "#define DIG_ABI_VERSION 12" in header and _lib.ABI_VERSION == 12
    # the workspace: 11 eight-byte slots per (cohort, chunk of 1024 windows) and two per cohort; nothing for an empty problem
    ws = lib.dig_map_scores_workspace
    assert ws(37, 288000) == 37 * (282 * 88 + 16) and ws(1, 1) == 104 and ws(1, 1024) == 104 and ws(1, 1025) == 192 and ws(0, 5) == 0 and ws(5, 0) == 0
    assert engine.MAP_LEVELS == S.LEVELS and engine.MAP_TAILS == {"upper": 0, "side": 1}


_ARR = dict(d=np.full(4, 0.5), i=np.zeros(4, np.int32), l=np.zeros(4, np.int64), u=np.zeros(4, np.uint8), r=np.array([0, 1], np.int64),
            w=np.zeros(13, np.int64))
_p = lambda v: None if v is None else _lib.host_ptr(_ARR[v])


def _windows(suffix, mu="d", sd="d", y="i", flag="u", C=1, N=1, run_ptr="r", M=1, drop=0, tail=0, n_bins="i", y_true="l", y_pred="d", std="d",
             pval="d"):
    return getattr(_lib.load(), WIN + suffix)(_p(mu), _p(sd), _p(y), _p(flag), C, N, _p(run_ptr), M, drop, tail, _p(n_bins), _p(y_true),
                                              _p(y_pred), _p(std), _p(pval), None if suffix == "" else 0)


def _scores(suffix, n_bins="i", y_true="l", y_pred="d", pval="d", C=1, M=1, counts="w", sums="d", workspace="w", workspace_bytes=104):
    lib = _lib.load()
    args = (_p(n_bins), _p(y_true), _p(y_pred), _p(pval), C, M, _p(counts), _p(sums))
    return lib.dig_map_scores(*args, _p(workspace), workspace_bytes, None) if suffix == "" else lib.dig_map_scores_host(*args, 0)


WINDOW_REFUSALS = [(dict(C=-1), "C, N, M >= 0"), (dict(N=-1), "C, N, M >= 0"), (dict(M=-1), "C, N, M >= 0"), (dict(tail=2), "tail = 0 (upper) or 1"),
                   (dict(tail=-1), "tail = 0 (upper) or 1"), (dict(drop=2), "drop_flagged = 0 or 1"), (dict(drop=1, flag=None), "non-null flag_cm"),
                   (dict(C=1 << 31), "C < 2^31"), (dict(N=1 << 40), "N and M < 2^40"), (dict(M=1 << 40), "N and M < 2^40"),
                   (dict(C=(1 << 31) // 4 + 1, N=1024, M=1024), "C * window groups below 2^31"), (dict(C=256, N=1 << 31, M=1 << 31), "C * window groups"),
                   (dict(run_ptr=None), "non-null run_ptr"), (dict(n_bins=None), "non-null run_ptr"), (dict(y_true=None), "non-null run_ptr"),
                   (dict(y_pred=None), "non-null run_ptr"), (dict(std=None), "non-null run_ptr"), (dict(pval=None), "non-null run_ptr"),
                   (dict(mu=None), "non-null mu_cm"), (dict(sd=None), "non-null mu_cm"), (dict(y=None), "non-null mu_cm")]
SCORE_REFUSALS = [(dict(C=-1), "C, M >= 0"), (dict(M=-1), "C, M >= 0"), (dict(C=1 << 31), "C * chunks below 2^31"),
                  (dict(C=(1 << 31) // 4 + 1, M=4096), "C * chunks below 2^31"), (dict(M=1 << 41), "C * chunks below 2^31"),
                  (dict(counts=None), "non-null counts, sums"), (dict(sums=None), "non-null counts, sums"), (dict(n_bins=None), "non-null n_bins"),
                  (dict(y_true=None), "non-null n_bins"), (dict(y_pred=None), "non-null n_bins"), (dict(pval=None), "non-null n_bins")]


@pytest.mark.parametrize("suffix", ["", "_host"])
def test_every_refusal_comes_before_a_device_is_touched(suffix):
    """(Neither form gets as far as a launch or a staging copy: the pointers are host arrays, and this test runs without a GPU.)"""
    for kw, fragment in WINDOW_REFUSALS:
        assert _windows(suffix, **kw) == -1, kw
        assert fragment in _lib.last_error() and _lib.last_error().startswith(WIN + suffix + ":"), (kw, _lib.last_error())
    for kw, fragment in SCORE_REFUSALS:
        assert _scores(suffix, **kw) == -1, kw
        assert fragment in _lib.last_error() and _lib.last_error().startswith(SCO + suffix + ":"), (kw, _lib.last_error())
    # nothing to do: success on an empty problem, whatever the pointers (flag_cm may be NULL without drop_flagged)
    for kw in (dict(C=0), dict(M=0), dict(C=0, N=0, M=0), dict(C=0, mu=None, sd=None, y=None, flag=None, run_ptr=None, n_bins=None, pval=None)):
        assert _windows(suffix, **kw) == 0, kw
    assert _scores(suffix, C=0) == 0 and _scores(suffix, C=0, M=0, n_bins=None, counts=None, sums=None, workspace=None, workspace_bytes=0) == 0


def test_the_device_form_refuses_its_workspace_and_the_twin_a_bad_run_ptr():
    for kw, fragment in ((dict(workspace=None), "non-null n_bins"), (dict(workspace_bytes=103), "workspace smaller than dig_map_scores_workspace"),
                         (dict(M=1025, workspace_bytes=104), "workspace smaller than")):
        assert _scores("", **kw) == -1 and fragment in _lib.last_error() and _lib.last_error().startswith(SCO + ":"), (kw, _lib.last_error())
    lib = _lib.load()
    odd = np.zeros(100, np.uint8)
    at = odd.ctypes.data + (-odd.ctypes.data % 8) + 4                        # 4 (mod 8)
    assert lib.dig_map_scores(_p("i"), _p("l"), _p("d"), _p("d"), 1, 1, _p("w"), _p("d"), ctypes.c_void_p(at), 104, None) == -1
    assert "workspace 8-byte aligned" in _lib.last_error()
    x, i, l = np.full(8, 0.5), np.zeros(8, np.int32), np.zeros(8, np.int64)
    p = _lib.host_ptr
    for ptr, fragment in (([0, 2, 1, 4], "run_ptr non-decreasing"), ([0, 1, 2, 3], "N last"), ([0, 1, 2, 5], "N last"), ([-1, 1, 2, 4], "non-negative first"),
                          ([0, 5, 3, 4], "run_ptr non-decreasing")):
        r = np.array(ptr, np.int64)
        assert lib.dig_map_windows_host(p(x), p(x), p(i), None, 1, 4, p(r), 3, 0, 0, p(i), p(l), p(x), p(x), p(x), 0) == -1, ptr
        assert _lib.last_error().startswith("dig_map_windows_host: requirement failed: run_ptr") and fragment in _lib.last_error()


def test_engine_raises_value_errors_without_a_device():
    a, i, r = np.full((2, 3), 0.5), np.zeros((2, 3), np.int32), np.array([0, 1, 3], np.int64)
    with pytest.raises(ValueError, match="tail must be 'upper' or 'side'"):
        engine.map_windows(a, a, i, None, r, tail="lower")
    with pytest.raises(ValueError, match="drop_flagged needs flag_cm"):
        engine.map_windows(a, a, i, None, r, drop_flagged=True)
    with pytest.raises(ValueError, match=r"mu_cm must be \[N\] or \[C, N\]"):
        engine.map_windows(a[None], a[None], i[None], None, r)
    with pytest.raises(ValueError, match="run_ptr non-decreasing"):
        engine.map_windows(a, a, i, None, np.array([0, 2, 1, 3]))
    with pytest.raises(ValueError, match=r"n_bins must be \[C, M\]"):
        engine.map_scores(i[0], i[0], a[0], a[0])
    # no window, no cohort: empty results of the right shapes and types, no device needed
    got = engine.map_windows(a, a, i, None, np.zeros(1, np.int64))
    assert {k: (v.shape, v.dtype.str) for k, v in got.items()} == dict(n_bins=((2, 0), "<i4"), y_true=((2, 0), "<i8"), y_pred=((2, 0), "<f8"),
                                                                        std=((2, 0), "<f8"), pval=((2, 0), "<f8"))
    e = np.zeros((0, 5))
    got = engine.map_scores(e, e, e, e)
    assert got["counts"].shape == (0, 7) and got["counts"].dtype == np.int64 and got["sums"].shape == (0, 4)


def _write_map(path, case, c, name=None, rows=None):
    rows = slice(None) if rows is None else rows
    df = pd.DataFrame(dict(CHROM=case["chrom"][rows].astype(np.int64), START=case["start"][rows], END=case["start"][rows] + case["window"],
                           Y_TRUE=case["y"][c][rows].astype(np.int64), Y_PRED=case["mu"][c][rows], STD=case["std"][c][rows],
                           FLAG=case["flag"][c][rows].astype(bool)))
    mapfile.write_frame(path, "region_params", df)
    if name:
        mapfile.write_attrs(path, cohort_name=name)
    return path


def test_route_and_command_refuse_before_a_device_is_touched_or_a_file_written(tmp_path):
    from digdriver_amd.region_model import map_report
    case, _ = MC.shape_case("37x301_s3")
    a, b = _write_map(str(tmp_path / "a.map"), case, 0, name="COHORT_A"), _write_map(str(tmp_path / "b.map"), case, 1)
    short = _write_map(str(tmp_path / "short.map"), case, 2, rows=slice(0, 200))
    out = str(tmp_path / "out")
    for kw, match in ((dict(f_maps=[a, b], labels=["A"]), "labels: one label per map"), (dict(f_maps=[a, b], tail="lower"), "tail: 'upper' or 'side'"),
                      (dict(f_maps=[a, b], outliers_fdr=0.0), r"outliers_fdr: a level within \(0, 1\]"),
                      (dict(f_maps=[a, b], outliers_fdr=1.5), "outliers_fdr: a level within"), (dict(f_maps=[a, b], scales_bp=[]), "scales_bp: one or more"),
                      (dict(f_maps=[a, b], scales_bp=[10000, 25000]), r"scales \[25000\] are not multiples of the maps' window of 10000 bp"),
                      (dict(f_maps=[a, short]), "all cohorts must share one bin grid"), (dict(f_maps=[a, a]), "share the label 'COHORT_A'")):
        with pytest.raises(ValueError, match=match):
            map_report.evaluate_maps(**dict(dict(scales_bp=[10000]), **kw))
    files, tables, names = map_report.load_maps([a, b])
    assert names == ["COHORT_A", None] and map_report.default_labels(files, names) == ["COHORT_A", "b"] and tables.window == MC.W
    assert tables.mu_cm.shape == (2, 301) and tables.y_cm.dtype == np.int32
    cli = _cli()
    args = cli.parse_args("evaluateMaps --maps a.h5 b.h5 --outdir out")
    assert (args.maps, args.outdir, args.labels, args.key, args.scales_bp, args.drop_flagged, args.tail, args.write_windows, args.outliers_fdr) == \
        (["a.h5", "b.h5"], "out", None, "region_params", [10000, 50000, 100000, 1000000], False, "upper", False, None)
    base = "evaluateMaps --maps %s %s --outdir %s " % (a, b, out)
    for extra, match in (("--labels A", "labels: one label per map"), ("--outliers-fdr 0", "outliers_fdr: a level within"),
                         ("--outliers-fdr 1.01", "outliers_fdr: a level within"), ("--scales-bp 10000 15000", "are not multiples of the maps' window"),
                         ("--scales-bp 10000 10000", "scales_bp: one or more different")):
        with pytest.raises(SystemExit, match=match):
            cli.main(base + extra)
    with pytest.raises(SystemExit, match="all cohorts must share one bin grid"):
        cli.main("evaluateMaps --maps %s %s --outdir %s" % (a, short, out))
    assert not os.path.exists(out)


def test_merged_runs_of_the_route_are_the_statements_and_the_fixtures():
    from digdriver_amd.region_model import map_report
    fx = MC.load_fixture()
    for si, s in enumerate(fx["scales"]):
        got = map_report.merged_runs(fx["chrom"], fx["start"], int(s) * MC.W)
        want = S.run_ptr(fx["chrom"], fx["start"], int(s) * MC.W)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        assert np.array_equal(got[0], fx["run_ptr_%d" % si]) and np.array_equal(np.column_stack(got[1:]), fx["coords_%d" % si])
    assert len(fx["run_ptr_4"]) == 4 and fx["scales"].tolist() == [1, 3, 7, 100, 10 ** 6]


@pytest.mark.parametrize("gate", [0, 1])
def test_statement_agrees_with_the_reference_fixture(gate):
    """merge_windows, the reference's p-values, pearsonr and calibration_score_by_pvals against the sequential-sum statement with the
    test-side p-value functions: integers exact, Y_PRED and STD within 1e-12 (at most 233 positive terms, 2^-53 each), p-values, R2,
    EXP_TOTAL, CALIB_SCORE and the fractions within the 1e-6 contract, NaN where the reference has NaN."""
    fx, case = MC.load_fixture(), MC.fixture_case()
    for si, s in enumerate(fx["scales"]):
        key = "%d_%d" % (si, gate)
        for t, tail in enumerate(MC.TAILS):
            want = MC.expected(case, int(s), bool(gate), tail)
            P = want["planes"]
            assert np.array_equal(P["n_bins"], fx["n_bins_" + key]) and np.array_equal(P["y_true"], fx["y_true_" + key])
            clean = ~fx["nan_input_" + key]
            assert np.isnan(P["y_pred"][~clean]).all()
            np.testing.assert_allclose(P["y_pred"][clean], fx["y_pred_" + key][clean], rtol=1e-12, atol=0)
            np.testing.assert_allclose(P["std"], fx["std_" + key], rtol=1e-12, atol=0)
            rel_close(P["pval"], fx["pval_" + key][t])
            assert MC.clear_of_levels(P["pval"]) and np.array_equal(want["counts"], fx["counts_" + key][t])
            for c in range(P["pval"].shape[0]):
                d = S.derived(want["counts"][c], want["sums"][c])
                ref = fx["floats_" + key][t, c]                       # EXP_TOTAL, R2, CALIB_SCORE, FRAC x 4
                if c < 4:
                    np.testing.assert_allclose([want["sums"][c, 0], d["R2"], d["CALIB_SCORE"]] + list(d["FRAC"]), ref, rtol=1e-6, atol=0)
                else:                                                 # the cohort with a NaN Y_PRED: R2 is 0 by the NaN rule
                    assert np.isnan(want["sums"][c, 0]) and d["R2"] == 0.0 == ref[1]
                    np.testing.assert_allclose([d["CALIB_SCORE"]] + list(d["FRAC"]), ref[2:], rtol=1e-6, atol=0)


def test_every_synthetic_shape_is_clear_of_the_levels_and_covers_its_path():
    """The shapes of the GPU test: p-values clear of the four levels (so their counts are exact), and the run lengths the kernel's
    three regimes need (one bin per window; many windows per workgroup; one run far longer than a tile)."""
    longest = {}
    for name, C, bins, s, _ in MC.SHAPES:
        case, s = MC.shape_case(name)
        for tail in MC.TAILS:
            want = MC.expected(case, s, True, tail)
            assert MC.clear_of_levels(want["planes"]["pval"]), (name, tail)
        longest[name] = int(np.diff(want["run_ptr"]).max())
        assert case["mu"].shape == (C, sum(bins))
    assert longest["37x257_s1"] == 1 and longest["3x1003_s100"] > 64 and longest["2x20011_chrom"] == 20011 and longest["1x2_s2"] == 2
