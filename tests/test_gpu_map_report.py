"""The map report on the GPU: engine.map_windows / engine.map_scores (the device form on CUDA tensors, the `_host` twins on numpy
arrays) against the numpy statement -- integers exact, Y_PRED and STD bit for bit -- and against the fixture made with the reference's
own functions (tests/golden/make_map_report_golden.py); the same bits from two runs, the twin and a side stream; the route's
outlier frames against nb_model.get_q_vals; `DigPretrain.py evaluateMaps` end to end."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import map_report_cases as MC
import map_report_statement as S
from conftest import ROOT, rel_close
from guarded_arena import side_stream_call
from map_report_cases import same_bits
from test_map_report_host import _write_map

pytestmark = pytest.mark.gpu

PLANES = ("n_bins", "y_true", "y_pred", "std", "pval")


@pytest.fixture(scope="module")
def dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    return torch.device("cuda:0")


def _run(case, ptr, drop, tail, dev=None):
    """engine.map_windows + engine.map_scores on host arrays (dev None: the twins) or on their device copies: numpy results."""
    import torch
    from digdriver_amd import engine
    on = (lambda x: x) if dev is None else (lambda x: torch.as_tensor(x, device=dev))
    w = engine.map_windows(on(case["mu"]), on(case["std"]), on(case["y"]), on(case["flag"]) if drop else None, on(ptr), drop_flagged=drop,
                           tail=tail)
    sc = engine.map_scores(w["n_bins"], w["y_true"], w["y_pred"], w["pval"])
    if dev is not None:
        assert all(v.is_cuda for v in w.values()) and w["n_bins"].dtype == torch.int32 and w["y_true"].dtype == torch.int64
        w, sc = {k: v.cpu().numpy() for k, v in w.items()}, {k: v.cpu().numpy() for k, v in sc.items()}
    return dict(w, **sc)


def _check_against_statement(got, want, what):
    """Integers exact, the two float sums bit for bit, p-values within the contract with NaN where the statement has NaN, the counts
    exact, the score sums the statement's bits."""
    P = want["planes"]
    for k in ("n_bins", "y_true"):
        assert got[k].dtype == P[k].dtype and np.array_equal(got[k], P[k]), (what, k)
    for k in ("y_pred", "std"):
        assert same_bits(got[k], P[k]), (what, k, float(np.nanmax(np.abs(got[k] - P[k]))))
    rel_close(got["pval"], P["pval"])
    assert np.array_equal(got["counts"], want["counts"]), (what, got["counts"], want["counts"])
    # the score sums on the DEVICE's own planes (its p-values may differ from the statement's in the last bits; the sums do not read them)
    assert same_bits(got["sums"], want["sums"]), (what, got["sums"], want["sums"])


@pytest.fixture(scope="module")
def statement_of_shapes():
    """The statement, once per (shape, gate, tail) that the tests below use."""
    out = {}
    for name, *_ in MC.SHAPES:
        case, s = MC.shape_case(name)
        for drop, tail in ((False, "upper"), (True, "side")):
            out[name, drop, tail] = (case, MC.expected(case, s, drop, tail))
    return out


@pytest.mark.parametrize("drop,tail", [(False, "upper"), (True, "side")], ids=["all_upper", "unflagged_side"])
@pytest.mark.parametrize("name", [t[0] for t in MC.SHAPES])
def test_shapes_against_the_statement_device_and_twin(name, drop, tail, dev, statement_of_shapes):
    case, want = statement_of_shapes[name, drop, tail]
    got = _run(case, want["run_ptr"], drop, tail, dev)
    _check_against_statement(got, want, name)
    twin = _run(case, want["run_ptr"], drop, tail, None)
    again = _run(case, want["run_ptr"], drop, tail, dev)
    for k in PLANES + ("counts", "sums"):
        assert same_bits(got[k], twin[k]) and same_bits(got[k], again[k]), (name, k)


@pytest.mark.parametrize("gate", [0, 1])
@pytest.mark.parametrize("tail", MC.TAILS)
def test_fixture_of_the_reference(gate, tail, dev):
    """Every scale of the fixture: integers and the score counts exact; Y_PRED and STD within 1e-12 of merge_windows (at most 233
    positive terms of 2^-53 each: 2.6e-14), bit-equal to the statement; p-values within 1e-6 (the log rule below 1e-250), NaN where the
    reference has NaN; R2, EXP_TOTAL, CALIB_SCORE and the fractions within 1e-6."""
    fx, case, t = MC.load_fixture(), MC.fixture_case(), MC.TAILS.index(tail)
    for si, s in enumerate(fx["scales"]):
        key = "%d_%d" % (si, gate)
        ptr = fx["run_ptr_%d" % si]
        got = _run(case, ptr, bool(gate), tail, dev)
        assert np.array_equal(got["n_bins"], fx["n_bins_" + key]) and np.array_equal(got["y_true"], fx["y_true_" + key])
        clean = ~fx["nan_input_" + key]
        assert np.isnan(got["y_pred"][~clean]).all()
        np.testing.assert_allclose(got["y_pred"][clean], fx["y_pred_" + key][clean], rtol=1e-12, atol=0)
        np.testing.assert_allclose(got["std"], fx["std_" + key], rtol=1e-12, atol=0)
        rel_close(got["pval"], fx["pval_" + key][t])
        assert np.array_equal(got["counts"], fx["counts_" + key][t])
        for c in range(5):
            w = S.merge(case["mu"][c], case["std"][c], case["y"][c], case["flag"][c], ptr, bool(gate))
            assert same_bits(got["y_pred"][c], w["y_pred"]) and same_bits(got["std"][c], w["std"]), (key, c)
            d, ref = S.derived(got["counts"][c], got["sums"][c]), fx["floats_" + key][t, c]
            if c < 4:
                np.testing.assert_allclose([got["sums"][c, 0], d["R2"], d["CALIB_SCORE"]] + list(d["FRAC"]), ref, rtol=1e-6, atol=0)
            else:
                assert np.isnan(got["sums"][c, 0]) and d["R2"] == 0.0 == ref[1]
                np.testing.assert_allclose([d["CALIB_SCORE"]] + list(d["FRAC"]), ref[2:], rtol=1e-6, atol=0)


def test_a_side_stream_gives_the_same_bits(dev):
    import torch
    from digdriver_amd import engine
    case, s = MC.shape_case("3x1003_s100")
    ptr = S.run_ptr(case["chrom"], case["start"], s * MC.W)[0]
    on = lambda x: torch.as_tensor(x, device=dev)
    args = [on(case[k]) for k in ("mu", "std", "y", "flag")] + [on(ptr)]

    def fn(stream):
        w = engine.map_windows(*args, drop_flagged=True, tail="upper")
        return dict(w, **engine.map_scores(w["n_bins"], w["y_true"], w["y_pred"], w["pval"]))
    plain = side_stream_call(fn, dev, "engine.map_windows + engine.map_scores")
    want = MC.expected(case, s, True, "upper")
    assert same_bits(plain["y_pred"], want["planes"]["y_pred"]) and same_bits(plain["sums"], want["sums"])


def _fixture_maps(tmp_path):
    case = MC.fixture_case()
    return case, [_write_map(str(tmp_path / ("m%d.map" % c)), case, c, name="COHORT_%d" % c if c < 3 else None) for c in range(5)]


def test_route_report_and_outliers(tmp_path, dev):
    """evaluate_maps on maps written by mapfile.write_frame: the report's rows from the fixture; the outlier frames are the windows with
    get_q_vals(testable p) <= fdr, in grid order, with those q-values."""
    from digdriver_amd.region_model import map_report
    from digdriver_amd.sequence_model import nb_model
    fx = MC.load_fixture()
    case, maps = _fixture_maps(tmp_path)
    fdr = 0.2
    res = map_report.evaluate_maps(maps, [10000, 30000, 1000000], drop_flagged=True, outliers_fdr=fdr)
    assert res["labels"] == ["COHORT_0", "COHORT_1", "COHORT_2", "m3", "m4"] and res["scales_bp"] == [10000, 30000, 1000000]
    rep = res["report"]
    assert list(rep.columns) == map_report.REPORT_COLUMNS and rep.index.name == "COHORT" and len(rep) == 15
    n_hits = 0
    for bp, si in ((10000, 0), (30000, 1), (1000000, 3)):
        key = "%d_1" % si
        rows = rep[rep.SCALE_BP == bp]
        assert list(rows.index) == res["labels"]
        assert np.array_equal(rows[["N_WINDOWS", "N_TESTED", "OBS_TOTAL"]].values, fx["counts_" + key][0][:, :3])
        ref = fx["floats_" + key][0]
        np.testing.assert_allclose(rows[["EXP_TOTAL", "R2", "CALIB_SCORE", "FRAC_0.05", "FRAC_0.01", "FRAC_0.001", "FRAC_0.0001"]].values[:4],
                                   ref[:4], rtol=1e-6, atol=0)
        assert rows.R2.values[4] == 0.0
        W = res["windows"][bp]
        assert np.array_equal(W["run_ptr"], fx["run_ptr_%d" % si]) and np.array_equal(np.column_stack([W["CHROM"], W["START"], W["END"]]),
                                                                                       fx["coords_%d" % si])
        planes = {k: v.cpu().numpy() for k, v in W["planes"].items()}
        for c, frame in enumerate(res["outliers"][bp]):
            p = planes["pval"][c]
            ok = np.flatnonzero(~np.isnan(p))
            q = nb_model.get_q_vals(p[ok])
            hit = ok[q <= fdr]
            assert list(frame.columns) == map_report.WINDOW_COLUMNS + ["QVAL"] and frame.index.name == "CHROM"
            assert np.array_equal(frame.index.values, W["CHROM"][hit]) and np.array_equal(frame.START.values, W["START"][hit])
            assert same_bits(frame.QVAL.values, q[q <= fdr]) and same_bits(frame.PVAL.values, p[hit])
            assert np.array_equal(frame.Y_TRUE.values, planes["y_true"][c][hit]) and same_bits(frame.STD.values, planes["std"][c][hit])
            n_hits += len(hit)
    assert n_hits > 12                                                       # (the planted hot windows of cohort 2, and more)


_DRIVER = """
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {scripts!r})
import DigPretrain
DigPretrain.main({text!r})
"""


def test_command_end_to_end(tmp_path, dev):
    """The files of `DigPretrain.py evaluateMaps` against the route's own frames; another sub-command of the same script still parses
    and refuses as before."""
    from digdriver_amd.region_model import map_report
    case, maps = _fixture_maps(tmp_path)
    out = str(tmp_path / "out")
    text = "evaluateMaps --maps %s --outdir %s --scales-bp 10000 70000 --tail side --write-windows --outliers-fdr 0.1 --labels A B C D E" % (
        " ".join(maps), out)
    script = _DRIVER.format(root=ROOT, scripts=os.path.join(ROOT, "scripts"), text=text)
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    res = map_report.evaluate_maps(maps, [10000, 70000], labels=list("ABCDE"), tail="side", outliers_fdr=0.1)
    assert sorted(os.listdir(out)) == sorted(["map_report.txt"] + ["%s.%s_%d.txt" % (l, k, bp) for l in "ABCDE" for k in ("windows", "outliers")
                                                                   for bp in (10000, 70000)])
    got = pd.read_csv(os.path.join(out, "map_report.txt"), sep="\t", index_col=0, float_precision="round_trip")
    assert open(os.path.join(out, "map_report.txt")).readline().rstrip("\n").split("\t") == ["COHORT"] + map_report.REPORT_COLUMNS
    pd.testing.assert_frame_equal(got, res["report"], check_exact=True)
    planes = {k: v.cpu().numpy() for k, v in res["windows"][70000]["planes"].items()}
    win = pd.read_csv(os.path.join(out, "C.windows_70000.txt"), sep="\t", index_col=0, float_precision="round_trip")
    assert open(os.path.join(out, "C.windows_70000.txt")).readline().rstrip("\n").split("\t") == ["CHROM"] + map_report.WINDOW_COLUMNS
    assert np.array_equal(win.N_BINS.values, planes["n_bins"][2]) and same_bits(win.Y_PRED.values, planes["y_pred"][2])
    assert same_bits(win.PVAL.values, planes["pval"][2])
    hot = pd.read_csv(os.path.join(out, "C.outliers_10000.txt"), sep="\t", index_col=0, float_precision="round_trip")
    pd.testing.assert_frame_equal(hot, res["outliers"][10000][2], check_exact=True)
    assert len(hot) >= 12 and list(hot.columns) == map_report.WINDOW_COLUMNS + ["QVAL"]
    from test_sequence_models_host import _cli
    cli = _cli()
    a = cli.parse_args("sequenceModels gc.h5 --mutation-files a.txt b.txt --maps a.h5 b.h5")
    assert (a.genome_counts, a.fmuts, a.maps, a.map_thresh, a.up, a.down) == ("gc.h5", ["a.txt", "b.txt"], ["a.h5", "b.h5"], 0.5, 1, 1)
    with pytest.raises(SystemExit, match="one map per mutation file"):
        cli.main("countMutationsCohorts --mutation-files a.txt b.txt --maps a.h5")
