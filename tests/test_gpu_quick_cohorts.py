"""quickDriver for many cohorts (driver_model/cohort_batch.py run_quick_cohorts) against the single route
(onthefly_tools.DIG_onthefly, one cohort at a time) on C = 3 maps of one small grid (tests/quick_cohort_cases.py): the same
columns in the same order with the same dtypes, the same index, integer and boolean columns equal, float columns within the relative
1e-9 of tests/test_gpu_cohort_batch.py (the same pipeline against the per-cohort route) -- for expectation scaling, given factors
and genome scaling; skip_pvals, a region string, strict_reference=False and the command line."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import quick_cohort_cases as K
from conftest import ROOT, rel_close

pytestmark = pytest.mark.gpu

FACTORS = (np.array([0.004, 0.002, 0.008]), np.array([0.0007, 0.0003, 0.001]))
MODES = {
    "expectation": (dict(scale_by_expectation=True, all_cosmic=K.ALL_COSMIC), lambda c: dict(scale_by_expectation=True, all_cosmic=K.ALL_COSMIC)),
    "factors": (dict(scale_factors=FACTORS, scale_by_expectation=False),
                lambda c: dict(scale_factor=FACTORS[0][c], scale_factor_indel=FACTORS[1][c], scale_by_expectation=False)),
    "genome": (dict(scale_type="genome", scale_by_expectation=False), lambda c: dict(scale_type="genome", scale_by_expectation=False)),
}


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    from digdriver_amd import _lib
    _lib.require_device()
    return K.make_case(tmp_path_factory.mktemp("quick"))


def same_frame(got, want, what):
    assert list(got.columns) == list(want.columns), what
    assert {c: str(got[c].dtype) for c in got.columns} == {c: str(want[c].dtype) for c in want.columns}, what
    assert got.index.name == want.index.name and list(got.index) == list(want.index) and got.index.dtype == want.index.dtype, what
    for col in want.columns:
        g, w = got[col].values, want[col].values
        if w.dtype.kind in "iub" or col.startswith("OBS_"):
            assert np.array_equal(g, w), (what, col)
        else:
            try:
                rel_close(g, w, rtol=1e-9)
            except AssertionError as exc:
                raise AssertionError("%s, column %s: %s" % (what, col, exc)) from exc


@pytest.mark.parametrize("mode", list(MODES))
def test_frames_equal_the_single_route(case, mode):
    from digdriver_amd.driver_model import cohort_batch, onthefly_tools
    batch_kw, single_kw = MODES[mode]
    seen = []
    frames = cohort_batch.run_quick_cohorts(case["muts"], case["maps"], case["fa"], f_elts_bed=case["bed"],
                                            max_muts_per_sample=K.HYPER_LIMIT, on_frame=lambda c, f: seen.append(c), **batch_kw)
    assert seen == [0, 1, 2] and len(frames) == 3
    for c in range(3):
        want = onthefly_tools.DIG_onthefly(case["maps"][c], case["muts"][c], case["fa"], f_elts_bed=case["bed"],
                                           max_muts_per_sample=K.HYPER_LIMIT, **single_kw(c))
        same_frame(frames[c], want, "%s, cohort %d" % (mode, c))
        assert "PVAL_MUT_BURDEN" in want.columns and len(want) == len(case["elts"])
    # what the case is there for: indels in cohorts 0 and 1 only, every window edge element counted, the blacklisted sample
    assert frames[0].OBS_INDEL.sum() > 0 and frames[1].OBS_INDEL.sum() > 0 and frames[2].OBS_INDEL.sum() == 0
    assert (frames[1].OBS_SNV.values > 0).any()
    if mode == "factors":
        loose = cohort_batch.run_quick_cohorts(case["muts"], case["maps"], case["fa"], f_elts_bed=case["bed"], **batch_kw)
        assert loose[1].OBS_SNV.sum() >= frames[1].OBS_SNV.sum() + 80      # the hypermutated sample's 90 rows are in without the limit
        assert loose[0].OBS_SNV.sum() == frames[0].OBS_SNV.sum() and loose[2].OBS_SNV.sum() == frames[2].OBS_SNV.sum()


def test_skip_pvals_and_region_string(case):
    from digdriver_amd.driver_model import cohort_batch, onthefly_tools
    batch_kw, single_kw = MODES["factors"]
    frames = cohort_batch.run_quick_cohorts(case["muts"], case["maps"], case["fa"], f_elts_bed=case["bed"], skip_pvals=True, **batch_kw)
    for c in range(3):
        want = onthefly_tools.DIG_onthefly(case["maps"][c], case["muts"][c], case["fa"], f_elts_bed=case["bed"], skip_pvals=True, **single_kw(c))
        same_frame(frames[c], want, "skip_pvals, cohort %d" % c)
        assert "PVAL_SNV_BURDEN" not in want.columns and "EXP_SNV" in want.columns
    region = "chr1:2500-7300"                                             # across five windows, not on their edges
    frames = cohort_batch.run_quick_cohorts(case["muts"], case["maps"], case["fa"], region_str=region, **batch_kw)
    for c in range(3):
        want = onthefly_tools.DIG_onthefly(case["maps"][c], case["muts"][c], case["fa"], region_str=region, **single_kw(c))
        same_frame(frames[c], want, "region string, cohort %d" % c)
        assert list(want.index) == ["UserELT"] and int(want.ELT_SIZE.iloc[0]) > 4000


def test_not_strict_changes_only_the_indel_columns(case):
    from digdriver_amd.driver_model import cohort_batch, onthefly_tools
    batch_kw, single_kw = MODES["factors"]
    strict = cohort_batch.run_quick_cohorts(case["muts"], case["maps"], case["fa"], f_elts_bed=case["bed"], **batch_kw)
    loose = cohort_batch.run_quick_cohorts(case["muts"], case["maps"], case["fa"], f_elts_bed=case["bed"], strict_reference=False, **batch_kw)
    indel = {"THETA_INDEL", "EXP_INDEL", "PVAL_INDEL_BURDEN", "PVAL_MUT_BURDEN"}
    for c in range(3):
        assert list(strict[c].columns) == list(loose[c].columns)
        for col in strict[c].columns:
            same = np.array_equal(strict[c][col].values, loose[c][col].values, equal_nan=strict[c][col].dtype.kind == "f")
            assert same == (col not in indel), (c, col)
        want = onthefly_tools.DIG_onthefly(case["maps"][c], case["muts"][c], case["fa"], f_elts_bed=case["bed"], strict_reference=False,
                                           **single_kw(c))
        same_frame(loose[c], want, "strict_reference=False, cohort %d" % c)


def test_opposite_strand_pair_is_counted_per_strand_when_not_strict(case, tmp_path):
    """The bed of the strict refusal (tests/test_quick_cohorts_host.py) under strict_reference=False: every element's L is that of its
    own strand -- ELT_SIZE of the pair is equal, and Pi_SUM is the single route's of each element alone."""
    from digdriver_amd.driver_model import cohort_batch, onthefly_tools
    batch_kw, single_kw = MODES["factors"]
    lines = [K.bed12_line("1", 5000, "fwd", "+", [(0, 400), (900, 300)]), K.bed12_line("1", 5000, "rev", "-", [(0, 400)])]
    bed = tmp_path / "pair.bed"
    bed.write_text("".join(lines))
    with pytest.raises(ValueError, match="fwd and rev"):
        cohort_batch.run_quick_cohorts(case["muts"], case["maps"], case["fa"], f_elts_bed=str(bed), **batch_kw)
    frames = cohort_batch.run_quick_cohorts(case["muts"], case["maps"], case["fa"], f_elts_bed=str(bed), strict_reference=False, **batch_kw)
    for name, line in zip(("fwd", "rev"), lines):
        alone = tmp_path / (name + ".bed")
        alone.write_text(line)
        want = onthefly_tools.DIG_onthefly(case["maps"][0], case["muts"][0], case["fa"], f_elts_bed=str(alone), strict_reference=False,
                                           **single_kw(0))
        for col in ("ELT_SIZE", "R_SIZE", "OBS_SNV"):
            assert frames[0].loc[name, col] == want.loc[name, col], (name, col)
        rel_close(np.array([frames[0].loc[name, "Pi_SUM"]]), np.array([want.loc[name, "Pi_SUM"]]), rtol=1e-9)


def test_command_line_writes_the_frames(case, tmp_path):
    from digdriver_amd.driver_model import cohort_batch
    batch_kw, _ = MODES["factors"]
    frames = cohort_batch.run_quick_cohorts(case["muts"], case["maps"], case["fa"], f_elts_bed=case["bed"],
                                            max_muts_per_sample=K.HYPER_LIMIT, **batch_kw)
    out = tmp_path / "out"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "DigDriver.py"), "quickCohorts", case["fa"], "--mutation-files",
                           *case["muts"], "--maps", *case["maps"], "--outdir", str(out), "--outpfx", "a", "b", "c", "--f_elts_bed", case["bed"],
                           "--max-muts-per-sample", str(K.HYPER_LIMIT), "--scale-factor-manual", *[repr(float(x)) for x in FACTORS[0]],
                           "--scale-factor-indel-manual", *[repr(float(x)) for x in FACTORS[1]]], env=dict(os.environ, PYTHONPATH=ROOT))
    assert sorted(os.listdir(out)) == ["a.results.txt", "b.results.txt", "c.results.txt"]
    for pfx, frame in zip("abc", frames):
        res = pd.read_csv(out / (pfx + ".results.txt"), sep="\t", index_col=0, float_precision="round_trip")
        assert list(res.columns) == list(frame.columns) and list(res.index) == list(frame.index) and res.index.name == "ELT"
        for col in ("OBS_SAMPLES", "OBS_SNV", "OBS_INDEL"):
            assert res[col].dtype.kind == "i"
        for col in frame.columns:
            np.testing.assert_array_equal(res[col].values.astype(float), frame[col].values.astype(float), err_msg=col)
