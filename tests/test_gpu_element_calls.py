"""q-values and calls of the many-cohort element route (cohort_batch.run_element_cohorts(qvalues=True), run_element_calls,
`DigDriver.py elementCohorts`) on three cohorts built by the recipe of tests/test_gpu_cohort_batch.py, with four changes that put
every case of the calls on the table: in cohort 0 element i receives i extra SNVs (p-values from the null to the very small, so that
the q-values are graded); in cohort 1's map the bins under one element have STD = 0 (its p-values are NaN: not testable); cohort 2's
file has no indel row (no indel columns) and no SNV inside one element (OBS_SNV = 0).
The full frames with q-values are the yardstick: QVAL_* = get_q_vals of the column's NaN-dropped p-values put back, bit for bit, and
the frames of run_element_calls equal the filtered full frames exactly (columns, dtypes, order, bits)."""
import importlib.util
import os

import numpy as np
import pandas as pd
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

PVALS = ["PVAL_SNV_BURDEN", "PVAL_SAMPLE_BURDEN", "PVAL_INDEL_BURDEN", "PVAL_MUT_BURDEN"]
NAN_ELT = 4                                                      # the element whose bins have STD = 0 in cohort 1
ZERO_ELT = 9                                                     # the element without an SNV in cohort 2


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return _build_case(tmp_path_factory.mktemp("element_calls"))


def _build_case(tmp_path):
    from test_gpu_onthefly import _make_case
    from digdriver_amd import _lib
    from digdriver_amd.driver_model import cohort_batch
    from digdriver_amd.io import mapfile
    from digdriver_amd.sequence_model import sequence_tools
    _lib.require_device()
    rng = np.random.default_rng(31)
    base = _make_case(tmp_path, rng)
    window, C = base["window"], 3
    pres, muts = [], []
    for c in range(C):
        rp = base["rp"].copy()
        rp["Y_PRED"] = rng.gamma(9.0, 3.0, len(rp))
        rp["STD"] = rng.gamma(4.0, 1.0, len(rp))
        rp["Y_TRUE"] = rng.poisson(rp.Y_PRED.values)
        rp["FLAG"] = rng.uniform(size=len(rp)) < 0.2
        if c == 1:                                                # no spread under one element: its p-values are NaN
            _, ch, _, blocks = base["elts"][NAN_ELT]
            for s, e in blocks:
                under = (rp.CHROM.values == int(ch)) & (rp.END.values > s) & (rp.START.values < e)
                assert under.any()
                rp.loc[under, "STD"] = 0.0
        sm = base["sm"].copy()
        sm["FREQ"] = rng.dirichlet(np.ones(192)) * 1e-3
        pre = str(tmp_path / ("cohort%d.map" % c))
        mapfile.write_frame(pre, "region_params", rp)
        mapfile.write_frame(pre, "sequence_model_192", sm)
        mapfile.write_array(pre, "idx", rp[["CHROM", "START", "END"]].values.astype(np.int32))
        mapfile.write_attrs(pre, cohort_name="c%d" % c, mappability_threshold=0.5)
        rows = []
        for i, (name, ch, strand, blocks) in enumerate(base["elts"]):
            for k in range(int(rng.poisson(3 + c)) + (i if c == 0 else 0)):
                s, e = blocks[int(rng.integers(0, len(blocks)))]
                p = int(rng.integers(s, e))
                rows.append((ch, p, p + 1, "A", "T", "S%d" % rng.integers(0, 9), ".", "Noncoding", "A>T", "CAG"))
            if rng.uniform() < 0.5 and c != 2:
                p = blocks[0][0]
                rows.append((ch, p, p + 2, "AG", "A", "S%d" % rng.integers(0, 9), ".", "INDEL", "DEL", "."))
        for _ in range(60):                                       # background mutations outside the elements
            ch = "12"[int(rng.integers(0, 2))]
            p = int(rng.integers(0, 20000))
            rows.append((ch, p, p + 1, "C", "G", "S%d" % rng.integers(0, 9), ".", "Noncoding", "C>G", "ACA"))
        if c == 2:                                                # no SNV inside one element: OBS_SNV = 0 there
            _, ch0, _, blocks0 = base["elts"][ZERO_ELT]
            rows = [r for r in rows if not (r[0] == ch0 and any(s <= r[1] < e for s, e in blocks0))]
        rows += rows[:5]                                          # exact duplicates
        blk = base["elts"][c][3][0]                             # the same indel in several samples, as the recipe has it
        for smp, gene in (("S1", "."), ("S2", "."), ("S3", "."), ("S4", "G2"), ("S5", "G2")) if c != 2 else ():
            rows.append((base["elts"][c][1], blk[0] + 3, blk[0] + 6, "ACG", "A", smp, gene, "INDEL", "DEL", "."))
            rows.append(("1", 15000 + c, 15003 + c, "TTA", "T", smp, gene, "INDEL", "DEL", "."))
        f = tmp_path / ("muts%d.tsv" % c)
        pd.DataFrame(rows).to_csv(f, sep="\t", header=False, index=False)
        pres.append(pre)
        muts.append(str(f))
    gc, ed = str(tmp_path / "gc.map"), str(tmp_path / "ed.map")
    win = sequence_tools.count_contexts_in_bed(base["fa"], base["rp"][["CHROM", "START", "END"]], n_up=1, n_down=1)
    mapfile.write_frame(gc, "all_window_genome_counts", win)
    mapfile.write_array(gc, "idx", base["rp"][["CHROM", "START", "END"]].values.astype(np.int32))
    sequence_tools.initialize_nonc_data(ed, gc, window)
    L = sequence_tools.precount_region_contexts_parallel(base["bed"], base["fa"], 1, window, True)
    sequence_tools.preprocess_nonc(base["bed"], ed, pres[0], L, "elts", window)
    full = cohort_batch.run_element_cohorts(muts, pres, ed, "elts", qvalues=True)
    return dict(muts=muts, pres=pres, ed=ed, full=full, tmp=tmp_path, nan_name=base["elts"][NAN_ELT][0], zero_name=base["elts"][ZERO_ELT][0])


def _exact(a, b):
    pd.testing.assert_frame_equal(a, b, check_exact=True)
    for col in a.columns:
        assert a[col].values.tobytes() == b[col].values.tobytes(), col


def test_the_case_has_what_the_calls_must_handle(case):
    full = case["full"]
    row = full[1].loc[case["nan_name"]]
    assert np.isnan(row.PVAL_SNV_BURDEN) and np.isnan(row.PVAL_SAMPLE_BURDEN) and np.isnan(row.QVAL_SNV_BURDEN)
    assert "PVAL_MUT_BURDEN" in full[0].columns and "PVAL_MUT_BURDEN" in full[1].columns and "PVAL_MUT_BURDEN" not in full[2].columns
    assert full[2].OBS_SNV.loc[case["zero_name"]] == 0 and any((f.OBS_SNV.values > 0).any() for f in full)


def test_frames_without_q_values_are_the_frames_of_before_and_a_prefix_of_those_with(case):
    from digdriver_amd.driver_model import cohort_batch
    plain = cohort_batch.run_element_cohorts(case["muts"], case["pres"], case["ed"], "elts")
    off = cohort_batch.run_element_cohorts(case["muts"], case["pres"], case["ed"], "elts", qvalues=False)
    for c, (a, b, f) in enumerate(zip(plain, off, case["full"])):
        _exact(a, b)
        n_q = 4 if "PVAL_MUT_BURDEN" in a.columns else 2
        assert list(f.columns) == list(a.columns) + ["QVAL_" + k[5:] for k in PVALS[:n_q]]
        _exact(f[list(a.columns)], a)


def test_q_value_columns_are_get_q_vals_of_the_testable_p_values_put_back(case):
    from digdriver_amd.sequence_model import nb_model
    seen_nan = 0
    for f in case["full"]:
        for k in [k for k in PVALS if k in f.columns]:
            p = f[k]
            want = pd.Series(np.nan, index=f.index)
            want[p.notna()] = nb_model.get_q_vals(p.dropna().values)
            got = f["QVAL_" + k[5:]]
            assert got.dtype == np.float64 and got.values.tobytes() == want.values.tobytes(), k
            seen_nan += int(p.isna().sum())
    assert seen_nan > 0


@pytest.mark.parametrize("form", ["records", "planes"])
def test_calls_at_an_fdr_equal_the_filtered_full_frames(case, form):
    from digdriver_amd.driver_model import cohort_batch
    full = case["full"]
    q0 = full[0].QVAL_SNV_BURDEN.dropna().values
    fdr = float(np.median(q0))                                   # a level equal to a q-value (or between two): the inclusive edge
    assert len(np.unique(q0)) >= 2
    hits = cohort_batch.run_element_calls(case["muts"], case["pres"], case["ed"], "elts", fdr=fdr, output_form=form)
    partial = 0
    for f, h in zip(full, hits):
        want = f[f.QVAL_SNV_BURDEN <= fdr]
        print("fdr", fdr, "hits", len(h), "want", len(want), "testable", h.attrs["n_testable"])
        _exact(h, want)
        assert h.attrs["n_testable"] == int(f.PVAL_SNV_BURDEN.notna().sum())
        partial += 0 < len(h) < h.attrs["n_testable"]
    assert partial >= 1
    assert case["nan_name"] not in hits[1].index


@pytest.mark.parametrize("cut_on", PVALS[:2])
def test_calls_at_a_p_value_equal_the_filtered_full_frames(case, cut_on):
    from digdriver_amd.driver_model import cohort_batch
    full = case["full"]
    pval_max = float(np.median(full[0][cut_on].dropna().values))
    hits = cohort_batch.run_element_calls(case["muts"], case["pres"], case["ed"], "elts", pval_max=pval_max, cut_on=cut_on)
    for f, h in zip(full, hits):
        _exact(h, f[f[cut_on] <= pval_max])
        assert h.attrs["n_testable"] == int(f[cut_on].notna().sum())
    assert 0 < len(hits[0]) < len(full[0])
    none = cohort_batch.run_element_calls(case["muts"], case["pres"], case["ed"], "elts", pval_max=1e-300, cut_on=cut_on)
    for f, h in zip(full, none):
        _exact(h, f[f[cut_on] <= 1e-300])


def test_an_indel_column_cuts_where_every_cohort_has_it_and_is_refused_where_one_lacks_it(case):
    from digdriver_amd.driver_model import cohort_batch
    with pytest.raises(ValueError, match=r"PVAL_INDEL_BURDEN: cohorts \[2\] have no indel columns"):
        cohort_batch.run_element_calls(case["muts"], case["pres"], case["ed"], "elts", fdr=0.5, cut_on="PVAL_INDEL_BURDEN")
    two = (case["muts"][:2], case["pres"][:2], case["ed"], "elts")
    full = cohort_batch.run_element_cohorts(*two, qvalues=True)
    for a, b in zip(full, case["full"]):                          # (a cohort's frame does not depend on its neighbours)
        _exact(a, b)
    fdr = float(np.median(full[0].QVAL_MUT_BURDEN.dropna().values))
    for h, f in zip(cohort_batch.run_element_calls(*two, fdr=fdr, cut_on="PVAL_MUT_BURDEN"), full):
        _exact(h, f[f.QVAL_MUT_BURDEN <= fdr])
        assert h.attrs["n_testable"] == int(f.PVAL_MUT_BURDEN.notna().sum())


def test_the_command_line_writes_hit_files_that_read_back_to_the_frames(case):
    spec = importlib.util.spec_from_file_location("dig_driver_cli_element_calls", os.path.join(ROOT, "scripts", "DigDriver.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    full = case["full"]
    fdr = float(np.median(full[0].QVAL_SNV_BURDEN.dropna().values))
    outdir = str(case["tmp"] / "cli_out")
    lists = "--mutation-files %s --maps %s --outpfx A B C --outdir %s" % (" ".join(case["muts"]), " ".join(case["pres"]), outdir)
    cli.main("elementCohorts %s elts %s --fdr %r" % (case["ed"], lists, fdr))
    for pfx, f in zip("ABC", full):
        want = f[f.QVAL_SNV_BURDEN <= fdr]
        back = pd.read_csv(os.path.join(outdir, pfx + ".hits.txt"), sep="\t", index_col=0, float_precision="round_trip")
        assert list(back.columns) == list(want.columns) and list(back.index) == list(want.index) and back.index.name == "ELT"
        for col in want.columns:
            assert np.array_equal(back[col].values.astype(float), want[col].values.astype(float), equal_nan=True), (pfx, col)
        assert not os.path.exists(os.path.join(outdir, pfx + ".results.txt"))
    with pytest.raises(SystemExit, match="no indel columns"):
        cli.main("elementCohorts %s elts %s --pval-max 0.5 --cut-on PVAL_MUT_BURDEN" % (case["ed"], lists))
    # without a cut: the results files, with the q-value columns on request
    cli.main("elementCohorts %s elts %s --qvalues" % (case["ed"], lists))
    for pfx, f in zip("ABC", full):
        back = pd.read_csv(os.path.join(outdir, pfx + ".results.txt"), sep="\t", index_col=0, float_precision="round_trip")
        assert list(back.columns) == list(f.columns) and list(back.index) == list(f.index)
        for col in f.columns:
            assert np.array_equal(back[col].values.astype(float), f[col].values.astype(float), equal_nan=True), (pfx, col)
