"""Meta-cohort frames of the element route (cohort_batch.run_element_meta, run_element_meta_calls, `DigDriver.py elementCohorts
--groups`) on the three cohorts of tests/test_gpu_element_calls.py -- cohort C has no indel row (no indel columns), one element is NaN
(not testable) in cohort B, one has no SNV in cohort C.  The yardstick is a numpy / pandas recombination of the three
run_element_cohorts(qvalues=True) frames: everything bit for bit, except the combined p-values of three members, which lie within M_G
(tests/test_group_fisher_fixture.py) of their 80-digit values; the q-values are then get_q_vals of the frame's own p-values."""
import importlib.util
import os

import numpy as np
import pandas as pd
import pytest

from conftest import ROOT
from test_group_fisher_fixture import M_G, load_maker
from test_gpu_element_calls import PVALS, _build_case

pytestmark = pytest.mark.gpu

LABELS = ["A", "B", "C"]
GROUPS = {"pan": ["A", "B", "C"], "ab": ["B", "A"], "onlyC": ["C"], "onlyB": [1], "bc": ["B", "C"]}
N_TESTED = ["N_TESTED_" + k[5:] for k in PVALS]
QVALS = ["QVAL_" + k[5:] for k in PVALS]


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    from digdriver_amd.driver_model import cohort_batch
    c = _build_case(tmp_path_factory.mktemp("element_meta"))
    c["meta"] = cohort_batch.run_element_meta(c["muts"], c["pres"], c["ed"], "elts", GROUPS, labels=LABELS)
    return c


def _exact(a, b):
    """Two frames with the same columns, dtypes, index and bits (a column of labels: the same strings)."""
    pd.testing.assert_frame_equal(a, b, check_exact=True)
    for col in a.columns:
        if a[col].dtype == object:
            assert list(a[col]) == list(b[col]), col
        else:
            assert a[col].values.tobytes() == b[col].values.tobytes(), col


def _members(name):
    return sorted(LABELS.index(v) if isinstance(v, str) else v for v in GROUPS[name])


def _column(full, c, k):
    """Column k of cohort c's frame, NaN where the cohort lacks it (it did not test it)."""
    return full[c][k].values if k in full[c].columns else np.full(len(full[c]), np.nan)


def recombine(full, idx, best_on="PVAL_SNV_BURDEN"):
    """What a group's frame must hold, from the cohort frames: (exact columns as a dict, p [4, members, E])."""
    from digdriver_amd.sequence_model import nb_model
    E = len(full[0])
    p = np.stack([np.stack([_column(full, c, k) for c in idx]) for k in PVALS])                  # [4, members, E]
    have_indel = any("PVAL_INDEL_BURDEN" in full[c].columns for c in idx)
    n_p = 4 if have_indel else 2
    d = {"ELT_SIZE": full[0].ELT_SIZE.values, "N_COHORTS": np.full(E, len(idx), np.int64)}
    for k in ("OBS_SAMPLES", "OBS_SNV", "OBS_INDEL"):
        d[k] = sum(full[c][k].values for c in idx) + 0.0
    for k, gate in (("EXP_SNV", 0), ("EXP_INDEL", 2))[:n_p // 2]:
        acc = np.zeros(E)
        for i, c in enumerate(idx):
            acc = acc + np.where(np.isnan(p[gate, i]), 0.0, _column(full, c, k))
        d[k] = acc
    m = (~np.isnan(p)).sum(axis=1)
    for j in range(n_p):
        d[N_TESTED[j]] = m[j].astype(np.int64)
    order = np.where(np.isnan(p[PVALS.index(best_on)]), np.inf, p[PVALS.index(best_on)]).argmin(axis=0)
    d["BEST_COHORT"] = np.where(m[PVALS.index(best_on)] > 0, np.array(LABELS, dtype=object)[np.array(idx)[order]], "")
    # the exact p-values: one member's own, two members' fisher_combine
    exact = np.full((4, E), np.nan)
    for j in range(4):
        for e in range(E):
            v = p[j, :, e][~np.isnan(p[j, :, e])]
            if len(v) == 1:
                exact[j, e] = v[0]
            elif len(v) == 2:
                exact[j, e] = nb_model.fisher_combine(float(v[0]), float(v[1]))
    return d, p, m, exact, n_p


def test_group_frames_are_the_recombination_of_the_cohort_frames(case):
    from digdriver_amd.sequence_model import nb_model
    mk = load_maker()
    full, meta = case["full"], case["meta"]
    assert [f.attrs["group"] for f in meta] == list(GROUPS)
    seen = {1: 0, 2: 0, 3: 0, "nan": 0}
    for name, f in zip(GROUPS, meta):
        idx = _members(name)
        d, p, m, exact, n_p = recombine(full, idx)
        want_cols = ["ELT_SIZE", "N_COHORTS", "OBS_SAMPLES", "OBS_SNV", "OBS_INDEL", "EXP_SNV"] + (["EXP_INDEL"] if n_p == 4 else []) + \
            PVALS[:n_p] + N_TESTED[:n_p] + QVALS[:n_p] + ["BEST_COHORT"]
        assert list(f.columns) == want_cols and f.index.equals(full[0].index) and f.index.name == "ELT", name
        for k, v in d.items():
            assert f[k].dtype == np.asarray(v).dtype, (name, k)
            if k == "BEST_COHORT":
                assert list(f[k]) == list(v), name
            else:
                assert f[k].values.tobytes() == np.asarray(v).tobytes(), (name, k)
        for j, k in enumerate(PVALS[:n_p]):
            got = f[k].values
            assert np.array_equal(np.isnan(got), m[j] == 0), (name, k)
            few = (m[j] == 1) | (m[j] == 2)
            assert got[few].tobytes() == exact[j][few].tobytes(), (name, k)
            for e in np.flatnonzero(m[j] >= 3):
                want, s = mk.reference(p[j, :, e][~np.isnan(p[j, :, e])])
                r = float(mk.ratios(got[e], want, s))
                print("%s %s element %d: got %r want %r ratio %.3g of M_G = %g" % (name, k, e, got[e], want, r, M_G))
                assert r <= M_G, (name, k, e)
                seen[3] += 1
            seen[1] += int((m[j] == 1).sum())
            seen[2] += int((m[j] == 2).sum())
            seen["nan"] += int((m[j] == 0).sum())
            # the q-values: Benjamini-Hochberg over the group's testable elements
            want_q = pd.Series(np.nan, index=f.index)
            want_q[f[k].notna()] = nb_model.get_q_vals(f[k].dropna().values)
            assert f[QVALS[j]].values.tobytes() == want_q.values.tobytes(), (name, k)
    assert seen[1] and seen[2] and seen[3] and seen["nan"]
    # the element cohort B did not test is carried by the other members
    row = meta[0].loc[case["nan_name"]]
    assert row.N_TESTED_SNV_BURDEN == 2 and row.N_COHORTS == 3 and row.N_TESTED_INDEL_BURDEN <= 1
    assert "PVAL_MUT_BURDEN" in meta[0].columns and "PVAL_MUT_BURDEN" not in meta[2].columns and "EXP_INDEL" not in meta[2].columns
    assert np.isnan(meta[3].loc[case["nan_name"]].PVAL_SNV_BURDEN) and meta[3].loc[case["nan_name"]].BEST_COHORT == ""


def test_a_singleton_group_reproduces_its_cohort_and_a_pair_group_is_fisher_combine(case):
    from digdriver_amd.sequence_model import nb_model
    full, meta = case["full"], dict(zip(GROUPS, case["meta"]))
    for name, c in (("onlyC", 2), ("onlyB", 1)):
        for k in [k for k in PVALS + QVALS if k in full[c].columns]:
            assert meta[name][k].values.tobytes() == full[c][k].values.tobytes(), (name, k)
        assert set(meta[name].BEST_COHORT) <= {LABELS[c], ""}
    ab = meta["ab"]
    both = full[0].PVAL_SNV_BURDEN.notna() & full[1].PVAL_SNV_BURDEN.notna()
    want = nb_model.fisher_combine(full[0].PVAL_SNV_BURDEN.values, full[1].PVAL_SNV_BURDEN.values)
    both = both.values
    assert both.sum() >= 5 and ab.PVAL_SNV_BURDEN.values[both].tobytes() == np.asarray(want)[both].tobytes()
    # without labels the members and BEST_COHORT are indices
    from digdriver_amd.driver_model import cohort_batch
    plain = cohort_batch.run_element_meta(case["muts"], case["pres"], case["ed"], "elts", {"pan": [0, 1, 2]}, qvalues=False)[0]
    pan = meta["pan"]
    assert list(plain.columns) == [k for k in pan.columns if not k.startswith("QVAL_")] and plain.BEST_COHORT.dtype == np.int64
    _exact(plain.drop(columns="BEST_COHORT"), pan[list(plain.columns)].drop(columns="BEST_COHORT"))
    assert [LABELS[i] if i >= 0 else "" for i in plain.BEST_COHORT] == list(pan.BEST_COHORT)


def test_meta_calls_are_the_restricted_frames(case):
    from digdriver_amd.driver_model import cohort_batch
    args = (case["muts"], case["pres"], case["ed"], "elts", GROUPS)
    meta = case["meta"]
    fdr = float(np.median(meta[0].QVAL_SNV_BURDEN.dropna().values))
    hits = cohort_batch.run_element_meta_calls(*args, labels=LABELS, fdr=fdr)
    partial = 0
    for f, h in zip(meta, hits):
        _exact(h, f[f.QVAL_SNV_BURDEN <= fdr])
        assert h.attrs["n_testable"] == int(f.PVAL_SNV_BURDEN.notna().sum()) and h.attrs["group"] == f.attrs["group"]
        partial += 0 < len(h) < h.attrs["n_testable"]
    assert partial >= 1
    # a p-value cut on another column: BEST_COHORT follows it
    cut_on = "PVAL_SAMPLE_BURDEN"
    by_sample = cohort_batch.run_element_meta(*args, labels=LABELS, best_on=cut_on)
    pval_max = float(np.median(by_sample[0][cut_on].dropna().values))
    hits = cohort_batch.run_element_meta_calls(*args, labels=LABELS, pval_max=pval_max, cut_on=cut_on)
    for f, h in zip(by_sample, hits):
        _exact(h, f[f[cut_on] <= pval_max])
        assert h.attrs["n_testable"] == int(f[cut_on].notna().sum())
    assert 0 < len(hits[0]) < len(by_sample[0])
    for f, g in zip(by_sample, meta):
        _exact(f.drop(columns="BEST_COHORT"), g.drop(columns="BEST_COHORT"))
    with pytest.raises(ValueError, match=r"PVAL_MUT_BURDEN: groups \['onlyC'\] have no indel columns"):
        cohort_batch.run_element_meta_calls(*args, labels=LABELS, fdr=0.5, cut_on="PVAL_MUT_BURDEN")


def test_the_command_line_writes_the_group_files_beside_untouched_cohort_files(case):
    spec = importlib.util.spec_from_file_location("dig_driver_cli_element_meta", os.path.join(ROOT, "scripts", "DigDriver.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    tmp = case["tmp"]
    gfile = tmp / "groups.tsv"
    gfile.write_text("".join("%s\t%s\n" % (g, LABELS[LABELS.index(v) if isinstance(v, str) else v]) for g, mem in GROUPS.items() for v in mem))
    read = lambda path: pd.read_csv(path, sep="\t", index_col=0, float_precision="round_trip", keep_default_na=True)
    meta = case["meta"]
    fdr = float(np.median(meta[0].QVAL_SNV_BURDEN.dropna().values))
    for extra, cohort_sfx, group_sfx in (("--qvalues", ".results.txt", ".meta.results.txt"), ("--fdr %r" % fdr, ".hits.txt", ".meta.hits.txt")):
        with_dir, without_dir = str(tmp / ("with" + cohort_sfx)), str(tmp / ("without" + cohort_sfx))
        lists = "--mutation-files %s --maps %s --outpfx A B C" % (" ".join(case["muts"]), " ".join(case["pres"]))
        cli.main("elementCohorts %s elts %s --outdir %s %s --groups %s" % (case["ed"], lists, with_dir, extra, gfile))
        cli.main("elementCohorts %s elts %s --outdir %s %s" % (case["ed"], lists, without_dir, extra))
        assert sorted(os.listdir(without_dir)) == sorted(p + cohort_sfx for p in LABELS)
        assert sorted(os.listdir(with_dir)) == sorted([p + cohort_sfx for p in LABELS] + [g + group_sfx for g in GROUPS])
        for pfx in LABELS:
            assert open(os.path.join(with_dir, pfx + cohort_sfx), "rb").read() == open(os.path.join(without_dir, pfx + cohort_sfx), "rb").read()
        for g, f in zip(GROUPS, meta):
            want = f if group_sfx == ".meta.results.txt" else f[f.QVAL_SNV_BURDEN <= fdr]
            back = read(os.path.join(with_dir, g + group_sfx))
            assert list(back.columns) == list(want.columns) and list(back.index) == list(want.index) and back.index.name == "ELT"
            for col in want.columns:
                if col == "BEST_COHORT":
                    assert list(back[col].fillna("")) == list(want[col]), (g, col)
                else:
                    assert np.array_equal(back[col].values.astype(float), want[col].values.astype(float), equal_nan=True), (g, col)
