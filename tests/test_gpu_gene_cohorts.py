"""GPU tests of geneDriver for many cohorts: engine.gene_counts (dig_gene_row_keys + key sort + dig_gene_counts) bit-exact against the
plain-Python statement gene_obs_statement.py, in its device-tensor and its host-array form; cohort_batch.run_gene_cohorts against
run_gene_model(fused=True) a cohort at a time; the written file against the geneDriver command line; the refusals."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import gene_cohort_cases as K
from conftest import ROOT, rel_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gene_cohorts")
    case = K.small_case(tmp)
    case["maps"] = K.write_maps(tmp, case["C"])
    case["want"] = K.statement_planes(case)
    case["tmp"] = tmp
    return case


@pytest.fixture(scope="module")
def long_run(tmp_path_factory):
    case = K.long_run_case(tmp_path_factory.mktemp("gene_long_run"))
    case["want"] = K.statement_planes(case)
    return case


def _encoded(case):
    from digdriver_amd.data_tools import tabulate_gpu
    index = pd.Index(K.GENES)
    rows = [tabulate_gpu.encode_gene_rows(f, index, c) for c, f in enumerate(case["files"])]
    offsets = np.concatenate([[0], np.cumsum([len(r["sample_names"]) for r in rows])])
    cat = {k: np.concatenate([r[k] for r in rows]) for k in ("gene", "sample", "annot", "cohort")}
    names = [r["sample_names"] for r in rows]
    return cat, offsets, names


def _counts(case, on_device):
    import torch
    from digdriver_amd import engine
    cat, offsets, names = _encoded(case)
    conv = (lambda a: torch.as_tensor(a, device="cuda:0")) if on_device else (lambda a: a)
    out = engine.gene_counts(conv(cat["gene"]), conv(cat["sample"]), conv(cat["annot"]), conv(cat["cohort"]), offsets, len(K.GENES),
                             case["C"], K.GENES.index("TP53"), max_muts_per_sample=case["max_muts_per_sample"],
                             max_muts_per_gene_per_sample=case["max_muts_per_gene_per_sample"])
    if on_device:
        assert all(v.is_cuda for v in out.values())
        out = {k: v.cpu().numpy() for k, v in out.items()}
    return out, offsets, names


@pytest.mark.parametrize("which", ["small", "long_run"])
def test_gene_counts_match_the_statement_in_both_forms(which, small, long_run):
    case = small if which == "small" else long_run
    want = case["want"]
    dev, offsets, names = _counts(case, True)
    host, _, _ = _counts(case, False)
    for k in ("obs", "n_samp", "n_syn", "n_samp_indel", "n_pairs"):
        assert dev[k].dtype == want[k].dtype and dev[k].shape == want[k].shape, k
        assert np.array_equal(dev[k], want[k]), k
    for k in dev:
        assert host[k].dtype == dev[k].dtype and np.array_equal(host[k], dev[k]), k
    assert dev["blacklisted"].dtype == np.uint8 and dev["blacklisted"].shape == (offsets[-1],)
    for c in range(case["C"]):
        black = [n for n, b in zip(names[c], dev["blacklisted"][offsets[c]:offsets[c + 1]]) if b]
        assert sorted(black) == want["blacklist"][c]
    if which == "long_run":                                          # the 700-row run, clipped to the cap of 500
        assert want["raw"][0]["obs"][("G03", "Missense")] >= 500 and want["n_samp"][K.GENES.index("G03"), 1, 0] >= 1
    else:
        assert sum(len(b) for b in want["blacklist"]) == 1 and want["obs"][:, 4, 2].sum() == 0


@pytest.mark.parametrize("n", [600, 577])
def test_sample_totals_of_runs_placed_on_the_wave_and_workgroup_edges(tmp_path, n):
    """dig_gene_row_keys adds a sample's rows once per run of consecutive lanes (segment_count): the runs of K.LANE_RUNS start at
    lane 0 and in mid-wave, end at lane 63, cross a wave and a workgroup boundary, are one row long, and one sample has two of them;
    the lanes behind row n - 1 hold no row (n = 577: the last row is alone in its wave).  The per-sample totals decide
    `blacklisted`, and under the three limits every run on an edge is once at the limit and once one above it; long_run above has
    one 700-row run at the end of random rows and no limit."""
    for limit in K.LANE_RUN_LIMITS:
        case = K.lane_run_case(tmp_path, n, limit)
        want = K.statement_planes(case)
        dev, offsets, names = _counts(case, True)
        host, _, _ = _counts(case, False)
        sample = _encoded(case)[0]["sample"]
        assert np.array_equal(sample, case["sample"][:n]) and offsets.tolist() == [0, sample.max() + 1]      # ids by first appearance
        total = np.bincount(sample)
        assert total[[0, 6, 8, 12]].tolist() == [56, 56, 55, 56] and limit in (total[8] - 1, total[8], total[6])
        assert np.array_equal(dev["blacklisted"], (total > limit).astype(np.uint8)), limit
        for k in ("obs", "n_samp", "n_syn", "n_samp_indel", "n_pairs"):
            assert dev[k].dtype == want[k].dtype and np.array_equal(dev[k], want[k]), (limit, k)
        for k in dev:
            assert host[k].dtype == dev[k].dtype and np.array_equal(host[k], dev[k]), (limit, k)
        assert want["obs"].sum() > 0 and sorted(n_ for n_, b in zip(names[0], dev["blacklisted"]) if b) == want["blacklist"][0]


def test_a_fractional_cap_is_clipped_as_a_number_then_cast(small):
    """3, 4 and 1 Missense rows of one gene in three samples under a cap of 2.5: int(2.5 + 2.5 + 1) = 6."""
    from digdriver_amd import engine
    gene, sample = np.zeros(8, np.int32), np.array([0, 0, 0, 1, 1, 1, 1, 2], np.int32)
    out = engine.gene_counts(gene, sample, np.ones(8, np.uint8), np.zeros(8, np.int32), [0, 3], 1, 1, 2, max_muts_per_gene_per_sample=2.5)
    assert out["obs"][0, :, 0].tolist() == [0, 6, 0, 0, 0] and out["n_samp"][0, :, 0].tolist() == [0, 3, 0, 0, 0, 3]


def _serial(case, c, **kw):
    from digdriver_amd.driver_model import transfer_tools as tt
    return tt.run_gene_model(case["files"][c], case["maps"][c], fused=True, all_cosmic=K.ALL_COSMIC,
                             max_muts_per_sample=case["max_muts_per_sample"],
                             max_muts_per_gene_per_sample=case["max_muts_per_gene_per_sample"], **kw)


@pytest.mark.parametrize("selection", [False, True], ids=["burden", "selection"])
def test_frames_are_those_of_run_gene_model(small, selection):
    from digdriver_amd.driver_model import cohort_batch
    frames = cohort_batch.run_gene_cohorts(small["files"], small["maps"], all_cosmic=K.ALL_COSMIC, selection=selection,
                                           max_muts_per_sample=small["max_muts_per_sample"],
                                           max_muts_per_gene_per_sample=small["max_muts_per_gene_per_sample"])
    assert len(frames) == 3
    for c, got in enumerate(frames):
        want = _serial(small, c, selection=selection)
        assert list(got.columns) == list(want.columns) and list(got.index) == list(want.index) and got.index.name == want.index.name
        assert ("PVAL_INDEL_BURDEN" in got.columns) == (c != 2) and ("PVAL_MUT_BURDEN" in got.columns) == (c != 2)
        assert ("T_SYN" in got.columns) == selection
        for col in got.columns:
            x, y = got[col].values, want[col].values
            assert x.dtype == y.dtype, (c, col, x.dtype, y.dtype)
            if col.startswith(("OBS_", "N_SAMP_")) or x.dtype.kind not in "f":
                assert (x == y).all(), (c, col)
            elif col == "THETA":                                     # the scale factor, to the last bit: THETA = sigma^2 / mu * cj
                assert np.array_equal(x, y), (c, col)
            else:
                rel_close(x, y, 1e-9)
        for a, name in enumerate(K._OBS):                            # and the statement once more, through the whole driver
            assert (got[name].values == small["want"]["obs"][:, a, c]).all()


def test_written_file_is_the_gene_driver_command_lines(small):
    from digdriver_amd.driver_model import cohort_batch, transfer_tools as tt
    tmp = small["tmp"]
    panel = tmp / "panels"
    panel.mkdir(exist_ok=True)
    (panel / "genes_CGC_ALL.txt").write_text("".join(s + "\n" for s in K.ALL_COSMIC))
    frames, paths = cohort_batch.run_and_write_gene_cohorts(small["files"], small["maps"], str(tmp / "batch"), ["c0", "c1", "c2"],
                                                            all_cosmic=K.ALL_COSMIC + tt._COSMIC_EXTRA, selection=True,
                                                            max_muts_per_sample=small["max_muts_per_sample"],
                                                            max_muts_per_gene_per_sample=small["max_muts_per_gene_per_sample"])
    assert [os.path.basename(p) for p in paths] == ["c0.results.txt", "c1.results.txt", "c2.results.txt"] and len(frames) == 3
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "DigDriver.py"), "geneDriver", small["files"][1], small["maps"][1],
           "--panel-dir", str(panel), "--outdir", str(tmp / "cli"), "--outpfx", "c1", "--selection",
           "--max-muts-per-sample", str(small["max_muts_per_sample"]),
           "--max-muts-per-gene-per-sample", str(small["max_muts_per_gene_per_sample"])]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=120)
    with open(paths[1], "rb") as a, open(tmp / "cli" / "c1.results.txt", "rb") as b:
        assert a.read() == b.read()


def _no_launch(monkeypatch):
    from digdriver_amd import _lib

    def refuse(name, *args):
        raise AssertionError("a library call (%s) in front of the refusal" % name)
    monkeypatch.setattr(_lib, "call", refuse)


def test_refusals_come_before_any_launch(small, tmp_path, monkeypatch):
    from digdriver_amd.driver_model import cohort_batch
    from digdriver_amd.io import mapfile
    maps = K.write_maps(tmp_path, 3)
    other = K.model_frame(1)
    other = other.iloc[::-1].reset_index(drop=True)                  # the same genes in another order
    mapfile.write_frame(maps[1], "genic_model", other)
    _no_launch(monkeypatch)
    with pytest.raises(ValueError, match="genes1.map"):
        cohort_batch.run_gene_cohorts(small["files"], maps)
    with pytest.raises(NotImplementedError):
        cohort_batch.run_gene_cohorts(small["files"], small["maps"], scale_by_sample=True)
