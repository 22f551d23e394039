"""GPU tests of the gene route's dN/dS correction and selection tests (dig_gene_selection) against the reference's own
functions: tests/golden/gene_selection_golden.npz holds the 34 columns gene_expected_muts_dnds, gene_pvalue_burden_dnds,
gene_pvalue_sel_nb, gene_pvalue_sel_gamma and selection_coefficient wrote for 1 000 genes + an edge block x 3 cohorts
(tests/golden/make_selection_golden.py).  Tolerance: conftest.rel_close, rtol 1e-6, floor 1e-250, matching NaN positions; the 14
arithmetic planes (T_SYN, MRFOLD, EXP_c_ML, SEL_c) are the reference's bits.  tests/test_gpu_gene_selection_routes.py holds the
p-value planes to 80-digit references."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN, ROOT, rel_close

pytestmark = pytest.mark.gpu

CLASSES = ("SYN", "MIS", "NONS", "SPL", "TRUNC", "NONSYN")
DNDS_COLS = ["T_SYN", "MRFOLD"] + ["EXP_%s_ML" % c for c in CLASSES]
BURDEN_DNDS_COLS = ["PVAL_%s_BURDEN_DNDS" % c for c in CLASSES]
SEL_NB_COLS = ["PVAL_%s_SEL_NB" % c for c in ("SYN", "MIS", "TRUNC", "NONSYN")]


@pytest.fixture(scope="module")
def gold():
    from digdriver_amd import _lib
    _lib.require_device()
    g = np.load(os.path.join(GOLDEN, "gene_selection_golden.npz"), allow_pickle=False)
    G, C = g["alpha"].shape
    assert (G, C) == (1048, 3) and g["planes"].shape == (34, G, C)
    assert [str(s) for s in g["plane_names"]] == list(_lib.SEL_PLANES)
    pi = np.ascontiguousarray(np.broadcast_to(g["pi"][:, :, None], (G, 6, C)))
    return dict(alpha=g["alpha"], theta=g["theta"], pi=pi, obs=g["obs"], planes=g["planes"], genes=[str(s) for s in g["genes"]],
                added={k[6:]: [str(s) for s in g[k]] for k in g.files if k.startswith("added_")})


@pytest.fixture(scope="module")
def device_planes(gold):
    """engine.gene_selection on device tensors, once: [34, G, C] as a host array."""
    import torch
    from digdriver_amd import engine
    dev = torch.device("cuda:0")
    t = {k: torch.as_tensor(gold[k], device=dev) for k in ("alpha", "theta", "pi", "obs")}
    res = engine.gene_selection(t["alpha"], t["theta"], t["pi"], t["obs"])
    assert list(res) == list(engine.SEL_PLANES) and all(v.is_cuda and v.shape == gold["alpha"].shape for v in res.values())
    return np.stack([res[name].cpu().numpy() for name in engine.SEL_PLANES])


def _check_planes(got, gold):
    from digdriver_amd import _lib
    for i, name in enumerate(_lib.SEL_PLANES):
        try:
            rel_close(got[i], gold["planes"][i], 1e-6)
        except AssertionError as exc:
            raise AssertionError("%s: %s" % (name, exc))
        # pure arithmetic, contraction off: every operation rounds as the reference's numpy operation does
        if name in ("T_SYN", "MRFOLD") or name.startswith(("EXP_", "SEL_")):
            assert np.array_equal(got[i], gold["planes"][i], equal_nan=True), "%s: not the reference's bits" % name


def test_device_entry_matches_the_reference_planes(gold, device_planes):
    _check_planes(device_planes, gold)


def test_four_class_probabilities_give_the_same_planes(gold):
    """n_pi = 4: TRUNC and NONSYN are formed in the kernel, as dig_gene_stats forms them."""
    import torch
    from digdriver_amd import engine
    dev = torch.device("cuda:0")
    res = engine.gene_selection(torch.as_tensor(gold["alpha"], device=dev), torch.as_tensor(gold["theta"], device=dev),
                                torch.as_tensor(gold["pi"][:, :4, :].copy(), device=dev), torch.as_tensor(gold["obs"], device=dev))
    _check_planes(np.stack([res[name].cpu().numpy() for name in engine.SEL_PLANES]), gold)


def test_host_twin_gives_the_bits_of_the_device_entry(gold, device_planes):
    from digdriver_amd import engine
    res = engine.gene_selection(gold["alpha"], gold["theta"], gold["pi"], gold["obs"])
    for i, name in enumerate(engine.SEL_PLANES):
        assert isinstance(res[name], np.ndarray)
        assert np.array_equal(res[name], device_planes[i], equal_nan=True), name
    # one cohort given as vectors and a [G, n_pi] table
    one = engine.gene_selection(gold["alpha"][:, 1], gold["theta"][:, 1], gold["pi"][:, :, 1], gold["obs"][:, :, 1:2])
    for i, name in enumerate(engine.SEL_PLANES):
        assert np.array_equal(one[name][:, 0], device_planes[i][:, 1], equal_nan=True), name


def _cohort_frame(gold, c):
    df = pd.DataFrame(index=gold["genes"])
    df["ALPHA"], df["THETA"] = gold["alpha"][:, c], gold["theta"][:, c]
    for q, cls in enumerate(CLASSES):
        df["Pi_" + cls] = gold["pi"][:, q, c]
    obs = gold["obs"][:, :, c].astype(float)
    for q, cls in enumerate(("SYN", "MIS", "NONS", "SPL")):
        df["OBS_" + cls] = obs[:, q]
    df["OBS_TRUNC"] = df.OBS_NONS + df.OBS_SPL
    df["OBS_NONSYN"] = df.OBS_MIS + df.OBS_TRUNC
    return df


def _steps(tt):
    steps = [("gene_expected_muts_dnds", tt.gene_expected_muts_dnds), ("gene_pvalue_burden_dnds", tt.gene_pvalue_burden_dnds),
             ("gene_pvalue_sel_nb", tt.gene_pvalue_sel_nb), ("gene_pvalue_sel_gamma", tt.gene_pvalue_sel_gamma)]
    return steps + [("selection_coefficient_" + c, lambda d, c=c: tt.selection_coefficient(d, c)) for c in CLASSES]


def test_frame_functions_add_the_reference_columns_in_order(gold):
    from digdriver_amd import _lib
    from digdriver_amd.driver_model import transfer_tools as tt
    c = 2
    df = _cohort_frame(gold, c)
    row = {name: i for i, name in enumerate(_lib.SEL_PLANES)}
    for name, fn in _steps(tt):
        before = list(df.columns)
        out = fn(df)
        assert out is df                                          # mutates and returns the frame
        new = [col for col in df.columns if col not in before]
        assert new == gold["added"][name], name
        for col in new:
            if col in row:
                rel_close(df[col].values, gold["planes"][row[col]][:, c], 1e-6)
    for q, cls in enumerate(CLASSES):                             # EXP_c: the columns gene_expected_muts_nb writes
        with np.errstate(all="ignore"):
            want = gold["alpha"][:, c] * gold["theta"][:, c] * gold["pi"][:, q, c]
        assert np.array_equal(df["EXP_" + cls].values, want, equal_nan=True)
    only = tt.selection_coefficient(_cohort_frame(gold, c), "TRUNC", pvalue=False)
    assert "SEL_TRUNC" in only.columns and "PVAL_TRUNC_SEL" not in only.columns


def test_selection_block_gives_the_values_of_the_functions_in_sequence(gold):
    from digdriver_amd.driver_model import transfer_tools as tt
    seq = _cohort_frame(gold, 1)
    for _, fn in _steps(tt):
        seq = fn(seq)
    blk = tt.gene_selection_block(_cohort_frame(gold, 1))
    want = ["EXP_" + c for c in CLASSES] + DNDS_COLS + BURDEN_DNDS_COLS + SEL_NB_COLS
    assert list(blk.columns)[-len(want):] == want
    for col in want:
        assert np.array_equal(blk[col].values, seq[col].values, equal_nan=True), col
    part = tt.gene_selection_block(_cohort_frame(gold, 1), burden_dnds=False)
    assert list(part.columns)[-len(DNDS_COLS + SEL_NB_COLS):] == DNDS_COLS + SEL_NB_COLS and "PVAL_SYN_BURDEN_DNDS" not in part.columns


@pytest.fixture(scope="module")
def gene_map(tmp_path_factory):
    """The pretrained gene model of test_gpu_host_mirror.py::test_run_gene_model_matches_reference as a map directory."""
    from digdriver_amd.io import mapfile
    g = np.load(os.path.join(GOLDEN, "gene_stats_golden.npz"))
    frame = pd.DataFrame(g["frame_vals"], columns=list(g["frame_cols"]))
    for c in ("GENE_LENGTH", "R_SIZE", "R_OBS", "R_INDEL", "FLAG"):
        frame[c] = frame[c].astype(np.int64)
    frame.insert(0, "GENE", g["genes"])
    frame.insert(0, "CHROM", g["frame_chrom"])
    path = str(tmp_path_factory.mktemp("selection") / "genes.map")
    mapfile.write_frame(path, "genic_model", frame)
    return path, g


def _run(gene_map, **kw):
    from digdriver_amd.driver_model import transfer_tools as tt
    path, g = gene_map
    return tt.run_gene_model(os.path.join(GOLDEN, "gene_mutations.tsv"), path, max_muts_per_sample=int(g["max_muts_per_sample"]),
                             max_muts_per_gene_per_sample=int(g["max_muts_per_gene_per_sample"]),
                             all_cosmic=list(g["null_excluded"]), **kw)


def _same_frame(a, b):
    assert list(a.columns) == list(b.columns) and list(a.index) == list(b.index)
    for c in a.columns:
        x, y = a[c].values, b[c].values
        assert np.array_equal(x, y, equal_nan=True) if x.dtype.kind == "f" else (x == y).all(), c


def test_run_gene_model_selection_columns(gold, gene_map):
    _, g = gene_map
    today = [str(c) for c in g["out_cols"]]
    off = _run(gene_map, fused=True, selection=False)
    assert [c for c in off.columns if c != "CHROM"] == today
    for i, c in enumerate(today):
        rel_close(off[c].values.astype(float), g["out_vals"][:, i], 1e-6)
    # the new columns sit between the PVAL_*_BURDEN_SAMPLE block and the indel columns; both routes write the same frame
    at = today.index("PVAL_NONSYN_BURDEN_SAMPLE") + 1
    want = today[:at] + DNDS_COLS + BURDEN_DNDS_COLS + SEL_NB_COLS + today[at:]
    frames = [_run(gene_map, fused=fused, selection=True) for fused in (False, True)]
    _same_frame(frames[0], frames[1])
    on = frames[1]
    assert [c for c in on.columns if c != "CHROM"] == want
    for c in today:                                               # nothing that exists today changes
        assert np.array_equal(on[c].values, off[c].values, equal_nan=True), c
    # the first cohort of the golden is this frame's first 1 000 genes
    from digdriver_amd import _lib
    n = 1000
    assert list(on.index[:n]) == gold["genes"][:n]
    for c in DNDS_COLS + BURDEN_DNDS_COLS + SEL_NB_COLS:
        rel_close(on[c].values[:n], gold["planes"][_lib.SEL_PLANES.index(c)][:n, 0], 1e-6)
    no_sel = _run(gene_map, fused=True, selection=True, pval_sel=False)
    assert [c for c in no_sel.columns if c != "CHROM"] == [c for c in want if c not in SEL_NB_COLS]
    no_dnds = _run(gene_map, fused=False, selection=True, pval_burden_dnds=False)
    assert [c for c in no_dnds.columns if c != "CHROM"] == [c for c in want if c not in BURDEN_DNDS_COLS]


def test_gene_driver_cli_writes_the_selection_columns_without_torch(gene_map, tmp_path):
    path, g = gene_map
    panel = tmp_path / "panels"
    panel.mkdir()
    (panel / "genes_CGC_ALL.txt").write_text("".join(s + "\n" for s in g["null_excluded"]))
    env = dict(os.environ, DIG_CLI_ASSERT_NO_TORCH="1")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "DigDriver.py"), "geneDriver", os.path.join(GOLDEN, "gene_mutations.tsv"), path,
           "--panel-dir", str(panel), "--outdir", str(tmp_path), "--outpfx", "sel", "--selection", "--max-muts-per-sample", "170",
           "--max-muts-per-gene-per-sample", "3"]
    subprocess.run(cmd, check=True, env=env, stdout=subprocess.DEVNULL, timeout=120)
    with open(tmp_path / "sel.results.txt") as f:
        header = f.readline().rstrip("\n").split("\t")
    at = header.index("PVAL_NONSYN_BURDEN_SAMPLE") + 1
    new = DNDS_COLS + BURDEN_DNDS_COLS + SEL_NB_COLS
    assert header[at:at + len(new)] == new
    assert header[at + len(new)] == "EXP_INDEL"
