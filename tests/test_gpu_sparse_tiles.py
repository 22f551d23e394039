"""The sparse per-base scan on the GPU (dig_tile_census, dig_sparse_tile_keys, the key sort, dig_sparse_tile_test behind
engine.tile_census / engine.sparse_tile_test; nb_model.nb_model_hits_sparse; `DigDriver.py tileDriver --sparse`).
  1  the census against dig_base_tile_probs_ctx (first_pos, n_valid bit for bit; n_positive = the count of pt > 0 in the dense plane)
     and against the plain-Python statement (denom to 1e-12), n_up 1 and 2, binsize 1, 7, 50, C = 3 and 65
  2  the mutated tiles of the engine against the statement (k exact, pt to 1e-12) and against the dense planes (pval to 1e-6),
     with rows of cohorts outside [0, C)
  3  nb_model_hits_sparse against nb_model_hits on the problem of tile_samples_cases (binsize 1: certified, every cut; binsize 50: not)
     and on the problem of sparse_tiles_cases (N-window rows, a zero-S_prob cohort, NaN and 0 mu, overlapping regions, a depleted
     cohort whose empty tiles are dense hits, C = 65)
  4  host arrays and device tensors give the same bits; two calls give the same bits
  5  tileDriver --sparse in a fresh child process; without --sparse the bytes of nb_model_hits
Exact: index, CHROM, POS, OBS, MU, SIGMA, REGION, n_testable, n_tiles.  Pi and EXP to 1e-12 relative (another order of additions in
the denominator), PVAL and QVAL to 1e-6 relative (the project's pin for p-values).
All new kernels launch a workgroup per region or a thread per key on an uncapped grid: there is no grid-stride state to test."""
import functools
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from conftest import ROOT
import sparse_tiles_cases as P
import sparse_tiles_statement as S
import tile_samples_cases as K

pytestmark = pytest.mark.gpu

EXACT = ["CHROM", "POS", "OBS", "MU", "SIGMA", "REGION"]
NEAR = 2e-6              # a dense value this close to its cut could fall on either side in the other route


@functools.lru_cache(maxsize=None)
def _genome():
    from digdriver_amd.data_tools.genome import PackedGenome
    return PackedGenome.from_sequences(K.genome_sequences())


@functools.lru_cache(maxsize=None)
def _old_problem():
    rows = [[r[:3] for r in rows] for rows in K.cohort_rows()]
    mu, sigma = K.mu_sigma()
    return dict(idx=K.IDX, rows=rows, frames=P.frames(rows), d_prs=[K.s_prob(c) for c in range(K.C)], mu=mu, sigma=sigma)


@functools.lru_cache(maxsize=None)
def _new_problem(C):
    rows = P.cohort_rows(C)
    mu, sigma = P.mu_sigma(C)
    return dict(idx=P.IDX, rows=rows, frames=P.frames(rows), d_prs=[P.s_prob(c) for c in range(C)], mu=mu, sigma=sigma)


def _call(fn, prob, binsize, **cut):
    return fn(prob["d_prs"], prob["idx"], prob["mu"], prob["sigma"], prob["frames"], _genome(), n_up=1, n_down=1, binsize=binsize, **cut)


@functools.lru_cache(maxsize=None)
def _dense(which, binsize, kind, level):
    """The dense route's frames, computed once per cut and left unchanged.  bonferroni: the dense route has no such keyword; its cut
    is pval_max = level / n_testable per cohort, one call per distinct cut."""
    from digdriver_amd.sequence_model import nb_model
    prob = _old_problem() if which == "old" else _new_problem(which)
    if kind != "bonferroni":
        return _call(nb_model.nb_model_hits, prob, binsize, **{kind: level})
    n_test = [f.attrs["n_testable"] for f in _call(nb_model.nb_model_hits, prob, binsize, pval_max=0.5)]
    by_cut = {n: _call(nb_model.nb_model_hits, prob, binsize, pval_max=level / max(n, 1)) for n in sorted(set(n_test))}
    return [by_cut[n][c] for c, n in enumerate(n_test)]


def _sparse(which, binsize, kind, level):
    from digdriver_amd.sequence_model import nb_model
    prob = _old_problem() if which == "old" else _new_problem(which)
    return _call(nb_model.nb_model_hits_sparse, prob, binsize, **{kind: level})


def _all_tiles(which, binsize):
    """Every tile with OBS >= 1 of the dense route with its PVAL (pval_max = 2 takes every testable tile) -- for the guard below."""
    return [f[f.OBS >= 1] for f in _dense(which, binsize, "pval_max", 2.0)]


def _assert_no_value_near_the_cut(which, binsize, kind, level):
    """On the DENSE results: no mutated tile's PVAL (for fdr: no QVAL of the whole list) within 2e-6 relative of the cut -- otherwise
    an equal hit list would prove nothing about the selection."""
    from digdriver_amd.sequence_model import nb_model
    for c, f in enumerate(_all_tiles(which, binsize)):
        n = f.attrs["n_testable"]
        if kind == "fdr":
            everything = _dense(which, binsize, "pval_max", 2.0)[c]
            assert len(everything) == n
            x, cut = nb_model.get_q_vals(everything.PVAL.values)[everything.OBS.values >= 1], level
        else:
            x, cut = f.PVAL.values, level / max(n, 1) if kind == "bonferroni" else level
        assert not (np.abs(x - cut) <= NEAR * cut).any(), (which, binsize, kind, c)


def _assert_frames_equal(sp, de, fdr):
    assert list(sp.columns) == list(de.columns) and list(sp.dtypes) == list(de.dtypes)
    assert sp.index.dtype == np.int64 and np.array_equal(sp.index.values, de.index.values)
    for col in EXACT:
        a, b = sp[col].values, de[col].values
        assert np.array_equal(a, b) if col == "REGION" else np.array_equal(a, b, equal_nan=True), col
    for col, tol in (("Pi", 1e-12), ("EXP", 1e-12), ("PVAL", 1e-6)) + ((("QVAL", 1e-6),) if fdr else ()):
        np.testing.assert_allclose(sp[col].values, de[col].values, rtol=tol, atol=0, err_msg=col)
    assert sp.attrs["n_testable"] == de.attrs["n_testable"] and sp.attrs["n_tiles"] == de.attrs["n_tiles"]


# ---- 1: the census -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 65])
@pytest.mark.parametrize("binsize", P.BINSIZES)
@pytest.mark.parametrize("n_up", [1, 2])
def test_census_equals_the_dense_front_half_and_the_statement(n_up, binsize, C):
    import torch
    from digdriver_amd import engine
    tables = [P.s_prob(c, n_up) for c in range(C)]
    keys = sorted(tables[0])
    s_prob = np.array([[t[k] for k in keys] for t in tables])
    chroms, st, en = [str(c) for c in P.IDX[:, 0]], P.IDX[:, 1], P.IDX[:, 2]
    first, nval, denom, npos = engine.tile_census(_genome(), chroms, st, en, s_prob, binsize)
    pt, first_d, nval_d = engine.base_tile_probs(_genome(), chroms, st, en, s_prob, binsize)
    assert first.dtype == torch.int64 and nval.dtype == torch.int32 and denom.dtype == torch.float64 and npos.dtype == torch.int32
    assert torch.equal(first, first_d) and torch.equal(nval, nval_d)
    exists = torch.arange(pt.shape[2], device=pt.device)[None, None, :] < nval_d[None, :, None]
    assert torch.equal(npos.long(), ((pt > 0) & exists).sum(dim=2))
    assert denom.shape == (C, len(P.IDX)) and npos.shape == (C, len(P.IDX))
    s_first, s_nval, s_denom, s_npos = S.census(K.genome_sequences(), P.regions(), tables, n_up, binsize, pt.shape[2])
    assert first.tolist() == s_first and nval.tolist() == s_nval and npos.tolist() == s_npos
    np.testing.assert_allclose(denom.cpu().numpy(), np.array(s_denom), rtol=1e-12, atol=0)
    assert nval.tolist()[5] == 0 and (denom[:, 2] == 0).all() and (npos[:, 2] == 0).all()       # no position; all N
    if binsize == 1:
        assert int(npos[1].sum()) < int(npos[0].sum())                     # the cohort with zeros in its table has fewer such tiles
    # fewer tiles than the regions hold: the counts stop at n_tiles, the denominators do not
    cap = max(1, pt.shape[2] // 2)
    first2, nval2, denom2, npos2 = engine.tile_census(_genome(), chroms, st, en, s_prob, binsize, n_tiles=cap)
    assert torch.equal(first2, first) and torch.equal(nval2, torch.clamp(nval, max=cap)) and torch.equal(denom2, denom)
    assert torch.equal(npos2.long(), ((pt[:, :, :cap] > 0) & exists[:, :, :cap]).sum(dim=2))


# ---- 2: the mutated tiles of the engine ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_up,binsize", [(1, 7), (2, 7), (1, 1), (2, 50)])
def test_mutated_tiles_equal_the_statement_and_the_dense_planes(n_up, binsize):
    import torch
    from digdriver_amd import engine
    C = 4
    tables = [P.s_prob(c, n_up) for c in range(C)]
    keys = sorted(tables[0])
    s_prob = np.array([[t[k] for k in keys] for t in tables])
    mu, sigma = P.mu_sigma(C)
    st = P.stacked(P.cohort_rows(C))                                       # (with two rows of cohorts C and -1)
    chroms, rs, re_ = [str(c) for c in P.IDX[:, 0]], P.IDX[:, 1], P.IDX[:, 2]
    g = _genome()
    dense = engine.tiled_nb_model(g, chroms, rs, re_, s_prob, mu, sigma, st["chrom"], st["start"], st["end"], st["cohort"], binsize=binsize)
    T = dense["pt"].shape[2]
    first, nval, denom, _ = engine.tile_census(g, chroms, rs, re_, s_prob, binsize)
    got = engine.sparse_tile_test(g, chroms, rs, re_, s_prob, binsize, T, first, nval, denom, mu, sigma, st["chrom"], st["start"], st["end"],
                                  st["cohort"])
    at = tuple(got[k].long() for k in ("cohort", "region", "tile"))
    # exactly the tiles with a row, in the dense frame's order
    want = torch.nonzero(dense["k"] > 0)
    assert torch.equal(torch.stack(at, dim=1), want)
    assert torch.equal(got["k"], dense["k"][at])
    ref = S.mutated_tiles(K.genome_sequences(), P.regions(), P.statement_rows(st), tables, n_up, binsize, T)
    tiles = [tuple(int(v) for v in row) for row in want.tolist()]
    assert tiles == sorted(ref) and got["k"].tolist() == [ref[t][0] for t in tiles]
    np.testing.assert_allclose(got["pt"].cpu().numpy(), np.array([ref[t][1] for t in tiles]), rtol=1e-12, atol=0)
    for name, tol in (("pt", 1e-12), ("exp", 1e-12), ("pval", 1e-6)):
        np.testing.assert_allclose(got[name].cpu().numpy(), dense[name][at].cpu().numpy(), rtol=tol, atol=0, err_msg=name)
    k = got["k"].cpu().numpy()
    assert k.max() >= 300 and (k >= 70).sum() >= 3                          # the run longer than a workgroup; the tile two regions share
    pv, pi = got["pval"].cpu().numpy(), got["pt"].cpu().numpy()
    assert np.isnan(pv).any() and ((pi == 0) & (pv == 0)).any()             # rows in regions without a test; rows on N windows


# ---- 3: the function against the dense route -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,level", [("pval_max", 0.05), ("fdr", 0.1), ("bonferroni", 0.05)])
def test_certified_scan_equals_the_dense_route(kind, level):
    """tile_samples_cases at binsize 1: floors 0.745, 0.580, 0.669 -- every cohort certified, the frames are the dense ones."""
    _assert_no_value_near_the_cut("old", 1, kind, level)
    sparse, dense = _sparse("old", 1, kind, level), _dense("old", 1, kind, level)
    assert [round(f.attrs["zero_floor"], 3) for f in sparse] == [0.745, 0.580, 0.669]
    for sp, de in zip(sparse, dense):
        assert sp.attrs["complete"] is True
        if kind == "bonferroni":
            de = de.drop(columns="QVAL", errors="ignore")
        _assert_frames_equal(sp, de, kind == "fdr")
    assert sum(len(f) for f in sparse) > 0 and (kind != "pval_max" or all(len(f) > 20 for f in sparse))


def test_uncertified_scan_says_so_and_fdr_refuses():
    """The same problem at binsize 50: every tile carries about seven rows, the floors are 2.8e-5, 1.1e-7, 2.0e-6."""
    from digdriver_amd.sequence_model import nb_model
    _assert_no_value_near_the_cut("old", 50, "pval_max", 1e-3)
    sparse, dense = _sparse("old", 50, "pval_max", 1e-3), _dense("old", 50, "pval_max", 1e-3)
    for sp, de in zip(sparse, dense):
        assert sp.attrs["complete"] is False and sp.attrs["zero_floor"] < 1e-3
        _assert_frames_equal(sp, de[de.OBS >= 1], False)
    assert len(sparse[0]) > 0
    with pytest.raises(ValueError, match=r"cohorts \[0, 1, 2\]") as exc:
        _sparse("old", 50, "fdr", 0.1)
    assert "fdr = 0.1" in str(exc.value) and "2.77e-05" in str(exc.value)


@pytest.mark.parametrize("C", [4, 65])
@pytest.mark.parametrize("kind,level", [("pval_max", 0.05), ("fdr", 0.1), ("bonferroni", 0.05)])
def test_new_cases_at_binsize_one(kind, level, C):
    _assert_no_value_near_the_cut(C, 1, kind, level)
    sparse, dense = _sparse(C, 1, kind, level), _dense(C, 1, kind, level)
    assert len(sparse) == C
    for sp, de in zip(sparse, dense):
        assert sp.attrs["complete"] is True
        _assert_frames_equal(sp, de, kind == "fdr")
    # the rows on windows with an N come out as the dense route has them: Pi = 0, PVAL = 0, hits at any cut
    n_rows = sparse[0][(sparse[0].Pi == 0) & (sparse[0].PVAL == 0)]
    assert {999.0, 1000.0, 1050.0} <= set(n_rows.POS) and (n_rows.OBS >= 1).all()
    # n_testable of the cohort with zeros in its table, and of regions with NaN / 0 mu, is the dense one (asserted above) and smaller
    assert sparse[1].attrs["n_testable"] < sparse[0].attrs["n_testable"]


@pytest.mark.parametrize("C", [4, 65])
def test_new_cases_with_a_depleted_cohort_at_binsize_fifty(C):
    _assert_no_value_near_the_cut(C, 50, "pval_max", 1e-3)
    sparse, dense = _sparse(C, 50, "pval_max", 1e-3), _dense(C, 50, "pval_max", 1e-3)
    d = dense[P.DEPLETED]
    assert (d.OBS == 0).sum() >= 3 and set(d[d.OBS == 0].REGION) == {"1:1500-1900"}        # empty tiles ARE dense hits there
    for c, (sp, de) in enumerate(zip(sparse, dense)):
        _assert_frames_equal(sp, de[de.OBS >= 1], False)
    assert sparse[P.DEPLETED].attrs["complete"] is False and sparse[P.DEPLETED].attrs["zero_floor"] < 1e-20
    assert len(sparse[P.DEPLETED]) < len(d)


# ---- 4: forms of input, determinism --------------------------------------------------------------------------------------------
def _bits(x):
    x = x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    return x.dtype.str, x.shape, x.tobytes()


@pytest.mark.parametrize("n_up,binsize", [(1, 1), (2, 50)])
def test_host_arrays_and_device_tensors_give_the_same_bits(n_up, binsize):
    from digdriver_amd import engine
    C = 4
    s_prob = np.array([[t[k] for k in sorted(t)] for t in (P.s_prob(c, n_up) for c in range(C))])
    mu, sigma = P.mu_sigma(C)
    st = P.stacked(P.cohort_rows(C))
    chroms, rs, re_ = [str(c) for c in P.IDX[:, 0]], P.IDX[:, 1], P.IDX[:, 2]
    g = _genome()
    dev = engine.tile_census(g, chroms, rs, re_, s_prob, binsize)
    host = engine.tile_census(g, chroms, rs, re_, s_prob, binsize, on_device=False)
    assert all(isinstance(h, np.ndarray) for h in host)
    assert [_bits(a) for a in dev] == [_bits(b) for b in host]
    T = -(-400 // binsize)
    rows = (st["chrom"], st["start"], st["end"], st["cohort"])
    a = engine.sparse_tile_test(g, chroms, rs, re_, s_prob, binsize, T, dev[0], dev[1], dev[2], mu, sigma, *rows)
    b = engine.sparse_tile_test(g, chroms, rs, re_, s_prob, binsize, T, host[0], host[1], host[2], mu, sigma, *rows)
    assert all(isinstance(v, np.ndarray) for v in b.values()) and len(b["k"]) > 100
    assert {k: _bits(v) for k, v in a.items()} == {k: _bits(v) for k, v in b.items()}


def test_two_calls_give_the_same_bits():
    for kind, level in (("fdr", 0.1), ("pval_max", 0.05)):
        one, two = _sparse(65, 1, kind, level), _sparse(65, 1, kind, level)
        for a, b in zip(one, two):
            assert a.attrs == b.attrs and a.index.equals(b.index)
            for col in a.columns:
                assert _bits(a[col].values if col != "REGION" else a[col].values.astype(str)) == \
                    _bits(b[col].values if col != "REGION" else b[col].values.astype(str)), col


# ---- 5: the command line -------------------------------------------------------------------------------------------------------
def test_tile_driver_sparse_in_a_fresh_child_process(tmp_path):
    """`DigDriver.py tileDriver --sparse` in a child process of its own writes nb_model_hits_sparse's frames and says where the scan
    is incomplete; the same command without --sparse writes the bytes of nb_model_hits."""
    from digdriver_amd.io import mapfile
    C = 4
    prob = _new_problem(C)
    fasta = tmp_path / "genome.fa"
    fasta.write_text("".join(">%s\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))) for n, s in K.genome_sequences().items()))
    maps, files = [], []
    for c in range(C):
        m = str(tmp_path / ("map%d" % c))
        mapfile.write_frame(m, "region_params", pd.DataFrame({"CHROM": P.IDX[:, 0], "START": P.IDX[:, 1], "END": P.IDX[:, 2],
                                                              "Y_PRED": prob["mu"][c], "STD": prob["sigma"][c]}))
        mapfile.write_frame(m, "sequence_model_64", pd.DataFrame({"FREQ": list(prob["d_prs"][c].values())},
                                                                 index=pd.Index(list(prob["d_prs"][c].keys()), name="CONTEXT")))
        maps.append(m)
        files.append(P.write_file(tmp_path / ("muts%d.bed" % c), prob["rows"][c]))
    script = os.path.join(ROOT, "scripts", "DigDriver.py")
    head = [sys.executable, script, "tileDriver", str(fasta), "--maps"] + maps + ["--mutation-files"] + files + \
        ["--binsize", "50", "--outpfx", "A", "B", "C", "D", "--pval-max", "1e-3"]
    runs = [subprocess.Popen(head + ["--outdir", str(tmp_path / "sparse"), "--sparse"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True),
            subprocess.Popen(head + ["--outdir", str(tmp_path / "dense")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)]
    said = []
    for run in runs:
        out, _ = run.communicate(timeout=300)
        assert run.returncode == 0, out
        said.append(out)
    assert said[0].count("(mutated tiles only)") == C and "zero-tile floor" in said[0]         # (at binsize 50 no cohort is certified)
    assert "zero-tile floor" not in said[1] and "mutated tiles only" not in said[1]
    sparse, dense = _sparse(C, 50, "pval_max", 1e-3), _dense(C, 50, "pval_max", 1e-3)
    for pfx, sp, de in zip("ABCD", sparse, dense):
        for sub, frame in (("sparse", sp), ("dense", de)):
            want = tmp_path / ("want_%s_%s.txt" % (sub, pfx))
            mapfile.write_results_tsv(frame, str(want))
            assert (tmp_path / sub / (pfx + ".hits.txt")).read_bytes() == want.read_bytes(), (sub, pfx)
    assert sum(len(f) for f in sparse) > 0
