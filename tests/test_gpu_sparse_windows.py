"""The sparse sliding-window scan on the GPU (dig_tile_window_census, dig_sparse_window_count, dig_sparse_window_test behind
engine.tile_window_census / engine.sparse_window_test; nb_model.nb_model_window_hits_sparse; `DigDriver.py tileDriver --sparse
--sparse-windows`), on both problems of sparse_tiles_cases (C = 3: tile_samples_cases' regions and rows; C = 4 and 65: its own, with N
runs, the all-N region, n_valid = 0, overlapping regions, the contig end, NaN and 0 mu, a zero-S_prob cohort, a depleted cohort).
  1  the window census against dig_tile_window_test's n_windows (bit for bit), the count of pt_w > 0 in the dense window planes and
     the plain-Python statement; with the census' n_positive (the shortcut) and without (the walk)
  2  the candidate windows against the dense window planes {k_w >= 1, w < n_windows}: the set, the order, each once, k exact, pt and
     exp to 1e-12, pval to 1e-6 (below 1e-250: both below it), NaNs in the same places; rows of cohorts outside [0, C) among the rows
  3  width 1 = engine.sparse_tile_test bit for bit; aligned full windows at (binsize 7, m = 3) = the pt bits of the sparse tile at 21
  4  chunks of 1, 7, 64 windows and one chunk, host arrays and device tensors, two calls: equal bits
  5  two regions of 10 000 positions at binsize 1 (T = 10 000), widths 7 and 1 024: N runs and mutated tiles on both sides of every
     256-tile chunk border of the window census, a run of 300 equal keys across a wave and a workgroup
  6  nb_model_window_hits_sparse against nb_model_window_hits; fdr refused before a window is tested; the command line in a child
Pi and EXP agree with the dense window route to 1e-12 relative, not in bits (one division here, a sum of quotients there); PVAL and
QVAL to 1e-6 relative (the project's pin for p-values)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from conftest import ROOT
import sparse_tiles_cases as P
import sparse_windows_statement as S
import tile_samples_cases as K
import tile_windows_cases as W

pytestmark = pytest.mark.gpu

NEAR = 2e-6              # a dense value this close to its cut could fall on either side in the other route
EXACT = ["CHROM", "POS", "OBS", "MU", "SIGMA", "REGION", "WIDTH", "PEAK"]
NAMES = ("cohort", "region", "window", "k", "pt", "exp", "pval")
SHORT_REGION = 3         # 1:1850-2250 in both problems: cut off at the contig's end


def _host(d):
    return {n: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for n, v in d.items()}


def _bits(x):
    x = x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    return x.dtype.str, x.shape, x.tobytes()


def _close_pvals(got, want, what=""):
    """The project's tolerance contract: NaNs in the same places, 1e-6 relative at or above 1e-250, below it both sides below it."""
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    big = ~np.isnan(want) & (want >= 1e-250)
    np.testing.assert_allclose(got[big], want[big], rtol=1e-6, atol=0, err_msg=str(what))
    small = ~np.isnan(want) & (want < 1e-250)
    assert (got[small] < 1.0001e-250).all(), what


@functools.lru_cache(maxsize=None)
def _genome():
    from digdriver_amd.data_tools.genome import PackedGenome
    return PackedGenome.from_sequences(K.genome_sequences())


@functools.lru_cache(maxsize=None)
def _problem(C):
    """C = 3: the regions, rows and rates of tile_samples_cases; else those of sparse_tiles_cases."""
    if C == 3:
        rows = [[r[:3] for r in rows] for rows in K.cohort_rows()]
        mu, sigma = K.mu_sigma()
        idx = K.IDX
    else:
        rows, (mu, sigma), idx = P.cohort_rows(C), P.mu_sigma(C), P.IDX
    return dict(idx=idx, rows=rows, frames=P.frames(rows), d_prs=[(K.s_prob if C == 3 else P.s_prob)(c) for c in range(C)], mu=mu, sigma=sigma,
                st=P.stacked(rows), chroms=[str(c) for c in idx[:, 0]], regions=P.regions(idx))


@functools.lru_cache(maxsize=None)
def _setup(C, n_up, binsize):
    """The dense front half, the census and the sparse scan of one problem (device tensors), the tables of the statement."""
    from digdriver_amd import engine
    prob = _problem(C)
    tables = [P.s_prob(c, n_up) for c in range(C)]
    s_prob = np.array([[t[k] for k in sorted(t)] for t in tables])
    st, idx = prob["st"], prob["idx"]                                      # (with two rows of cohorts C and -1)
    a = (_genome(), prob["chroms"], idx[:, 1], idx[:, 2], s_prob)
    rows = (st["chrom"], st["start"], st["end"], st["cohort"])
    dense = engine.tiled_nb_model(*a, prob["mu"], prob["sigma"], *rows, binsize=binsize)
    T = int(dense["pt"].shape[2])
    first, nval, denom, npos = engine.tile_census(*a, binsize)
    scan = engine.sparse_window_test(*a, binsize, T, first, nval, denom, prob["mu"], prob["sigma"], *rows)
    return dict(prob, a=a, rows_st=rows, tables=tables, s_prob=s_prob, dense=dense, T=T, census=(first, nval, denom, npos), scan=scan)


def _widths(su):
    T, short = su["T"], int(su["census"][1][SHORT_REGION])
    return [1, 2, 3, T, T + 1, short + 1]


@functools.lru_cache(maxsize=None)
def _dense_windows(C, n_up, binsize, width):
    from digdriver_amd import engine
    su = _setup(C, n_up, binsize)
    d = su["dense"]
    return _host(engine.tile_window_test(d["pt"], d["k"], su["mu"], su["sigma"], d["n_valid"], width))


@functools.lru_cache(maxsize=None)
def _positive_tiles(C, n_up, binsize):
    su = _setup(C, n_up, binsize)
    return S.positive_tiles(K.genome_sequences(), su["regions"], su["tables"], n_up, binsize, su["T"])


SHAPES = [(C, n_up, b) for C in (3, 4, 65) for n_up in (1, 2) for b in P.BINSIZES]


# ---- 1: the window census ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,n_up,binsize", SHAPES)
def test_window_census_equals_the_dense_planes_and_the_statement(C, n_up, binsize):
    import torch
    from digdriver_amd import engine
    su = _setup(C, n_up, binsize)
    first, nval, denom, npos = su["census"]
    positive, s_nval = _positive_tiles(C, n_up, binsize)
    assert s_nval == nval.tolist()
    some = (npos.cpu().numpy() > 0) & (npos.cpu().numpy() < nval.cpu().numpy()[None, :])
    assert some.any() or C == 3                       # a region with some, not all, tiles positive: the shortcut does not take it
    for m in _widths(su):
        dense = _dense_windows(C, n_up, binsize, m)
        by_census = engine.tile_window_census(*su["a"], binsize, m, n_tiles=su["T"], n_positive=npos)
        by_walk = engine.tile_window_census(*su["a"], binsize, m, n_tiles=su["T"])
        assert all(t.is_cuda and t.dtype == torch.int32 for t in by_census + by_walk)
        assert _bits(by_census[0]) == _bits(by_walk[0]) == _bits(dense["n_windows"])
        assert _bits(by_census[1]) == _bits(by_walk[1]) and by_walk[1].shape == (C, len(su["idx"]))
        inside = np.arange(su["T"])[None, None, :] < dense["n_windows"][None, :, None]
        got = by_walk[1].cpu().numpy()
        assert np.array_equal(got, ((dense["pt"] > 0) & inside).sum(axis=2))
        want = [[S.positive_windows_runs(positive[c][r], s_nval[r], m) for r in range(len(s_nval))] for c in range(C)]
        if C <= 4:
            assert want == [[S.positive_windows_brute(positive[c][r], s_nval[r], m) for r in range(len(s_nval))] for c in range(C)]
        assert got.tolist() == want
        if m == 1:
            assert np.array_equal(got, npos.cpu().numpy())
    host = engine.tile_window_census(*su["a"], binsize, 3, n_tiles=su["T"], on_device=False)
    assert all(isinstance(h, np.ndarray) for h in host)
    assert [_bits(h) for h in host] == [_bits(t) for t in engine.tile_window_census(*su["a"], binsize, 3, n_tiles=su["T"])]


# ---- 2: the candidate windows --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,n_up,binsize", SHAPES)
def test_mutated_windows_equal_the_dense_window_planes(C, n_up, binsize):
    su = _setup(C, n_up, binsize)
    seen_nan = seen_zero = 0
    for m in _widths(su):
        got = _host(su["scan"].windows(m))
        dense = _dense_windows(C, n_up, binsize, m)
        inside = np.arange(su["T"])[None, None, :] < dense["n_windows"][None, :, None]
        want = np.argwhere((dense["k"] >= 1) & inside)                      # cohort-major, then region, then window: each once
        at = np.stack([got[n].astype(np.int64) for n in NAMES[:3]], axis=1)
        assert np.array_equal(at, want), (m, len(at), len(want))
        sel = tuple(want.T)
        assert np.array_equal(got["k"], dense["k"][sel]) and got["k"].dtype == np.int32
        np.testing.assert_allclose(got["pt"], dense["pt"][sel], rtol=1e-12, atol=0, equal_nan=True)
        np.testing.assert_allclose(got["exp"], dense["exp"][sel], rtol=1e-12, atol=0, equal_nan=True)
        _close_pvals(got["pval"], dense["pval"][sel], (C, n_up, binsize, m))
        seen_nan += int(np.isnan(got["pval"]).sum())
        seen_zero += int(((got["pt"] == 0) & (got["pval"] == 0)).sum())
        assert len(want) > 0 and (m > 1 or got["k"].max() >= 70)
    assert C == 3 or (seen_nan > 0 and seen_zero > 0)                       # rows in regions without a test; rows on N windows


@pytest.mark.parametrize("C,n_up,binsize,width", [(4, 1, 7, 2), (4, 2, 50, 3), (3, 1, 1, 3), (4, 1, 1, 401)])
def test_mutated_windows_equal_the_statement(C, n_up, binsize, width):
    su = _setup(C, n_up, binsize)
    got = _host(su["scan"].windows(width))
    ref = S.mutated_window_table(K.genome_sequences(), su["regions"], P.statement_rows(su["st"]), su["tables"], n_up, binsize, su["T"], width)
    wins = [tuple(int(got[n][i]) for n in NAMES[:3]) for i in range(len(got["k"]))]
    assert wins == sorted(ref) and got["k"].tolist() == [ref[w][0] for w in wins]
    np.testing.assert_allclose(got["pt"], np.array([ref[w][1] for w in wins]), rtol=1e-12, atol=0, equal_nan=True)


# ---- 3: width 1 and aligned windows --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,n_up,binsize", [(3, 1, 1), (4, 2, 7), (65, 1, 50)])
def test_width_one_is_the_sparse_tile_test_bit_for_bit(C, n_up, binsize):
    from digdriver_amd import engine
    su = _setup(C, n_up, binsize)
    first, nval, denom, _ = su["census"]
    tiles = engine.sparse_tile_test(*su["a"], binsize, su["T"], first, nval, denom, su["mu"], su["sigma"], *su["rows_st"])
    got = su["scan"].windows(1)
    assert len(got["k"]) > 100 or binsize == 50
    for name in NAMES:
        assert _bits(got[name]) == _bits(tiles["tile" if name == "window" else name]), name


@pytest.mark.parametrize("C,n_up", [(3, 1), (4, 2)])
def test_aligned_full_windows_have_the_pt_bits_of_the_wider_sparse_tile(C, n_up):
    from digdriver_amd import engine
    su = _setup(C, n_up, 7)
    got = _host(su["scan"].windows(3))
    first, nval, denom, _ = engine.tile_census(*su["a"], 21)
    T21 = -(-su["T"] * 7 // 21)
    wide = _host(engine.sparse_tile_test(*su["a"], 21, T21, first, nval, denom, su["mu"], su["sigma"], *su["rows_st"]))
    assert _bits(denom) == _bits(su["census"][2])                           # (the denominators do not depend on the bin size)
    nv7 = su["census"][1].cpu().numpy()
    tile_at = {(int(c), int(r), int(t)): i for i, (c, r, t) in enumerate(zip(wide["cohort"], wide["region"], wide["tile"]))}
    compared = 0
    for i, (c, r, w) in enumerate(zip(got["cohort"], got["region"], got["window"])):
        j = tile_at.get((int(c), int(r), int(w) // 3))
        if w % 3 == 0 and w + 3 <= nv7[r] and j is not None:
            assert got["pt"][i].tobytes() == wide["pt"][j].tobytes() and got["k"][i] == wide["k"][j], (c, r, w)
            compared += 1
    assert compared >= 20


# ---- 4: chunks, forms of input, determinism ------------------------------------------------------------------------------------
def test_chunks_of_any_size_give_equal_bits():
    su = _setup(4, 1, 50)
    for m in (1, 3):
        whole = su["scan"].windows(m)
        assert 64 < len(whole["k"]) < 2000
        for chunk in (1, 7, 64):
            parts = list(su["scan"].chunks(m, chunk))
            assert len(parts) == -(-len(whole["k"]) // chunk) and all(len(p["k"]) <= chunk for p in parts)
            assert {n: _bits(v) for n, v in su["scan"].windows(m, chunk).items()} == {n: _bits(v) for n, v in whole.items()}, (m, chunk)
    with pytest.raises(ValueError, match="chunk_windows"):
        list(su["scan"].chunks(2, 0))


@pytest.mark.parametrize("n_up,binsize,width", [(1, 1, 2), (2, 50, 3), (1, 7, 59)])
def test_host_arrays_and_device_tensors_give_the_same_bits_and_two_calls_too(n_up, binsize, width):
    from digdriver_amd import engine
    su = _setup(4, n_up, binsize)
    dev = su["scan"].windows(width)
    again = su["scan"].windows(width)
    assert {n: _bits(v) for n, v in dev.items()} == {n: _bits(v) for n, v in again.items()}
    census = [t.cpu().numpy() for t in su["census"]]
    host_scan = engine.sparse_window_test(*su["a"], binsize, su["T"], census[0], census[1], census[2], su["mu"], su["sigma"], *su["rows_st"])
    host = host_scan.windows(width)
    assert all(isinstance(v, np.ndarray) for v in host.values()) and len(host["k"]) > 20
    assert {n: _bits(v) for n, v in dev.items()} == {n: _bits(v) for n, v in host.items()}
    off_dev, total_dev = su["scan"].offsets(width)
    off_host, total_host = host_scan.offsets(width)
    assert total_dev == total_host == len(host["k"]) and _bits(off_dev) == _bits(off_host) and off_host.dtype == np.int64
    assert len(off_host) == len(host_scan.keys) + 1 and off_host[0] == 0 and off_host[-1] == total_host


# ---- 5: rows of 10 000 tiles ---------------------------------------------------------------------------------------------------
CENSUS_CHUNK = 256                                                         # tiles per step of tile_window_census_kernel
LONG_N_RUNS = [(40, 70), (240, 300), (500, 1300), (2040, 2060), (3000, 4100), (9000, 9999)]      # tiles of region 0 (positions - 50)


@functools.lru_cache(maxsize=None)
def _long():
    import torch
    from digdriver_amd import engine
    from digdriver_amd.data_tools.genome import PackedGenome
    from digdriver_amd.sequence_model import nb_model
    seqs = {n: list(s) for n, s in W.long_genome_sequences().items()}
    for name, first in (("1", 50), ("2", 40)):
        for a, b in LONG_N_RUNS:
            seqs[name][first + a:first + b] = "N" * (b - a)
    seqs = {n: "".join(s) for n, s in seqs.items()}
    g = PackedGenome.from_sequences(seqs)
    tables = [W.long_s_prob(0), dict(W.long_s_prob(1))]
    for i, k in enumerate(sorted(tables[1])):                               # cohort 1: a quarter of the contexts has S_prob 0
        if i % 4 == 1:
            tables[1][k] = 0.0
    s_prob = np.stack([nb_model._s_prob_table(t, 1) for t in tables])
    mu, sigma = W.long_mu_sigma()
    chrom, start, cohort = [], [], []
    borders = np.arange(CENSUS_CHUNK, W.LONG_T - 60, CENSUS_CHUNK)
    for c in range(W.LONG_C):
        rng = np.random.default_rng(41 + c)
        for ch, first, _ in W.LONG_IDX:
            at = np.concatenate([borders - 1, borders, rng.integers(0, W.LONG_T - 60, 40), np.full(300 if c == 0 else 1, 777)])
            chrom += [str(ch)] * len(at)
            start += list(first + at)
            cohort += [c] * len(at)
    start = np.array(start, np.int64)
    a = (g, [str(c) for c in W.LONG_IDX[:, 0]], W.LONG_IDX[:, 1], W.LONG_IDX[:, 2], s_prob)
    up = lambda x: torch.as_tensor(x, device="cuda:0")
    rows = (np.array(chrom), up(start), up(start + 1), up(np.array(cohort, np.int32)))
    dense = engine.tiled_nb_model(*a, mu, sigma, *rows, binsize=1)
    first, nval, denom, npos = engine.tile_census(*a, 1)
    assert dense["pt"].shape == (W.LONG_C, 2, W.LONG_T) and nval.tolist() == [10000, 9950]
    scan = engine.sparse_window_test(*a, 1, W.LONG_T, first, nval, denom, mu, sigma, *rows)
    return dict(a=a, dense=dense, census=(first, nval, denom, npos), scan=scan, mu=mu, sigma=sigma)


@pytest.mark.parametrize("width", W.LONG_WIDTHS)
def test_rows_of_ten_thousand_tiles(width):
    from digdriver_amd import engine
    L = _long()
    d = L["dense"]
    dense = _host(engine.tile_window_test(d["pt"], d["k"], L["mu"], L["sigma"], d["n_valid"], width))
    npos = L["census"][3]
    by_census = engine.tile_window_census(*L["a"], 1, width, n_tiles=W.LONG_T, n_positive=npos)
    by_walk = engine.tile_window_census(*L["a"], 1, width, n_tiles=W.LONG_T)
    assert _bits(by_census[0]) == _bits(by_walk[0]) == _bits(dense["n_windows"]) and _bits(by_census[1]) == _bits(by_walk[1])
    inside = np.arange(W.LONG_T)[None, None, :] < dense["n_windows"][None, :, None]
    want_pos = ((dense["pt"] > 0) & inside).sum(axis=2)
    assert np.array_equal(by_walk[1].cpu().numpy(), want_pos)
    assert (want_pos < dense["n_windows"][None, :]).all() and (want_pos > 0).all()          # windows inside the N runs, and others
    # runs of tiles without a positive position lie across the census' chunk borders 256, 512 .. 1280, 3072 .. 4096 and 9216 ..
    zero = ~(d["pt"][0, 0].cpu().numpy() > 0)
    assert all(zero[b - 1] and zero[b] for b in (256, 512, 768, 1024, 1280, 3072, 4096, 9216, 9728)) and not zero[2000] and zero[2048]
    got = _host(L["scan"].windows(width, 1 << 12))
    want = np.argwhere((dense["k"] >= 1) & inside)
    assert np.array_equal(np.stack([got[n].astype(np.int64) for n in NAMES[:3]], axis=1), want)
    sel = tuple(want.T)
    assert np.array_equal(got["k"], dense["k"][sel]) and got["k"].max() >= 300
    np.testing.assert_allclose(got["pt"], dense["pt"][sel], rtol=1e-12, atol=0, equal_nan=True)
    np.testing.assert_allclose(got["exp"], dense["exp"][sel], rtol=1e-12, atol=0, equal_nan=True)
    _close_pvals(got["pval"], dense["pval"][sel], width)
    k0 = d["k"][0, 0].cpu().numpy()
    assert all(k0[b - 1] >= 1 and k0[b] >= 1 for b in range(CENSUS_CHUNK, W.LONG_T - 60, CENSUS_CHUNK))      # both sides of every border


# ---- 6: the function against the dense window route ----------------------------------------------------------------------------
def _call(fn, which, binsize, **kw):
    prob = _problem(which)
    return fn(prob["d_prs"], prob["idx"], prob["mu"], prob["sigma"], prob["frames"], _genome(), n_up=1, n_down=1, binsize=binsize, **kw)


@functools.lru_cache(maxsize=None)
def _dense_frames(which, binsize, width, pval_max=None, fdr=None):
    """nb_model_window_hits at one width, computed once per cut and left unchanged."""
    from digdriver_amd.sequence_model import nb_model
    kw = dict(pval_max=pval_max) if fdr is None else dict(fdr=fdr)
    return _call(nb_model.nb_model_window_hits, which, binsize, widths=(width,), **kw)


def _dense_cut(which, binsize, width, kind, level):
    """The dense frames under the cut; bonferroni: the dense route has no such keyword, its cut is pval_max = level / n_testable."""
    if kind != "bonferroni":
        return _dense_frames(which, binsize, width, **{kind: level})
    n_test = [f.attrs["n_testable"][0] for f in _dense_frames(which, binsize, width, pval_max=2.0)]
    return [_dense_frames(which, binsize, width, pval_max=level / max(n, 1))[c] for c, n in enumerate(n_test)]


def _assert_no_value_near_the_cut(which, binsize, width, kind, level):
    """On the DENSE results: no mutated window's PVAL (for fdr: no QVAL of the whole list) within 2e-6 relative of the cut."""
    from digdriver_amd.sequence_model import nb_model
    for c, f in enumerate(_dense_frames(which, binsize, width, pval_max=2.0)):
        n = f.attrs["n_testable"][0]
        assert len(f) == n
        if kind == "fdr":
            x, cut = nb_model.get_q_vals(f.PVAL.values)[f.OBS.values >= 1], level
        else:
            x, cut = f.PVAL.values[f.OBS.values >= 1], level / max(n, 1) if kind == "bonferroni" else level
        assert not (np.abs(x - cut) <= NEAR * cut).any(), (which, binsize, width, kind, c)


def _mutated_only(frame, width):
    """The dense hits of one width with OBS >= 1, PEAK made again on them (index differences inside a region are tile differences)."""
    from digdriver_amd.sequence_model import nb_model
    f = frame[frame.OBS >= 1].copy()
    region = pd.factorize(f.REGION)[0]
    f["PEAK"] = nb_model.window_peaks(region, f.index.values, f.PVAL.values, width)
    return f


def _assert_frames_equal(sp, de, fdr):
    assert list(sp.columns) == list(de.columns) and list(sp.dtypes) == list(de.dtypes)
    assert sp.index.dtype == np.int64 and np.array_equal(sp.index.values, de.index.values)
    for col in EXACT:
        a, b = sp[col].values, de[col].values
        assert np.array_equal(a, b) if col in ("REGION", "PEAK") else np.array_equal(a, b, equal_nan=True), col
    for col, tol in (("Pi", 1e-12), ("EXP", 1e-12), ("PVAL", 1e-6)) + ((("QVAL", 1e-6),) if fdr else ()):
        np.testing.assert_allclose(sp[col].values, de[col].values, rtol=tol, atol=0, err_msg=col)


def _compare(which, binsize, widths, kind, level, certified):
    from digdriver_amd.sequence_model import nb_model
    for m in widths:
        _assert_no_value_near_the_cut(which, binsize, m, kind, level)
    sparse = _call(nb_model.nb_model_window_hits_sparse, which, binsize, widths=widths, **{kind: level})
    dense = [_dense_cut(which, binsize, m, kind, level) for m in widths]
    assert len(sparse) == len(dense[0])
    for c, sp in enumerate(sparse):
        blocks = []
        for j, m in enumerate(widths):
            de = dense[j][c]
            if kind == "bonferroni":
                de = de.drop(columns="QVAL", errors="ignore")
            if sp.attrs["complete"][j]:
                assert (de.OBS >= 1).all()                                  # the certificate: no empty window is a dense hit
            else:
                de = _mutated_only(de, m)
            blocks.append(de)
            assert sp.attrs["n_testable"][j] == dense[j][c].attrs["n_testable"][0], (c, m)
            assert sp.attrs["n_windows"][j] == dense[j][c].attrs["n_windows"][0], (c, m)
        _assert_frames_equal(sp, pd.concat(blocks), kind == "fdr")
        assert len(sp.attrs["zero_floor"]) == len(sp.attrs["complete"]) == len(widths)
        if certified is not None:
            assert sp.attrs["complete"] == [certified] * len(widths), (c, sp.attrs)
    return sparse


@pytest.mark.parametrize("kind,level", [("pval_max", 0.05), ("fdr", 0.1), ("bonferroni", 0.05)])
def test_certified_scan_equals_the_dense_window_route(kind, level):
    """tile_samples_cases at binsize 1, widths 2 and 3: every cohort certified at every width, the frames are the dense ones."""
    sparse = _compare(3, 1, (2, 3), kind, level, True)
    assert sum(len(f) for f in sparse) > 0 and all(f.attrs["zero_floor"][0] > f.attrs["zero_floor"][1] > level for f in sparse)


@pytest.mark.parametrize("which", [3, 4])
def test_uncertified_scan_is_the_dense_hits_with_a_row(which):
    """binsize 50: no cohort is certified, the frames are the dense hits with OBS >= 1 and say so."""
    sparse = _compare(which, 50, (1, 3), "pval_max", 1e-3, False)
    assert sum(len(f) for f in sparse) > 0


@pytest.mark.parametrize("C", [4, 65])
def test_new_cases_at_binsize_one_certified_but_for_the_depleted_cohort(C):
    """sparse_tiles_cases at binsize 1, widths 2 and 3, pval_max 0.01: the floors of cohorts 0 .. 2 are 0.057, 0.086, 0.147 at width 2
    and 0.016, 0.029, 0.061 at width 3 -- certified; the depleted cohort's are 0.041 and 0.0085: certified at width 2 only."""
    sparse = _compare(C, 1, (2, 3), "pval_max", 0.01, None)
    assert [f.attrs["complete"] for f in sparse[:4]] == [[True, True]] * 3 + [[True, False]]
    assert [round(f.attrs["zero_floor"][1], 4) for f in sparse[:4]] == [0.0163, 0.0289, 0.0609, 0.0085]
    assert all(f.attrs["complete"] == [True, True] for f in sparse[4:])
    n_rows = sparse[0][(sparse[0].Pi == 0) & (sparse[0].PVAL == 0)]
    assert len(n_rows) > 0 and (n_rows.OBS >= 1).all()                      # rows on windows of N only: Pi = 0, PVAL = 0


def test_empty_windows_of_the_depleted_cohort_are_dense_hits_the_sparse_frame_leaves_out():
    """The same problem at pval_max 0.1: an empty window of three tiles of the depleted cohort's region has PVAL about 0.05."""
    sparse = _compare(4, 1, (2, 3), "pval_max", 0.1, None)
    dense = _dense_frames(4, 1, 3, pval_max=0.1)[P.DEPLETED]
    assert (dense.OBS == 0).sum() >= 3 and set(dense[dense.OBS == 0].REGION) == {"1:1500-1900"}
    assert sparse[P.DEPLETED].attrs["complete"] == [False, False] and len(sparse[P.DEPLETED]) < len(dense)
    assert sum(len(f) for f in sparse) > 0


def test_fdr_on_an_uncertified_width_raises_before_a_window_is_tested(monkeypatch):
    from digdriver_amd import _lib
    from digdriver_amd.sequence_model import nb_model
    called = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    with pytest.raises(ValueError, match=r"no certificate that an empty window is no hit for cohorts \[3\] at widths \[3\]") as exc:
        _call(nb_model.nb_model_window_hits_sparse, 4, 1, widths=(1, 2, 3), fdr=0.01)
    assert "fdr = 0.01" in str(exc.value) and "zero-window floors ['0.00853']" in str(exc.value)
    assert "dig_tile_window_census" in called and "dig_sparse_window_test" not in called and "dig_sparse_tile_keys" not in called


def test_tile_driver_sparse_windows_in_a_fresh_child_process(tmp_path):
    """`DigDriver.py tileDriver --sparse --sparse-windows 1 3` in a child process of its own writes nb_model_window_hits_sparse's
    frames and says where the scan is incomplete; `--sparse` alone writes the bytes of nb_model_hits_sparse, as before."""
    from digdriver_amd.io import mapfile
    from digdriver_amd.sequence_model import nb_model
    C = 4
    prob = _problem(C)
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
        ["--binsize", "50", "--outpfx", "A", "B", "C", "D", "--pval-max", "1e-3", "--sparse"]
    runs = [subprocess.Popen(head + ["--outdir", str(tmp_path / "windows"), "--sparse-windows", "1", "3"], stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True),
            subprocess.Popen(head + ["--outdir", str(tmp_path / "tiles")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)]
    said = []
    for run in runs:
        out, _ = run.communicate(timeout=300)
        assert run.returncode == 0, out
        said.append(out)
    assert said[0].count("(mutated windows only)") == 2 * C and "zero-window floors" in said[0] and "widths [1, 3]" in said[0]
    assert "zero-window" not in said[1] and said[1].count("(mutated tiles only)") == C
    windows = _call(nb_model.nb_model_window_hits_sparse, C, 50, widths=(1, 3), pval_max=1e-3)
    tiles = _call(nb_model.nb_model_hits_sparse, C, 50, pval_max=1e-3)
    for pfx, win, til in zip("ABCD", windows, tiles):
        for sub, frame in (("windows", win), ("tiles", til)):
            want = tmp_path / ("want_%s_%s.txt" % (sub, pfx))
            mapfile.write_results_tsv(frame, str(want))
            assert (tmp_path / sub / (pfx + ".hits.txt")).read_bytes() == want.read_bytes(), (sub, pfx)
    assert sum(len(f) for f in windows) > 0
