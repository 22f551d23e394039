"""Sliding windows in the per-base route on the GPU (dig_tile_window_test behind engine.tile_window_test, nb_model.nb_model_window_hits,
`DigDriver.py tileDriver --window-tiles`) on the problems of tile_windows_cases.py.
  1  pt_w, k_w, n_windows of the device entry point and of the `_host` twin equal the plain-Python statement bit for bit, tails included
  2  pval_w, exp_w are dig_tiled_nb_test on the returned pt_w, k_w, bit for bit; at width 1 all four planes are the existing route's
  3  windows t = j m against tile j of the existing route at bin size m binsize: k exact, pt to 1e-12, pval and exp to 1e-6 relative
     (the project's parity bounds: README, nb_model.ZERO_FLOOR_MARGIN; the two sides add a tile's positions in different orders)
  4  rows longer than a workgroup's chunk (T = 10 000, widths 7 and 1 024), windows with k_w > 0 across every chunk border, exact
  5  nb_model_window_hits column by column against what the statement selects from the full planes, against nb_model_hits at
     widths=[1], with a cap and a filter against host-thinned rows; tileDriver in fresh child processes
tile_window_kernel is no template and its grid is not capped (one workgroup per run of 1 024 outputs): there is one compiled form
and no grid-stride pass.  Its two paths -- whole rows per workgroup (T <= 1 024) and chunks of one row with a halo (T > 1 024) -- are
taken by the small and the long problem."""
import functools
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from conftest import ROOT
import tile_samples_cases as K
import tile_samples_statement as SS
import tile_windows_cases as W
import tile_windows_statement as S

pytestmark = pytest.mark.gpu

PVAL_MAX, FDR = 1e-3, 0.1
PLANES = ("pt", "k", "exp", "pval")


def _bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        word = np.uint64 if got.dtype.itemsize == 8 else np.uint32
        at = np.argwhere(got.view(word) != want.view(word))
        raise AssertionError("%s: %d elements differ, first at %s: %r against %r" % (what, len(at), at[0], got[tuple(at[0])], want[tuple(at[0])]))


def _host(d):
    return {n: (v.cpu().numpy() if hasattr(v, "cpu") else v) for n, v in d.items()}


@functools.lru_cache(maxsize=None)
def _problem():
    from digdriver_amd.data_tools.genome import PackedGenome
    rows = K.cohort_rows()
    mu, sigma = K.mu_sigma()
    return dict(genome=PackedGenome.from_sequences(K.genome_sequences()), rows=rows, frames=K.frames(rows), st=K.stacked(rows),
                d_prs=[K.s_prob(c) for c in range(K.C)], mu=mu, sigma=sigma, chroms=[str(c) for c in K.IDX[:, 0]])


@functools.lru_cache(maxsize=None)
def _base(binsize):
    """The existing route's result on the small problem (device tensors: pval, exp, pt, k, first_pos, n_valid) and host copies."""
    import torch
    from digdriver_amd import engine
    from digdriver_amd.sequence_model import nb_model
    P = _problem()
    st = P["st"]
    s_prob = np.stack([nb_model._s_prob_table(d, 1) for d in P["d_prs"]])
    up = lambda x: torch.as_tensor(x, device="cuda:0")
    dev = engine.tiled_nb_model(P["genome"], P["chroms"], K.IDX[:, 1], K.IDX[:, 2], s_prob, P["mu"], P["sigma"], st["chrom"], up(st["start"]),
                                up(st["end"]), up(st["cohort"]), binsize=binsize)
    host = _host(dev)
    T = -(-400 // binsize)
    assert host["pt"].shape == (K.C, 6, T)
    assert list(host["n_valid"][:5]) == [T, -(-350 // binsize), T, W.SHORT_TILES[binsize], T] and host["n_valid"][5] <= 0
    return dev, host, T


@functools.lru_cache(maxsize=None)
def _windows(binsize, width, device=True):
    """engine.tile_window_test on the base planes: device tensors in (the device entry point) or host arrays in (the twin); host arrays out."""
    from digdriver_amd import engine
    P = _problem()
    dev, host, _ = _base(binsize)
    src = dev if device else host
    got = engine.tile_window_test(src["pt"], src["k"], P["mu"], P["sigma"], src["n_valid"], width)
    if device:
        assert all(v.is_cuda for v in got.values())
    else:
        assert all(isinstance(v, np.ndarray) for v in got.values())
    return _host(got)


CASES = [(b, m) for b in K.BINSIZES for m in W.widths(b)]


# ---- 1: the sums against the statement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binsize,width", CASES)
def test_sums_and_window_counts_equal_the_statement_bit_for_bit(binsize, width):
    _, host, T = _base(binsize)
    want_pt, want_k, want_n = S.window_planes(host["pt"], host["k"], host["n_valid"], width)
    for device in (True, False):
        got = _windows(binsize, width, device)
        _bits(got["n_windows"], want_n, (device, "n_windows"))
        _bits(got["k"], want_k, (device, "k_w"))
        _bits(got["pt"], want_pt, (device, "pt_w"))
    # what the problem was built to hold: a region without tiles, one that is cut short, and windows that hold rows
    nv = np.clip(host["n_valid"], 0, T)
    assert want_n[5] == 0 and list(want_n[:5]) == [max(v - width + 1, 1) for v in nv[:5]]
    assert want_k[0, 0].sum() >= host["k"][0, 0].sum() and np.isnan(want_pt[:, 5]).all() and not want_k[:, 5].any()
    if width == W.SHORT_TILES[binsize] + 1:
        assert want_n[3] == 1 and want_k[0, 3, 0] == host["k"][0, 3].sum() > 0 and want_n[0] > 1


# ---- 2: the test itself ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binsize,width", CASES)
def test_pval_and_exp_are_the_tiled_nb_test_of_the_returned_sums(binsize, width):
    import torch
    from digdriver_amd import engine
    P = _problem()
    got = _windows(binsize, width)
    pval, ex = engine.tiled_nb_test(torch.as_tensor(got["pt"], device="cuda:0"), torch.as_tensor(got["k"], device="cuda:0"),
                                    torch.as_tensor(P["mu"], device="cuda:0"), torch.as_tensor(P["sigma"], device="cuda:0"))
    _bits(got["pval"], pval.cpu().numpy(), "pval_w")
    _bits(got["exp"], ex.cpu().numpy(), "exp_w")
    twin = _windows(binsize, width, False)
    _bits(twin["pval"], got["pval"], "pval_w of the twin")
    _bits(twin["exp"], got["exp"], "exp_w of the twin")
    n = got["n_windows"]
    inside = np.arange(got["pval"].shape[2])[None, :] < n[:, None]
    assert np.isnan(got["pval"][:, ~inside]).all() and np.isnan(got["exp"][:, ~inside]).all()
    assert np.isfinite(got["pval"][:, inside]).sum() > 0


@pytest.mark.parametrize("binsize", K.BINSIZES)
def test_width_one_gives_the_planes_of_the_existing_route(binsize):
    _, host, _ = _base(binsize)
    for device in (True, False):
        got = _windows(binsize, 1, device)
        for name in PLANES:
            _bits(got[name], host[name], (device, name))
        _bits(got["n_windows"], np.maximum(host["n_valid"], 0).astype(np.int32), (device, "n_windows"))


# ---- 3: against the existing route at another bin size --------------------------------------------------------------------------
@pytest.mark.parametrize("binsize,width", [(50, 2), (50, 4), (1, 50), (1, 150)])
def test_aligned_windows_are_the_tiles_of_a_wider_bin_size(binsize, width):
    """The rows of the problem that lie inside region 3's interval but behind its last tile of the NARROW grid (S4 at 1:2020 on a
    contig of 2 000 bases; at bin size 1 also the rows that start on the contig's last base, which has no window and so is no
    position) are left out of the wider grid's rows: dig_tile_mut_counts skips a row by its TILE (at or past n_valid), so the narrow
    grid counts them nowhere, while a wider grid whose clipped last tile nominally reaches them counts them there.  That is the
    existing route's rule and no window can undo it; the end of the test pins it: on the full rows the wider grid differs from the
    one compared here by exactly those rows, in the tiles that hold them, and nowhere else."""
    _, small, _ = _base(binsize)
    wide = _wide(binsize * width, binsize)
    got = _windows(binsize, width)
    compared = short = 0
    for r in range(len(K.IDX)):
        nv = int(max(small["n_valid"][r], 0))
        tiles = [(j * width, j) for j in range(nv // width)] or ([(0, 0)] if nv > 0 else [])
        short += 0 < nv < width
        for t, j in tiles:
            assert j < wide["n_valid"][r]
            for c in range(K.C):
                assert got["k"][c, r, t] == wide["k"][c, r, j], (c, r, t)
                np.testing.assert_allclose(got["pt"][c, r, t], wide["pt"][c, r, j], rtol=1e-12, atol=0, equal_nan=True)
                np.testing.assert_allclose(got["pval"][c, r, t], wide["pval"][c, r, j], rtol=1e-6, atol=0, equal_nan=True)
                np.testing.assert_allclose(got["exp"][c, r, t], wide["exp"][c, r, j], rtol=1e-6, atol=0, equal_nan=True)
                compared += 1
    assert compared >= 3 * 5 and (short > 0) == (width in (4, 150))
    st = _problem()["st"]
    want_extra = np.zeros_like(wide["k"])
    for i in np.flatnonzero(_behind_region_3(binsize)):
        its_tile = (st["start"][i] - 1850) // (binsize * width)          # of the wider grid: it exists when the grid's last tile reaches that far
        if its_tile < wide["n_valid"][3]:
            want_extra[st["cohort"][i], 3, its_tile] += 1
    assert np.array_equal(_wide(binsize * width, None)["k"] - wide["k"], want_extra)
    assert want_extra.sum() > 0 and _behind_region_3(binsize).sum() >= 1


def _behind_region_3(binsize):
    """The rows that start inside region 3's interval at or behind the end of its last tile at this bin size."""
    st = _problem()["st"]
    _, host, _ = _base(binsize)
    return (st["chrom"] == "1") & (st["start"] >= 1850 + int(host["n_valid"][3]) * binsize) & (st["start"] < 2250)


@functools.lru_cache(maxsize=None)
def _wide(binsize, narrow):
    """The existing route on the small problem at any bin size (host arrays); narrow: without the rows behind region 3's last tile at
    that bin size (None: all rows)."""
    import torch
    from digdriver_amd import engine
    from digdriver_amd.sequence_model import nb_model
    P = _problem()
    st = P["st"]
    stay = np.ones(len(st["start"]), bool) if narrow is None else ~_behind_region_3(narrow)
    s_prob = np.stack([nb_model._s_prob_table(d, 1) for d in P["d_prs"]])
    up = lambda x: torch.as_tensor(x[stay], device="cuda:0")
    return _host(engine.tiled_nb_model(P["genome"], P["chroms"], K.IDX[:, 1], K.IDX[:, 2], s_prob, P["mu"], P["sigma"], st["chrom"][stay],
                                       up(st["start"]), up(st["end"]), up(st["cohort"]), binsize=binsize))


# ---- 4: rows longer than a workgroup's chunk ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _long_base():
    import torch
    from digdriver_amd import engine
    from digdriver_amd.data_tools.genome import PackedGenome
    from digdriver_amd.sequence_model import nb_model
    g = PackedGenome.from_sequences(W.long_genome_sequences())
    rows = W.long_rows()
    s_prob = np.stack([nb_model._s_prob_table(W.long_s_prob(c), 1) for c in range(W.LONG_C)])
    mu, sigma = W.long_mu_sigma()
    up = lambda x: torch.as_tensor(x, device="cuda:0")
    chrom = np.concatenate([r[0] for r in rows])
    start, end = np.concatenate([r[1] for r in rows]), np.concatenate([r[2] for r in rows])
    cohort = np.concatenate([np.full(len(r[1]), c, np.int32) for c, r in enumerate(rows)])
    dev = engine.tiled_nb_model(g, [str(c) for c in W.LONG_IDX[:, 0]], W.LONG_IDX[:, 1], W.LONG_IDX[:, 2], s_prob, mu, sigma, chrom, up(start),
                                up(end), up(cohort), binsize=1)
    host = _host(dev)
    assert host["pt"].shape == (W.LONG_C, 2, W.LONG_T) and list(host["n_valid"]) == [10000, 9950] and W.LONG_T > W.CHUNK
    return dev, host, mu, sigma


@pytest.mark.parametrize("width", W.LONG_WIDTHS)
def test_rows_longer_than_a_chunk_equal_the_statement(width):
    import torch
    from digdriver_amd import engine
    dev, host, mu, sigma = _long_base()
    want_pt, want_k, want_n = S.window_planes(host["pt"], host["k"], host["n_valid"], width)
    for device in (True, False):
        src = dev if device else host
        got = _host(engine.tile_window_test(src["pt"], src["k"], mu, sigma, src["n_valid"], width))
        _bits(got["n_windows"], want_n, (device, "n_windows"))
        _bits(got["k"], want_k, (device, "k_w"))
        _bits(got["pt"], want_pt, (device, "pt_w"))
        if device:
            up = lambda x: torch.as_tensor(x, device="cuda:0")
            pval, ex = engine.tiled_nb_test(up(got["pt"]), up(got["k"]), up(mu), up(sigma))
            _bits(got["pval"], pval.cpu().numpy(), "pval_w")
            _bits(got["exp"], ex.cpu().numpy(), "exp_w")
    # a window that holds a row lies across every chunk border of every row: it starts in front of the border and ends behind it
    for r, nw in enumerate(want_n):
        for border in range(W.CHUNK, int(nw), W.CHUNK):
            assert want_k[0, r, border - 1] >= 2, (r, border)                       # (the rows at border - 1 and border: width >= 2)
            if width == 1024:
                # cohort 1's row in the LAST tile of the window that starts one tile in front of the border: the halo's far end
                assert host["k"][1, r, border + 1022] >= 1 and want_k[1, r, border - 1] >= 1, (r, border)
    assert list(want_n) == [10000 - width + 1, 9950 - width + 1]


def test_the_largest_width_and_one_above():
    """DIG_TILE_WINDOW_MAX_WIDTH is taken (the largest staged run: 1 024 outputs and a halo of 2 047 tiles) and one above is refused."""
    from digdriver_amd import engine
    dev, host, mu, sigma = _long_base()
    got = _host(engine.tile_window_test(dev["pt"], dev["k"], mu, sigma, dev["n_valid"], W.MAX_WIDTH, out=None))
    want_pt, want_k, want_n = S.window_planes(host["pt"], host["k"], host["n_valid"], W.MAX_WIDTH)
    _bits(got["n_windows"], want_n, "n_windows")
    _bits(got["k"], want_k, "k_w")
    _bits(got["pt"], want_pt, "pt_w")
    with pytest.raises(ValueError, match="DIG_TILE_WINDOW_MAX_WIDTH"):
        engine.tile_window_test(dev["pt"], dev["k"], mu, sigma, dev["n_valid"], W.MAX_WIDTH + 1)


def test_empty_inputs_launch_nothing_and_the_planes_are_reused():
    import torch
    from digdriver_amd import engine
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda:0")
    got = engine.tile_window_test(z(0, 3, 5), z(0, 3, 5).int(), z(0, 3), z(0, 3), torch.tensor([5, 2, 0], dtype=torch.int32, device="cuda:0"), 3)
    assert got["pt"].shape == (0, 3, 5) and list(got["n_windows"].cpu().numpy()) == [3, 1, 0]
    got = engine.tile_window_test(np.zeros((2, 0, 4)), np.zeros((2, 0, 4), np.int32), np.zeros((2, 0)), np.zeros((2, 0)), np.zeros(0, np.int32), 2)
    assert got["pval"].shape == (2, 0, 4) and got["n_windows"].shape == (0,)
    # out=: the same tensors come back, written for the new width
    P = _problem()
    dev, _, _ = _base(50)
    first = engine.tile_window_test(dev["pt"], dev["k"], P["mu"], P["sigma"], dev["n_valid"], 2)
    again = engine.tile_window_test(dev["pt"], dev["k"], P["mu"], P["sigma"], dev["n_valid"], 3, out=first)
    assert all(again[n].data_ptr() == first[n].data_ptr() for n in first)
    for n, v in _windows(50, 3).items():
        _bits(again[n].cpu().numpy(), v, n)


# ---- 5: nb_model_window_hits ----------------------------------------------------------------------------------------------------
def _call(binsize, widths, mode, frames=None, **kw):
    from digdriver_amd.sequence_model import nb_model
    P = _problem()
    cut = dict(pval_max=PVAL_MAX) if mode == "pval" else dict(fdr=FDR)
    return nb_model.nb_model_window_hits(P["d_prs"], K.IDX, P["mu"], P["sigma"], P["frames"] if frames is None else frames, P["genome"],
                                         n_up=1, n_down=1, binsize=binsize, widths=widths, **cut, **kw)


def _same_frame(got, want, what):
    assert list(got.columns) == list(want.columns), what
    assert got.index.dtype == np.int64 and list(got.index) == list(want.index), what
    assert len(got) == len(want), what
    if len(want) == 0:
        return
    pd.testing.assert_frame_equal(got, want, check_exact=True)
    for col in got.columns:
        if col not in ("REGION", "PEAK"):
            assert np.asarray(got[col], float).tobytes() == np.asarray(want[col], float).tobytes(), (what, col)


@pytest.mark.parametrize("binsize,widths", [(50, (2, 1, 4)), (1, (30, 150))])
@pytest.mark.parametrize("mode", ["pval", "fdr"])
def test_window_hits_equal_what_the_statement_selects_from_the_full_planes(binsize, widths, mode):
    from digdriver_amd.sequence_model import nb_model
    P = _problem()
    _, host, _ = _base(binsize)
    frames = _call(binsize, widths, mode)
    n_pos = nb_model._region_positions(P["genome"], P["chroms"], K.IDX[:, 2], host["first_pos"], 1)
    n_hits = n_peaks = 0
    for c, got in enumerate(frames):
        planes = [{n: (v if n == "n_windows" else v[c]) for n, v in _windows(binsize, m).items()} for m in widths]
        cols, index, attrs = S.window_hits(K.IDX, P["mu"][c], P["sigma"][c], host["first_pos"], n_pos, host["n_valid"], binsize, widths, planes,
                                           **(dict(pval_max=PVAL_MAX) if mode == "pval" else dict(fdr=FDR)))
        want = pd.DataFrame(cols, index=pd.Index(index, dtype=np.int64))[list(cols)]
        assert list(got.columns) == ["CHROM", "POS", "OBS", "EXP", "PVAL", "Pi", "MU", "SIGMA", "REGION", "WIDTH", "PEAK"] + (["QVAL"] if mode == "fdr" else [])
        _same_frame(got, want, (c, mode))
        assert got.attrs == attrs, (got.attrs, attrs)
        assert got.PEAK.dtype == bool and got.WIDTH.dtype == float
        n_hits, n_peaks = n_hits + len(got), n_peaks + int(got.PEAK.sum())
    assert 0 < n_peaks < n_hits                                  # (overlapping hits exist: HOT's tile lies in `width` windows)


@pytest.mark.parametrize("binsize", K.BINSIZES)
@pytest.mark.parametrize("mode", ["pval", "fdr"])
def test_width_one_gives_the_frames_of_nb_model_hits(binsize, mode):
    from digdriver_amd.sequence_model import nb_model
    P = _problem()
    cut = dict(pval_max=PVAL_MAX) if mode == "pval" else dict(fdr=FDR)
    want = nb_model.nb_model_hits(P["d_prs"], K.IDX, P["mu"], P["sigma"], P["frames"], P["genome"], n_up=1, n_down=1, binsize=binsize, **cut)
    got = _call(binsize, [1], mode)
    total = 0
    for c, (g, w) in enumerate(zip(got, want)):
        _same_frame(g[list(w.columns)], w, (c, mode))
        assert g.PEAK.all() and (g.WIDTH <= binsize).all()
        assert g.attrs == dict(n_testable=[w.attrs["n_testable"]], n_windows=[w.attrs["n_tiles"]])
        total += len(g)
    assert total > 0


@functools.lru_cache(maxsize=None)
def _thinned_frames(binsize):
    """Per cohort the frame of the rows tile_samples_statement leaves: dropped samples removed, min(n, cap) rows per (tile, sample)."""
    P = _problem()
    _, host, T = _base(binsize)
    st = P["st"]
    keep = SS.keep_from_max_muts([int(s) for s in st["sample"]], int(st["sample_offsets"][-1]), K.MAX_MUTS_PER_SAMPLE)
    stay = np.array(SS.thinned_rows(K.statement_regions(host["first_pos"], host["n_valid"]), K.statement_rows(st), K.C, binsize, T,
                                    keep=list(keep), cap=K.CAP))
    bounds = np.concatenate([[0], np.cumsum([len(r) for r in P["rows"]])])
    out = []
    for c, frame in enumerate(P["frames"]):
        mine = stay[(stay >= bounds[c]) & (stay < bounds[c + 1])] - bounds[c]
        out.append(frame.iloc[mine].reset_index(drop=True).drop(columns="ID"))
    assert len(out[0]) < len(P["frames"][0]) - 400
    return out


@pytest.mark.parametrize("binsize,widths", [(50, (2, 3)), (1, (30,))])
def test_a_cap_and_a_sample_filter_equal_the_same_call_on_host_thinned_rows(binsize, widths):
    got = _call(binsize, widths, "fdr", max_muts_per_sample=K.MAX_MUTS_PER_SAMPLE, max_muts_per_tile_per_sample=K.CAP)
    want = _call(binsize, widths, "fdr", frames=_thinned_frames(binsize))
    plain = _call(binsize, widths, "fdr")
    for c, (g, w) in enumerate(zip(got, want)):
        _same_frame(g, w, c)
        assert g.attrs == w.attrs
    assert len(got[0]) > 0 and (len(got[0]) != len(plain[0]) or not np.array_equal(got[0].OBS, plain[0].OBS))


# ---- the command line ----------------------------------------------------------------------------------------------------------
def test_tile_driver_in_fresh_child_processes(tmp_path):
    """`DigDriver.py tileDriver` twice, each in a child process of its own: with --window-tiles 1 3 the .hits.txt files are
    nb_model_window_hits' frames; without the option the bytes are those of nb_model_hits, as before."""
    from digdriver_amd.io import mapfile
    from digdriver_amd.sequence_model import nb_model
    P = _problem()
    fastas = [tmp_path / "genome_new.fa", tmp_path / "genome_old.fa"]          # one per child: each packs its genome beside its FASTA
    for fasta in fastas:
        fasta.write_text("".join(">%s\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))) for n, s in K.genome_sequences().items()))
    maps, files = [], []
    for c in range(K.C):
        m = str(tmp_path / ("map%d" % c))
        mapfile.write_frame(m, "region_params", pd.DataFrame({"CHROM": K.IDX[:, 0], "START": K.IDX[:, 1], "END": K.IDX[:, 2],
                                                              "Y_PRED": P["mu"][c], "STD": P["sigma"][c]}))
        mapfile.write_frame(m, "sequence_model_64", pd.DataFrame({"FREQ": list(P["d_prs"][c].values())},
                                                                 index=pd.Index(list(P["d_prs"][c].keys()), name="CONTEXT")))
        maps.append(m)
        files.append(K.write_file(tmp_path / ("muts%d.bed" % c), P["rows"][c]))
    script = os.path.join(ROOT, "scripts", "DigDriver.py")
    head = lambda fasta: [sys.executable, script, "tileDriver", str(fasta), "--maps"] + maps + ["--mutation-files"] + files + [
        "--binsize", "50", "--outpfx", "A", "B", "C", "--fdr", str(FDR)]
    runs = [subprocess.Popen(head(fastas[0]) + ["--outdir", str(tmp_path / "new"), "--window-tiles", "1", "3"], stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True),
            subprocess.Popen(head(fastas[1]) + ["--outdir", str(tmp_path / "old")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)]
    for run in runs:
        said, _ = run.communicate(timeout=300)
        assert run.returncode == 0, said
    new = _call(50, [1, 3], "fdr")
    old = nb_model.nb_model_hits(P["d_prs"], K.IDX, P["mu"], P["sigma"], P["frames"], P["genome"], n_up=1, n_down=1, binsize=50, fdr=FDR)
    for pfx, n, o in zip("ABC", new, old):
        for sub, frame in (("new", n), ("old", o)):
            want = tmp_path / ("want_%s_%s.txt" % (sub, pfx))
            mapfile.write_results_tsv(frame, str(want))
            assert (tmp_path / sub / (pfx + ".hits.txt")).read_bytes() == want.read_bytes(), (sub, pfx)
        header = (tmp_path / "new" / (pfx + ".hits.txt")).read_text().split("\n")[0].split("\t")
        assert header[1:] == ["CHROM", "POS", "OBS", "EXP", "PVAL", "Pi", "MU", "SIGMA", "REGION", "WIDTH", "PEAK", "QVAL"]
        assert (tmp_path / "old" / (pfx + ".hits.txt")).read_text().split("\n")[0].split("\t")[1:] == header[1:10] + ["QVAL"]
    assert sum(len(f) for f in new) > 0 and set(new[0].WIDTH) >= {50.0, 150.0}
