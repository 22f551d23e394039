"""The distinct samples of sliding windows on the GPU (dig_tile_window_sample_keys, the key sort, dig_tile_window_samples behind
engine.tile_window_sample_keys / tile_window_samples; nb_model.nb_model_window_hits(window_samples=True); `DigDriver.py tileDriver
--window-tiles M --window-samples`).  Every comparison is exact: the counts are integers, and the p-values come from the same kernel on
equal inputs.
  1  the re-keyed keys and s_w of the device entry points and of the `_host` twins equal the plain-Python statement over the whole
     planes, tails included, on the problem of tile_samples_cases.py at the widths of tile_windows_cases.py; width 1 is k_samples
  2  on rows thinned on the host to one row per (cohort, region, sample), s_w is k_w of dig_tile_window_test and PVAL_SAMPLE its pval_w
  3  rows of 10 000 tiles (widths 7 and 1 024), samples on both sides of every 256-tile and 1 024-tile border: the scan's carry, the
     window clip at the row's end
  4  nb_model_window_hits(window_samples=True) column by column against what the statements select from the full planes, under
     pval_max and fdr, with either cut_on; tileDriver in fresh child processes, with the option and without it
The kernels launch one lane per key and one wave per row on uncapped grids: there is no grid-stride pass.  The scan has two compiled
forms (16-byte and 4-byte accesses); ordinary tensors with T a multiple of 4 take the first, test_gpu_window_samples_guarded.py takes
both."""
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
import tile_windows_statement as WS
import window_samples_statement as S

pytestmark = pytest.mark.gpu

PVAL_MAX, FDR = 1e-3, 0.1
CASES = [(b, m) for b in K.BINSIZES for m in W.widths(b)]


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def _up(x):
    import torch
    return None if x is None else torch.as_tensor(x, device="cuda:0")


@functools.lru_cache(maxsize=None)
def _problem():
    from digdriver_amd.data_tools.genome import PackedGenome
    from digdriver_amd.sequence_model import nb_model
    rows = K.cohort_rows()
    mu, sigma = K.mu_sigma()
    st = K.stacked(rows)
    keep = np.array(SS.keep_from_max_muts([int(s) for s in st["sample"]], int(st["sample_offsets"][-1]), K.MAX_MUTS_PER_SAMPLE), np.uint8)
    assert keep.sum() == len(keep) - 1 and keep[st["names"][0].index("HYPER")] == 0                 # the dropped sample
    d_prs = [K.s_prob(c) for c in range(K.C)]
    return dict(genome=PackedGenome.from_sequences(K.genome_sequences()), rows=rows, frames=K.frames(rows), st=st, keep=keep, d_prs=d_prs,
                s_prob=np.stack([nb_model._s_prob_table(d, 1) for d in d_prs]), mu=mu, sigma=sigma, chroms=[str(c) for c in K.IDX[:, 0]],
                n_samples=int(st["sample_offsets"][-1]))


def _with_foreign_cohorts(st):
    """The stack with two more rows in the busiest tile whose cohort ids lie outside [0, C)."""
    extra = dict(chrom=["1", "1"], start=[305, 305], end=[306, 306], cohort=[-1, K.C], sample=[0, 0])
    return {k: np.concatenate([st[k], np.array(extra[k], st[k].dtype)]) for k in extra}


def _front_of(P, rows, binsize, keep):
    """base_tile_probs and tile_sample_counts(return_keys=True) on device tensors: dict of device tensors."""
    from digdriver_amd import engine
    pt, first, nval = engine.base_tile_probs(P["genome"], P["chroms"], K.IDX[:, 1], K.IDX[:, 2], P["s_prob"], binsize)
    T = int(pt.shape[2])
    k, k_samples, keys = engine.tile_sample_counts(P["genome"], P["chroms"], K.IDX[:, 1], K.IDX[:, 2], first, nval, rows["chrom"],
                                                   _up(rows["start"]), _up(rows["end"]), _up(rows["cohort"]), _up(rows["sample"]),
                                                   P["st"]["sample_offsets"], _up(keep), None, K.C, binsize, T, return_keys=True)
    return dict(pt=pt, first_pos=first, n_valid=nval, k=k, k_samples=k_samples, keys=keys)


@functools.lru_cache(maxsize=None)
def _front(binsize):
    """The front half on the small problem (a dropped sample, rows of cohorts outside [0, C)): device tensors, host copies, T."""
    P = _problem()
    dev = _front_of(P, _with_foreign_cohorts(P["st"]), binsize, P["keep"])
    host = {n: _host(v) for n, v in dev.items()}
    T = -(-400 // binsize)
    assert host["pt"].shape == (K.C, 6, T) and list(host["n_valid"][:5]) == [T, -(-350 // binsize), T, W.SHORT_TILES[binsize], T]
    assert host["n_valid"][5] <= 0 and host["keys"].dtype == np.int64
    return dev, host, T


@functools.lru_cache(maxsize=None)
def _counts(binsize):
    """The statement's n[(cohort, region, tile, sample)] of the small problem."""
    P = _problem()
    _, host, T = _front(binsize)
    rows = K.statement_rows(_with_foreign_cohorts(P["st"]))
    return SS.counts_by_sample(K.statement_regions(host["first_pos"], host["n_valid"]), rows, K.C, binsize, T, list(P["keep"]))


@functools.lru_cache(maxsize=None)
def _want(binsize, width):
    _, host, T = _front(binsize)
    return S.window_sample_planes(_counts(binsize), K.C, [int(v) for v in host["n_valid"]], T, width)


@functools.lru_cache(maxsize=None)
def _sample_major(binsize, device=True):
    """engine.tile_window_sample_keys on the front's keys: a device tensor, or (device=False: the twin) an array."""
    from digdriver_amd import engine
    dev, host, T = _front(binsize)
    return engine.tile_window_sample_keys((dev if device else host)["keys"], K.C, 6, T, _problem()["n_samples"])


def _s_w(binsize, width, device=True, out=None):
    from digdriver_amd import engine
    dev, host, T = _front(binsize)
    got = engine.tile_window_samples(_sample_major(binsize, device), (dev if device else host)["n_valid"], K.C, 6, T, _problem()["n_samples"],
                                     width, out=out)
    assert got.is_cuda if device else isinstance(got, np.ndarray)
    return got


# ---- 1: keys and counts against the statement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("binsize", K.BINSIZES)
def test_keys_of_device_and_twin_equal_the_integer_arithmetic(binsize):
    _, host, T = _front(binsize)
    sb, slots = S.sample_bits(_problem()["n_samples"]), K.C * 6 * T
    old = [int(k) for k in host["keys"]]
    assert old == sorted(old) and [k for k in old if k != S.NO_KEY] == S.tile_major_keys(_counts(binsize), 6, T, sb)
    want = np.array(sorted(S.rekey(k, T, sb, slots) for k in old), np.int64)
    for device in (True, False):
        got = _host(_sample_major(binsize, device))
        assert got.dtype == np.int64 and np.array_equal(got, want), device
    # what the problem holds: pairs that count nowhere, a run of 300 equal keys, and the 70 samples of one tile apart from each other
    real = want[want != S.NO_KEY]
    assert 0 < len(real) < len(want) and np.unique(real, return_counts=True)[1].max() >= 300
    assert len(set(int(k) // T for k in real)) > 150


def test_keys_in_place_unsorted_and_hostile():
    """keys_out may be keys; the input need not be sorted; negative keys, INT64_MAX and keys of a tile outside the planes become INT64_MAX."""
    import torch
    from digdriver_amd import _lib
    C, R, T, n_samples = 2, 3, 5, 9
    sb, slots = S.sample_bits(n_samples), C * R * T
    rng = np.random.default_rng(8)
    old = [int(((int(rng.integers(0, slots)) << sb) | int(rng.integers(0, n_samples)))) for _ in range(700)] + [-1, -(1 << 62), S.NO_KEY, slots << sb,
                                                                                                               (1 << 62) + 5]
    old = [old[i] for i in rng.permutation(len(old))]
    want = np.array([S.rekey(k, T, sb, slots) for k in old], np.int64)
    keys = torch.tensor(old, dtype=torch.int64, device="cuda:0")
    _lib.call("dig_tile_window_sample_keys", keys.data_ptr(), len(old), C, R, T, n_samples, keys.data_ptr(), _lib.stream_ptr())
    assert np.array_equal(keys.cpu().numpy(), want) and (want == S.NO_KEY).sum() == 5


@pytest.mark.parametrize("binsize,width", CASES)
def test_counts_of_device_and_twin_equal_the_statement(binsize, width):
    _, host, T = _front(binsize)
    want = _want(binsize, width)
    for device in (True, False):
        got = _host(_s_w(binsize, width, device))
        assert got.dtype == np.int32 and got.shape == want.shape
        assert np.array_equal(got, want), (device, np.argwhere(got != want)[:5])
    nwin = np.array([WS.n_windows(v, T, width) for v in host["n_valid"]])
    behind = np.arange(T)[None, :] >= nwin[:, None]
    assert not want[:, behind].any() and not want[:, 5].any() and want[0, 0].max() >= 70
    if width == W.SHORT_TILES[binsize] + 1:
        assert nwin[3] == 1 and want[0, 3, 0] > 0 and nwin[0] > 1                       # ONE window over a short region


@pytest.mark.parametrize("binsize", K.BINSIZES)
def test_the_statements_planes_hold_what_can_go_wrong(binsize):
    """Nothing above passes vacuously: windows with two samples and more, with fewer samples than rows, and with more samples than
    any of their tiles has."""
    _, host, T = _front(binsize)
    seen = set()
    for width in W.widths(binsize):
        s_w = _want(binsize, width)
        _, k_w, nwin = WS.window_planes(host["pt"], host["k"], host["n_valid"], width)
        assert (s_w <= k_w).all()
        if (s_w >= 2).any():
            seen.add("two samples")
        if (s_w < k_w).any():
            seen.add("fewer samples than rows")
        most = np.zeros_like(s_w)                                                          # the most samples of a tile of the window
        for r in range(6):
            nv = max(min(int(host["n_valid"][r]), T), 0)
            for t in range(int(nwin[r])):
                most[:, r, t] = host["k_samples"][:, r, t:min(t + width, nv)].max(axis=1)
        assert (s_w >= most).all() and (s_w <= np.minimum(k_w, most * width)).all()
        if width > 1 and (s_w > most).any():
            seen.add("more samples than any tile")
        if width in (2, 3):
            assert (s_w >= 2).any() and (s_w < k_w).any() and (s_w > most).any(), width
    assert seen == {"two samples", "fewer samples than rows", "more samples than any tile"}


@pytest.mark.parametrize("binsize", K.BINSIZES)
def test_width_one_gives_k_samples_and_the_plane_is_reused(binsize):
    dev, host, T = _front(binsize)
    first = _s_w(binsize, 1)
    assert first.cpu().numpy().tobytes() == host["k_samples"].tobytes() and host["k_samples"].max() >= 70
    again = _s_w(binsize, 3, out=first)
    assert again.data_ptr() == first.data_ptr() and np.array_equal(again.cpu().numpy(), _want(binsize, 3))


def test_no_pairs_and_no_rows_give_zero_planes():
    from digdriver_amd import engine
    P = _problem()
    # five rows inside region 3's interval but behind its last tile (pairs of the join that count nowhere), and no rows at all
    nowhere = dict(chrom=np.array(["1"] * 5), start=2020 + np.arange(5, dtype=np.int64), end=2021 + np.arange(5, dtype=np.int64),
                   cohort=np.zeros(5, np.int32), sample=np.zeros(5, np.int32))
    for rows in (nowhere, {k: v[:0] for k, v in nowhere.items()}):
        front = _front_of(P, rows, 50, None)
        assert len(front["keys"]) == len(rows["start"])
        for device in (True, False):
            keys, nval = (front["keys"], front["n_valid"]) if device else (_host(front["keys"]), _host(front["n_valid"]))
            sm = engine.tile_window_sample_keys(keys, K.C, 6, 8, P["n_samples"])
            assert len(sm) == len(keys) and bool((sm == S.NO_KEY).all())
            got = _host(engine.tile_window_samples(sm, nval, K.C, 6, 8, P["n_samples"], 3, out=None if not device else _up(np.full((K.C, 6, 8), 7, np.int32))))
            assert got.shape == (K.C, 6, 8) and not got.any()


def test_the_engine_route_inside_a_side_stream():
    """Re-key, sort, memset, difference kernel and scan all go to the current stream: inside a side stream, with the default stream
    held busy, the planes carry the bits of the default-stream run (guarded_arena.side_stream_call)."""
    import guarded_arena as GA
    from digdriver_amd import engine
    dev, _, T = _front(1)
    ns = _problem()["n_samples"]

    def route(stream):
        sm = engine.tile_window_sample_keys(dev["keys"], K.C, 6, T, ns)
        return [sm] + [engine.tile_window_samples(sm, dev["n_valid"], K.C, 6, T, ns, w) for w in (3, 150)]
    ref = GA.side_stream_call(route, "cuda:0", "tile_window_samples")
    assert np.array_equal(ref["[1]"], _want(1, 3)) and np.array_equal(ref["[2]"], _want(1, 150))


# ---- 2: against the existing route on thinned rows ----------------------------------------------------------------------------------
@pytest.mark.parametrize("binsize,width", [(50, 2), (50, 3), (1, 3), (1, 150)])
def test_one_row_per_sample_and_region_gives_the_window_sums_of_the_existing_route(binsize, width):
    """Rows thinned on the host to one per (cohort, region, sample): a window's distinct samples are then its rows, so s_w is k_w of
    dig_tile_window_test on the row counts of dig_tile_mut_counts, and PVAL_SAMPLE its pval_w -- bit for bit."""
    from digdriver_amd import engine
    P = _problem()
    _, host, T = _front(binsize)
    regions, rows = K.statement_regions(host["first_pos"], host["n_valid"]), K.statement_rows(P["st"])
    seen, stay = set(), []
    for i, row in enumerate(rows):
        where = [(r, SS.pair_tile(row, region, binsize, T, K.C)) for r, region in enumerate(regions)]
        where = [(r, at) for r, at in where if at is not None]
        assert len(where) <= 1
        if where and (where[0][1][0], where[0][0], where[0][1][2]) not in seen:
            seen.add((where[0][1][0], where[0][0], where[0][1][2]))
            stay.append(i)
    thin = {k: P["st"][k][np.array(stay)] for k in ("chrom", "start", "end", "cohort", "sample")}
    front = _front_of(P, thin, binsize, None)
    k = engine.tile_mut_counts(P["genome"], P["chroms"], K.IDX[:, 1], K.IDX[:, 2], front["first_pos"], front["n_valid"], thin["chrom"],
                               _up(thin["start"]), _up(thin["end"]), _up(thin["cohort"]), K.C, binsize, T)
    planes = engine.tile_window_test(front["pt"], k, P["mu"], P["sigma"], front["n_valid"], width)
    sm = engine.tile_window_sample_keys(front["keys"], K.C, 6, T, P["n_samples"])
    s_w = engine.tile_window_samples(sm, front["n_valid"], K.C, 6, T, P["n_samples"], width)
    assert s_w.cpu().numpy().tobytes() == planes["k"].cpu().numpy().tobytes()
    pval_sample = engine.tiled_nb_test(planes["pt"], s_w, P["mu"], P["sigma"])[0]
    assert pval_sample.cpu().numpy().tobytes() == planes["pval"].cpu().numpy().tobytes()
    # (of the 70 samples of one tile, those whose first row in the region lies elsewhere were thinned away there)
    assert int(s_w.max()) >= 20 and len(stay) > 300 and np.isfinite(planes["pval"].cpu().numpy()).sum() > 0


# ---- 3: long rows ---------------------------------------------------------------------------------------------------------------
SCAN_CHUNK = 256                                                    # tiles of one step of a wave of tile_window_scan_kernel


@functools.lru_cache(maxsize=None)
def _long():
    """The rows of tile_windows_cases.long_rows() with labels dealt here: the background round-robin over five samples per cohort, and
    three more samples per cohort on both sides of every 256-tile border (and so of every 1 024-tile border) and in each region's last tile."""
    from digdriver_amd import engine
    from digdriver_amd.data_tools.genome import PackedGenome
    from digdriver_amd.sequence_model import nb_model
    g = PackedGenome.from_sequences(W.long_genome_sequences())
    chroms = [str(c) for c in W.LONG_IDX[:, 0]]
    s_prob = np.stack([nb_model._s_prob_table(W.long_s_prob(c), 1) for c in range(W.LONG_C)])
    pt, first, nval = engine.base_tile_probs(g, chroms, W.LONG_IDX[:, 1], W.LONG_IDX[:, 2], s_prob, 1)
    first_h, nval_h = first.cpu().numpy(), nval.cpu().numpy()
    assert pt.shape == (W.LONG_C, 2, W.LONG_T) and list(nval_h) == [10000, 9950] and list(first_h) == list(W.LONG_IDX[:, 1])
    per = 8                                                          # samples of a cohort: 5 dealt + 3 at the borders
    chrom, start, cohort, sample = [], [], [], []
    for c, (ch, st, _) in enumerate(W.long_rows()):
        chrom += [np.asarray(ch)]
        start += [np.asarray(st)]
        cohort += [np.full(len(st), c, np.int32)]
        sample += [(c * per + np.arange(len(st)) % 5).astype(np.int32)]
        for r in range(2):
            borders = np.arange(SCAN_CHUNK, int(nval_h[r]), SCAN_CHUNK)
            for j in range(3):
                at = np.concatenate([borders - 1 - j, borders + j, [int(nval_h[r]) - 1]])
                chrom += [np.full(len(at), chroms[r])]
                start += [first_h[r] + at]
                cohort += [np.full(len(at), c, np.int32)]
                sample += [np.full(len(at), c * per + 5 + j, np.int32)]
    rows = dict(chrom=np.concatenate([np.asarray(x) for x in chrom]), start=np.concatenate(start).astype(np.int64),
                cohort=np.concatenate(cohort), sample=np.concatenate(sample))
    rows["end"] = rows["start"] + 1
    offsets = np.arange(W.LONG_C + 1, dtype=np.int64) * per
    k, k_samples, keys = engine.tile_sample_counts(g, chroms, W.LONG_IDX[:, 1], W.LONG_IDX[:, 2], first, nval, rows["chrom"], _up(rows["start"]),
                                                   _up(rows["end"]), _up(rows["cohort"]), _up(rows["sample"]), offsets, None, None, W.LONG_C, 1,
                                                   W.LONG_T, return_keys=True)
    regions = [(chroms[r], int(W.LONG_IDX[r, 1]), int(W.LONG_IDX[r, 2]), int(first_h[r]), int(nval_h[r])) for r in range(2)]
    st_rows = [(str(a), int(b), int(b) + 1, int(c), int(s)) for a, b, c, s in zip(rows["chrom"], rows["start"], rows["cohort"], rows["sample"])]
    n = SS.counts_by_sample(regions, st_rows, W.LONG_C, 1, W.LONG_T)
    return dict(keys=keys, n_valid=nval, nval_h=nval_h, n=n, n_samples=W.LONG_C * per, k_samples=k_samples.cpu().numpy())


@pytest.mark.parametrize("width", W.LONG_WIDTHS)
def test_rows_longer_than_a_scan_step_equal_the_statement(width):
    from digdriver_amd import engine
    L = _long()
    C, R, T, ns = W.LONG_C, 2, W.LONG_T, L["n_samples"]
    want = S.window_sample_planes(L["n"], C, [int(v) for v in L["nval_h"]], T, width, marked=True)
    for device in (True, False):
        keys, nval = (L["keys"], L["n_valid"]) if device else (_host(L["keys"]), L["nval_h"])
        got = _host(engine.tile_window_samples(engine.tile_window_sample_keys(keys, C, R, T, ns), nval, C, R, T, ns, width))
        assert np.array_equal(got, want), (device, np.argwhere(got != want)[:5])
    for r in range(R):
        nw = int(L["nval_h"][r]) - width + 1
        assert not want[:, r, nw:].any() and (want[:, r, nw - 1] >= 3).all()                # the clip at the row's end: the last window holds three
        for border in range(SCAN_CHUNK, nw, SCAN_CHUNK):
            # the three border samples lie in the window that starts one tile in front of the border, once each, and the carry
            # arrives with them: the count at the border is what the statement says, and it is not 0
            assert (want[:, r, border - 1] >= 3).all() and (want[:, r, border] >= 3).all(), (r, border)
    assert (want > L["k_samples"]).any() and want.max() <= 8
    # the marked form of the statement is the set form: on the first 600 tiles of one row
    head = {s: [t for t in tiles if t < 600] for s, tiles in S.tiles_by_row(L["n"])[(0, 0)].items()}
    assert S.window_counts_row_marked(head, 600, 600, width) == S.window_counts_row(head, 600, 600, width)


# ---- 4: nb_model_window_hits ------------------------------------------------------------------------------------------------------
def _call(binsize, widths, mode, cut_on, **kw):
    from digdriver_amd.sequence_model import nb_model
    P = _problem()
    cut = dict(pval_max=PVAL_MAX) if mode == "pval" else dict(fdr=FDR)
    return nb_model.nb_model_window_hits(P["d_prs"], K.IDX, P["mu"], P["sigma"], P["frames"], P["genome"], n_up=1, n_down=1, binsize=binsize,
                                         widths=widths, max_muts_per_sample=K.MAX_MUTS_PER_SAMPLE, cut_on=cut_on, **cut, **kw)


@functools.lru_cache(maxsize=None)
def _full_planes(binsize, width):
    """The full window planes of the small problem as host arrays: the existing route's (dig_tile_window_test, pinned by
    test_gpu_tile_windows.py) on the front's planes, the statement's s_w, and dig_tiled_nb_test on (pt_w, s_w)."""
    from digdriver_amd import engine
    P = _problem()
    dev, _, _ = _front(binsize)
    planes = engine.tile_window_test(dev["pt"], dev["k"], P["mu"], P["sigma"], dev["n_valid"], width)
    s_w = _want(binsize, width)
    pval_sample = engine.tiled_nb_test(planes["pt"], _up(s_w), P["mu"], P["sigma"])[0]
    return dict({n: _host(v) for n, v in planes.items()}, s_w=s_w, pval_sample=_host(pval_sample))


@pytest.mark.parametrize("binsize,widths", [(50, (2, 1, 4)), (1, (30, 150))])
@pytest.mark.parametrize("mode", ["pval", "fdr"])
@pytest.mark.parametrize("cut_on", ["PVAL", "PVAL_SAMPLE"])
def test_window_hits_equal_what_the_statements_select_from_the_full_planes(binsize, widths, mode, cut_on):
    from digdriver_amd.sequence_model import nb_model
    P = _problem()
    _, host, _ = _front(binsize)
    frames = _call(binsize, widths, mode, cut_on, window_samples=True)
    n_pos = nb_model._region_positions(P["genome"], P["chroms"], K.IDX[:, 2], host["first_pos"], 1)
    score_of = "pval_sample" if cut_on == "PVAL_SAMPLE" else "pval"
    n_hits = n_peaks = 0
    for c, got in enumerate(frames):
        full = [_full_planes(binsize, m) for m in widths]
        planes = [dict(pt=f["pt"][c], k=f["k"][c], exp=f["exp"][c], pval=f[score_of][c], n_windows=f["n_windows"]) for f in full]
        # width by width (peaks and q-values are per width): the statement numbers a hit by its row in the width's full frame, which
        # names its (region, window)
        cols, index, where, attrs = None, [], [], dict(n_testable=[], n_windows=[])
        for w, (m, f, pl) in enumerate(zip(widths, full, planes)):
            one, rows_w, attrs_w = WS.window_hits(K.IDX, P["mu"][c], P["sigma"][c], host["first_pos"], n_pos, host["n_valid"], binsize, [m], [pl],
                                                  **(dict(pval_max=PVAL_MAX) if mode == "pval" else dict(fdr=FDR)))
            rt = [(r, t) for r in range(len(K.IDX)) for t in range(int(f["n_windows"][r]))]
            where += [(w,) + rt[i] for i in rows_w]
            index += rows_w
            cols = one if cols is None else {n: cols[n] + one[n] for n in one}
            for n in attrs:
                attrs[n] += attrs_w[n]
        cols["PVAL"] = [full[w]["pval"][c][r][t] for w, r, t in where]
        names = list(cols)
        want = pd.DataFrame(cols, index=pd.Index(index, dtype=np.int64))
        want["OBS_SAMPLES"] = [float(full[w]["s_w"][c][r][t]) for w, r, t in where]
        want["PVAL_SAMPLE"] = [full[w]["pval_sample"][c][r][t] for w, r, t in where]
        order = names[:9] + ["OBS_SAMPLES", "PVAL_SAMPLE"] + names[9:]
        want = want[order]
        assert list(got.columns) == ["CHROM", "POS", "OBS", "EXP", "PVAL", "Pi", "MU", "SIGMA", "REGION", "OBS_SAMPLES", "PVAL_SAMPLE", "WIDTH",
                                     "PEAK"] + (["QVAL"] if mode == "fdr" else [])
        _same_frame(got, want, (c, mode, cut_on))
        assert got.attrs == attrs, (got.attrs, attrs)
        assert (got.OBS_SAMPLES <= got.OBS).all() and got.PEAK.dtype == bool
        n_hits, n_peaks = n_hits + len(got), n_peaks + int(got.PEAK.sum())
    assert 0 < n_peaks <= n_hits


def _same_frame(got, want, what):
    assert list(got.columns) == list(want.columns), what
    assert got.index.dtype == np.int64 and list(got.index) == list(want.index), what
    if len(want) == 0:
        assert len(got) == 0, what
        return
    pd.testing.assert_frame_equal(got, want, check_exact=True)
    for col in got.columns:
        if col not in ("REGION", "PEAK"):
            assert np.asarray(got[col], float).tobytes() == np.asarray(want[col], float).tobytes(), (what, col)


def test_the_sample_score_drops_the_hit_that_one_sample_makes():
    """HOT's 300 rows in one tile make every window over it a hit on PVAL; they are one sample, and on PVAL_SAMPLE those windows are
    hits only where other samples carry them.  Without the keyword the frames are those of before."""
    on_rows = _call(1, (10,), "pval", "PVAL", window_samples=True)[0]
    on_samples = _call(1, (10,), "pval", "PVAL_SAMPLE", window_samples=True)[0]
    plain = _call(1, (10,), "pval", "PVAL")[0]
    hot = on_rows[(on_rows.OBS >= 300)]
    assert len(hot) >= 5 and (hot.OBS_SAMPLES < 20).all() and (hot.PVAL <= PVAL_MAX).all()
    assert len(on_samples) < len(on_rows) and (on_samples.PVAL_SAMPLE <= PVAL_MAX).all() and not (on_rows.PVAL_SAMPLE <= PVAL_MAX).all()
    _same_frame(on_rows.drop(columns=["OBS_SAMPLES", "PVAL_SAMPLE"]), plain, "the columns of before")
    assert on_rows.attrs == plain.attrs


# ---- the command line ----------------------------------------------------------------------------------------------------------
def test_tile_driver_in_fresh_child_processes(tmp_path):
    """`DigDriver.py tileDriver --window-tiles 1 3` twice, each in a child process of its own: with --window-samples --cut-on PVAL_SAMPLE
    the .hits.txt files are the frames of nb_model_window_hits(window_samples=True); without the option the bytes are those of the
    route as it is."""
    from digdriver_amd.io import mapfile
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
        "--binsize", "50", "--outpfx", "A", "B", "C", "--fdr", str(FDR), "--window-tiles", "1", "3", "--max-muts-per-sample", str(K.MAX_MUTS_PER_SAMPLE)]
    runs = [subprocess.Popen(head(fastas[0]) + ["--outdir", str(tmp_path / "new"), "--window-samples", "--cut-on", "PVAL_SAMPLE"],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True),
            subprocess.Popen(head(fastas[1]) + ["--outdir", str(tmp_path / "old")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)]
    for run in runs:
        said, _ = run.communicate(timeout=300)
        assert run.returncode == 0, said
    new = _call(50, [1, 3], "fdr", "PVAL_SAMPLE", window_samples=True)
    old = _call(50, [1, 3], "fdr", "PVAL")
    for pfx, n, o in zip("ABC", new, old):
        for sub, frame in (("new", n), ("old", o)):
            want = tmp_path / ("want_%s_%s.txt" % (sub, pfx))
            mapfile.write_results_tsv(frame, str(want))
            assert (tmp_path / sub / (pfx + ".hits.txt")).read_bytes() == want.read_bytes(), (sub, pfx)
        header = (tmp_path / "new" / (pfx + ".hits.txt")).read_text().split("\n")[0].split("\t")
        assert header[1:] == ["CHROM", "POS", "OBS", "EXP", "PVAL", "Pi", "MU", "SIGMA", "REGION", "OBS_SAMPLES", "PVAL_SAMPLE", "WIDTH", "PEAK", "QVAL"]
        assert (tmp_path / "old" / (pfx + ".hits.txt")).read_text().split("\n")[0].split("\t")[1:] == header[1:10] + header[12:]
    assert sum(len(f) for f in new) > 0 and list(old[0].columns) == header[1:10] + header[12:]
