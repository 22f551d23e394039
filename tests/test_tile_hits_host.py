"""The hits of the per-base route, the parts that need no GPU: the refusals of nb_model_hits and of `DigDriver.py tileDriver`
before any device or file is touched, the two Benjamini-Hochberg identities the fdr mode rests on (nb_model.bh_cut,
nb_model.hits_q_values) bit for bit against get_q_vals of the NaN-dropped list, the frame helper nb_model and nb_model_hits share,
and the refusals of the two `_host` twins."""
import ctypes
import importlib.util
import os

import numpy as np
import pandas as pd
import pytest

from conftest import ROOT
from digdriver_amd import _lib
from digdriver_amd.sequence_model import nb_model


def _cli():
    spec = importlib.util.spec_from_file_location("dig_driver_cli_tiles", os.path.join(ROOT, "scripts", "DigDriver.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_nb_model_hits_refuses_both_cuts_and_no_cut_before_any_work():
    """Neither the genome nor the mutation files exist, and no device is needed: the cut is checked first."""
    args = ([{}], np.zeros((1, 3), int), [[1.0]], [[1.0]], ["/nonexistent/muts.bed"], "/nonexistent/genome.fa")
    with pytest.raises(ValueError, match="exactly one of pval_max and fdr"):
        nb_model.nb_model_hits(*args)
    with pytest.raises(ValueError, match="exactly one of pval_max and fdr"):
        nb_model.nb_model_hits(*args, pval_max=1e-3, fdr=0.1)


def test_tile_driver_refuses_unequal_lists_and_bad_cuts_before_reading_a_file():
    cli = _cli()
    a = cli.parse_args("tileDriver g.fa --mutation-files a.bed b.bed --maps a.h5 b.h5 --outdir o --outpfx A B --fdr 0.1 --chroms 1 2")
    assert a.func is cli.cmd_tile and a.mutation_files == ["a.bed", "b.bed"] and a.outpfx == ["A", "B"] and a.chroms == ["1", "2"]
    assert (a.binsize, a.up, a.down, a.pval_max, a.fdr) == (50, 1, 1, None, 0.1)
    base = "tileDriver /nonexistent/g.fa --outdir /nonexistent/out "
    with pytest.raises(SystemExit, match="same number of cohorts"):
        cli.main(base + "--mutation-files a.bed b.bed --maps a.h5 --outpfx A B --fdr 0.1")
    with pytest.raises(SystemExit, match="same number of cohorts"):
        cli.main(base + "--mutation-files a.bed b.bed --maps a.h5 b.h5 --outpfx A --pval-max 1e-3")
    with pytest.raises(SystemExit, match="exactly one of --pval-max and --fdr"):
        cli.main(base + "--mutation-files a.bed --maps a.h5 --outpfx A --pval-max 1e-3 --fdr 0.1")
    with pytest.raises(SystemExit, match="exactly one of --pval-max and --fdr"):
        cli.main(base + "--mutation-files a.bed --maps a.h5 --outpfx A")
    with pytest.raises(NotImplementedError, match="n_up = n_down = 1 or 2"):
        cli.main(base + "--mutation-files a.bed --maps a.h5 --outpfx A --fdr 0.1 --up 1 --down 2")
    assert not os.path.exists("/nonexistent/out")


def _random_list(rng, n):
    """p-values with ties, zeros, ones and NaNs, in random order."""
    p = rng.uniform(size=n) ** rng.choice([1, 3, 6])
    if n > 4:
        m = int(rng.integers(0, n // 2 + 1))
        p[rng.integers(0, n, m)] = p[rng.integers(0, n, m)]                      # ties
        p[rng.integers(0, n, int(rng.integers(0, 4)))] = 0.0
        p[rng.integers(0, n, int(rng.integers(0, 3)))] = 1.0
        p[rng.integers(0, n, int(rng.integers(0, n // 3 + 1)))] = np.nan
    return p


def test_the_two_bh_identities_hold_bit_for_bit():
    """For a list with NaNs: q = get_q_vals(the NaN-dropped list).  (1) {q <= fdr} = {p <= p*} with p* = bh_cut; (2) the hits'
    q-values, formed from the hits and the length of the testable list alone (hits_q_values), carry the bits of q.  Lists with
    ties, zeros, ones and NaNs; cuts that take nothing, something and everything, and one that equals a q-value."""
    rng = np.random.default_rng(11)
    seen_none = seen_all = seen_some = 0
    for trial in range(400):
        n = int(rng.choice([1, 2, 3, 7, 50, 333]))
        p = _random_list(rng, n)
        testable = p[~np.isnan(p)]
        q = nb_model.get_q_vals(testable)
        assert not np.isnan(q).any()
        cuts = [0.0, 0.05, 0.1, 0.5, 1.0] + ([float(q[rng.integers(0, q.size)])] if q.size else [])
        for fdr in cuts:
            p_star = nb_model.bh_cut(testable, q, fdr)
            want = q <= fdr
            with np.errstate(invalid="ignore"):
                hit = p <= p_star                                                # on the list WITH its NaNs: a NaN never hits
            assert np.array_equal(hit[~np.isnan(p)], want), (trial, fdr)
            assert not hit[np.isnan(p)].any()
            assert (p_star < 0) == (not want.any())
            got = nb_model.hits_q_values(p[hit], testable.size)
            assert got.tobytes() == q[want].tobytes(), (trial, fdr)
            seen_none += not want.any()
            seen_all += bool(want.all()) and want.size > 0
            seen_some += bool(want.any()) and not want.all()
    assert seen_none > 50 and seen_all > 50 and seen_some > 50
    assert nb_model.hits_q_values(np.zeros(0), 5).shape == (0,)
    assert nb_model.bh_cut(np.zeros(0), np.zeros(0), 0.1) < 0


def test_frame_helper_on_a_subset_equals_the_filtered_full_frame():
    """_tile_frame fed the rows of a filter == the full frame it builds, filtered: every column bit for bit; a ragged last
    tile, binsize 1 and > 1, a region without tiles, and an empty selection."""
    rng = np.random.default_rng(5)
    idx = np.array([[1, 0, 500], [1, 500, 1000], [2, 0, 99], [2, 2000, 2500], [3, 100, 137]])
    first = np.array([1, 500, 1, 2000, 100], np.int64)
    n_pos = np.array([499, 500, 97, 0, 37], np.int64)
    mu, sigma = rng.uniform(3, 40, 5), rng.uniform(1, 6, 5)
    for binsize in (1, 50):
        nval = -(-n_pos // binsize)
        reg = np.repeat(np.arange(5), nval)
        t = np.arange(nval.sum()) - np.repeat(np.cumsum(nval) - nval, nval)
        n = len(reg)
        obs, exp, pval, pi = rng.integers(0, 4, n).astype(np.int32), rng.uniform(size=n), rng.uniform(size=n) ** 4, rng.uniform(size=n)
        pval[rng.integers(0, n, 9)] = np.nan
        full = nb_model._tile_frame(idx, mu, sigma, first, n_pos, binsize, reg, t, obs, exp, pval, pi)
        assert list(full.columns) == ["CHROM", "POS", "OBS", "EXP", "PVAL", "Pi", "MU", "SIGMA", "REGION"] and len(full) == n
        assert full.REGION.iloc[0] == "1:0-500" and full.REGION.iloc[-1] == "3:100-137" and "2:2000-2500" not in set(full.REGION)
        last = full[full.REGION == "2:0-99"].iloc[-1]                           # 97 positions from 1 on: the last tile ends at 97
        assert last.POS == (97.0 if binsize == 1 else (51 + 97) / 2.0)
        for cut in (0.05, -1.0, 2.0):
            with np.errstate(invalid="ignore"):
                keep = pval <= cut
            sub = nb_model._tile_frame(idx, mu, sigma, first, n_pos, binsize, reg[keep], t[keep], obs[keep], exp[keep], pval[keep], pi[keep])
            sub.index = pd.Index(np.flatnonzero(keep), dtype=np.int64)
            pd.testing.assert_frame_equal(sub, full[full.PVAL <= cut], check_exact=True)
            for col in ("POS", "EXP", "PVAL", "Pi", "MU", "SIGMA"):
                assert sub[col].values.tobytes() == full[col].values[keep].tobytes()


def test_host_twins_and_binding_refuse_bad_sizes_before_touching_a_device():
    """C R >= 2^31, T >= 2^31 and a negative size are refused on the sizes alone; offsets that are no prefix sum by the fill twin."""
    lib = _lib.load()
    one = np.zeros(1)
    i1, o1 = np.zeros(1, np.int32), np.zeros(1, np.int64)
    p = _lib.host_ptr
    for C, R, T, fragment in ((1 << 16, 1 << 15, 1, "C R below 2^31"), (1, 1, 1 << 31, "fewer than 2^31 tiles"), (1, -1, 1, "C, R, T >= 0")):
        assert lib.dig_tile_select_count_host(p(one), p(i1), p(one), C, R, T, p(i1), 0) == -1
        assert fragment in _lib.last_error() and "dig_tile_select_count_host" in _lib.last_error()
        assert lib.dig_tile_select_fill_host(p(one), p(i1), p(one), C, R, T, p(o1), 1, *[None] * 9, 0) == -1
        assert fragment in _lib.last_error() and "dig_tile_select_fill_host" in _lib.last_error()
    assert lib.dig_tile_select_count_host(None, None, None, 1, 1, 1, p(i1), 0) == -1 and "non-null" in _lib.last_error()
    bad = np.array([0, 3, 2], np.int64)
    assert lib.dig_tile_select_fill_host(p(np.zeros(6)), p(np.full(1, 2, np.int32)), p(np.ones(3)), 3, 1, 2, p(bad), 4, *[None] * 9, 0) == -1
    assert "exclusive prefix sum" in _lib.last_error()
    assert lib.dig_tile_select_count_host(None, None, None, 0, 5, 7, None, 0) == 0             # nothing to do
    assert lib.dig_tile_select_fill_host(None, None, None, 2, 2, 2, None, 0, *[None] * 9, 0) == 0
    for name in ("dig_tile_select_count", "dig_tile_select_fill"):
        assert _lib._SIGNATURES[name][-1] is ctypes.c_void_p and _lib._SIGNATURES[name + "_host"][:-1] == _lib._SIGNATURES[name][:-1]
