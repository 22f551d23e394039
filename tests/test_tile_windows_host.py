"""Sliding windows in the per-base route, the parts that need no GPU: the plain-Python statement's hand-worked cases, its two forms
against each other, the PEAK rule (ties included), the bindings, the refusals of the `_host` twin before any device work, the
ValueErrors of engine.tile_window_test and nb_model.nb_model_window_hits, and the command line."""
import ctypes
import importlib.util
import os
import struct

import numpy as np
import pytest

from conftest import ROOT
import tile_windows_cases as W
import tile_windows_statement as S
from digdriver_amd import _lib, engine
from digdriver_amd.sequence_model import nb_model


def _same(got, want):
    """Equal floats, NaN in the same places."""
    return len(got) == len(want) and all(struct.pack("d", g) == struct.pack("d", w) or (g != g and w != w) for g, w in zip(got, want))


@pytest.mark.parametrize("name", sorted(S.HAND_CASES))
def test_statement_hand_cases(name):
    pt, k, n_valid, m, pt_w, k_w, nw = S.HAND_CASES[name]
    got = S.window_row(pt, k, n_valid, m)
    assert _same(got[0], pt_w) and got[1] == k_w and got[2] == nw == S.n_windows(n_valid, len(pt), m)
    # the whole-plane form says the same
    planes = S.window_planes(np.array(pt)[None, None, :], np.array(k, np.int32)[None, None, :], [n_valid], m)
    assert _same(list(planes[0][0, 0]), pt_w) and list(planes[1][0, 0]) == k_w and list(planes[2]) == [nw]


@pytest.mark.parametrize("m", [1, 2, 3, 7, 8, 9, 40])
def test_the_two_forms_of_the_statement_agree_bit_for_bit(m):
    rng = np.random.default_rng(m)
    C, R, T = 2, 5, 8
    pt = rng.uniform(0, 1, (C, R, T)) * 10.0 ** rng.integers(-12, 3, (C, R, T))         # terms of very different sizes: the order shows
    k = rng.integers(0, 5, (C, R, T)).astype(np.int32)
    n_valid = [8, 7, 3, 0, -1]
    pt_w, k_w, nw = S.window_planes(pt, k, n_valid, m)
    for c in range(C):
        for r in range(R):
            row = S.window_row(list(pt[c, r]), [int(x) for x in k[c, r]], n_valid[r], m)
            assert pt_w[c, r].tobytes() == np.array(row[0]).tobytes() and list(k_w[c, r]) == row[1] and nw[r] == row[2]


def test_the_widths_of_the_cases_are_what_the_issue_names():
    for binsize, T in ((50, 8), (1, 400)):
        w = W.widths(binsize)
        assert w[:3] == [1, 2, 3] and T % 3 != 0 and w[3:5] == [T, T + 1] and w[5] == W.SHORT_TILES[binsize] + 1 and len(set(w)) == 6
    assert W.MAX_WIDTH == engine.TILE_WINDOW_MAX_WIDTH >= 1024 and max(W.LONG_WIDTHS) <= W.MAX_WIDTH and W.LONG_T > W.CHUNK
    header = open(os.path.join(ROOT, "include", "dig_hip.h")).read()
    assert "#define DIG_TILE_WINDOW_MAX_WIDTH %d" % W.MAX_WIDTH in header
    source = open(os.path.join(ROOT, "digdriver_amd", "csrc", "dig_tilewindows.hip")).read()
    assert "kWinBlock = 256" in source and "kWinItems = 4" in source and "kWinChunk = kWinBlock * kWinItems" in source and W.CHUNK == 1024


@pytest.mark.parametrize("name", sorted(S.PEAK_CASES))
def test_peak_rule(name):
    region, tile, score, m, want = S.PEAK_CASES[name]
    assert S.peaks(region, tile, score, m) == want
    assert list(nb_model.window_peaks(region, tile, score, m)) == want
    # the rule does not depend on the order the hits are listed in
    order = list(reversed(range(len(tile))))
    got = nb_model.window_peaks([region[i] for i in order], [tile[i] for i in order], [score[i] for i in order], m)
    assert [bool(got[order.index(i)]) for i in range(len(tile))] == want


def test_peaks_of_random_hits_agree_with_the_statement():
    rng = np.random.default_rng(3)
    for m in (1, 2, 5):
        n = 60
        region, tile = rng.integers(0, 3, n), rng.integers(0, 40, n)
        score = rng.choice([1e-9, 1e-6, 1e-6, 1e-4], n)                                   # many ties
        _, first = np.unique(region * 100 + tile, return_index=True)                         # a (region, tile) is one hit
        region, tile, score = region[first], tile[first], score[first]
        want = S.peaks(list(region), list(tile), list(score), m)
        assert list(nb_model.window_peaks(region, tile, score, m)) == want and (m > 1) == (not all(want))


# ---- the library: bindings and refusals, no device -----------------------------------------------------------------------------
def test_bindings_mirror_the_header():
    header = open(os.path.join(ROOT, "include", "dig_hip.h")).read()
    name = "dig_tile_window_test"
    assert name + "(" in header and name + "_host(" in header
    assert _lib._SIGNATURES[name][-1] is ctypes.c_void_p and _lib._SIGNATURES[name + "_host"][-1] is ctypes.c_int
    assert _lib._SIGNATURES[name + "_host"][:-1] == _lib._SIGNATURES[name][:-1] and len(_lib._SIGNATURES[name]) == 15
    assert name in _lib.EXPORTED_SYMBOLS and name + "_host" in _lib.EXPORTED_SYMBOLS
    assert _lib.load().dig_abi_version() == 12


def _twin(C, R, T, width, buf=None):
    buf = np.zeros(64, np.float64) if buf is None else buf
    p = _lib.host_ptr(buf)
    return _lib.load().dig_tile_window_test_host(p, p, p, p, p, C, R, T, width, p, p, p, p, p, 0)


@pytest.mark.parametrize("sizes,fragment", [((1, 1, 1, 0), "1 <= width"), ((1, 1, 1, -3), "1 <= width"), ((1, 1, 1, W.MAX_WIDTH + 1), "1 <= width"),
                                            ((1 << 16, 1 << 15, 1, 1), "C R below 2^31"), ((1, 1 << 31, 1, 1), "C R below 2^31"),
                                            ((1, 1, 1 << 31, 1), "fewer than 2^31 tiles"), ((-1, 1, 1, 1), "C, R, T >= 0")])
def test_host_twin_refuses_before_any_device_work(sizes, fragment):
    assert _twin(*sizes) == -1
    msg = _lib.last_error()
    assert "dig_tile_window_test_host" in msg and "requirement failed" in msg and fragment in msg, msg


def test_host_twin_returns_at_once_for_empty_inputs_and_without_outputs():
    """Nothing to do: DIG_OK before any device call, so it is seen without a device."""
    for sizes in ((0, 5, 7, 3), (4, 0, 7, 3), (4, 5, 0, 3), (0, 0, 0, W.MAX_WIDTH)):
        assert _twin(*sizes) == 0
    p = _lib.host_ptr(np.zeros(64))
    assert _lib.load().dig_tile_window_test_host(p, p, p, p, p, 1, 2, 3, 1, None, None, None, None, None, 0) == 0


def test_engine_refusals_are_value_errors():
    pt, k, mu = np.zeros((1, 2, 3)), np.zeros((1, 2, 3), np.int32), np.ones((1, 2))
    for width in (0, -1, W.MAX_WIDTH + 1):
        with pytest.raises(ValueError, match="1 <= width"):
            engine.tile_window_test(pt, k, mu, mu, [3, 3], width)
    for width in (1.5, True):
        with pytest.raises(ValueError, match="an integer >= 1"):
            engine.tile_window_test(pt, k, mu, mu, [3, 3], width)
    with pytest.raises(ValueError, match=r"\[C, R, T\]"):
        engine.tile_window_test(pt, k[:, :, :2], mu, mu, [3, 3], 1)


@pytest.mark.parametrize("kw,match", [(dict(widths=[]), "at least one"), (dict(widths=[2, 0]), "integer >= 1"), (dict(widths=[1.5]), "integer >= 1"),
                                      (dict(widths=[True]), "integer >= 1"), (dict(widths=["2"]), "integer >= 1"),
                                      (dict(widths=[2, 3, 2]), "given twice"), (dict(widths=[W.MAX_WIDTH + 1]), "at most"),
                                      (dict(widths=[2], by_sample=True), "by_sample"), (dict(widths=[2], cut_on="PVAL_SAMPLE"), "cut_on"),
                                      (dict(widths=[2], pval_max=None), "exactly one"), (dict(widths=[2], fdr=0.1), "exactly one")])
def test_window_hits_refuses_before_a_genome_is_packed_or_a_device_is_touched(kw, match):
    args = dict(pval_max=0.1)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        nb_model.nb_model_window_hits([{}], np.zeros((0, 3)), [[]], [[]], ["no such file"], "no such fasta", n_up=1, n_down=1, **args)


def test_widths_are_taken_in_the_order_given():
    assert nb_model._check_widths((3, 1, 2)) == [3, 1, 2] and nb_model._check_widths([np.int64(4), 2.0]) == [4, 2] and nb_model._check_widths(5) == [5]


# ---- the command line ----------------------------------------------------------------------------------------------------------
def _cli():
    spec = importlib.util.spec_from_file_location("dig_driver_cli_tile_windows", os.path.join(ROOT, "scripts", "DigDriver.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BASE = "tileDriver g.fa --mutation-files a.bed b.bed --maps ma mb --outdir out --outpfx A B --fdr 0.1 "


def test_command_line_parses_the_option():
    cli = _cli()
    assert cli.parse_args(BASE).window_tiles is None
    a = cli.parse_args(BASE + "--window-tiles 3 1 10")
    assert a.window_tiles == [3, 1, 10] and a.func is cli.cmd_tile
    for bad in ("--window-tiles", "--window-tiles 1.5", "--window-tiles x"):
        with pytest.raises(SystemExit):
            cli.parse_args(BASE + bad)


@pytest.mark.parametrize("options,match", [("--window-tiles 2 --sparse", "--window-tiles is not part of --sparse"),
                                           ("--window-tiles 2 --by-sample", "--window-tiles does not take --by-sample"),
                                           ("--window-tiles 2 --by-sample --cut-on PVAL_SAMPLE", "--window-tiles does not take --by-sample"),
                                           ("--window-tiles 2 --cut-on PVAL_SAMPLE", "--window-tiles selects on PVAL only"),
                                           ("--window-tiles 2 0", "distinct integers >= 1"), ("--window-tiles 2 2", "distinct integers >= 1")])
def test_command_line_refusals_come_before_any_file_is_read(options, match):
    cli = _cli()
    with pytest.raises(SystemExit, match=match):
        cli.main(BASE + options)
    assert not os.path.exists("out")
