"""The distinct samples of sliding windows, the parts that need no GPU: the plain-Python statement's hand-worked cases, its three forms
against each other, the re-keying as integer arithmetic, the bindings, the refusals of the `_host` twins before any device work, the
ValueErrors of engine.tile_window_samples and nb_model.nb_model_window_hits, and the command line."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
import tile_windows_cases as W
import window_samples_statement as S
from digdriver_amd import _lib, engine
from digdriver_amd.sequence_model import nb_model

NAMES = ("dig_tile_window_sample_keys", "dig_tile_window_samples")


@pytest.mark.parametrize("name", sorted(S.HAND_CASES))
def test_statement_hand_cases(name):
    tiles, n_valid, T, m, diff, s_w = S.HAND_CASES[name]
    assert S.window_counts_row(tiles, n_valid, T, m) == s_w
    assert S.interval_differences(tiles, n_valid, T, m) == diff and S.prefix_sums(diff) == s_w
    assert S.window_counts_row_marked(tiles, n_valid, T, m) == s_w


def test_the_hand_cases_of_the_issue_are_among_them():
    assert S.HAND_CASES["two samples"][4:] == ([2, 0, 0, -2, 1, 0, -1, 0], [2, 2, 2, 0, 1, 1, 0, 0])
    assert S.HAND_CASES["short region"][1:4] == (2, 8, 3) and S.HAND_CASES["short region"][5][:2] == [1, 0]
    tiles = S.HAND_CASES["gaps around the width"][0]["A"]
    assert [b - a for a, b in zip(tiles, tiles[1:])] == [2, 3, 4] and S.HAND_CASES["gaps around the width"][3] == 3


@pytest.mark.parametrize("m", [1, 2, 3, 5, 8, 9, 40])
def test_the_three_forms_of_the_statement_agree(m):
    rng = np.random.default_rng(m)
    T = 8 if m < 9 else 37
    for n_valid in (T, T - 1, 3, 1, 0, -2, T + 5):
        tiles = {s: sorted(set(int(t) for t in rng.integers(0, T, rng.integers(0, 6)))) for s in range(7)}
        tiles[7] = list(range(T))                                                        # one sample in every tile
        want = S.window_counts_row(tiles, n_valid, T, m)
        assert S.prefix_sums(S.interval_differences(tiles, n_valid, T, m)) == want
        assert S.window_counts_row_marked(tiles, n_valid, T, m) == want
        nw = S.WS.n_windows(n_valid, T, m)
        assert all(x == 0 for x in want[nw:]) and (nw == 0 or min(want[:nw]) >= 1)


def test_a_sample_has_no_predecessor_across_rows():
    """The same sample in the last tile of one row and in the first tile of the next: two rows, two keys whose quotients by T differ."""
    C, R, T, m, sb = 1, 2, 6, 3, S.sample_bits(4)
    n = {(0, 0, T - 1, 2): 1, (0, 1, 0, 2): 3}
    got = S.window_sample_planes(n, C, [T, T], T, m)
    assert got.tolist() == [[[0, 0, 0, 1, 0, 0], [1, 0, 0, 0, 0, 0]]]
    keys = sorted(S.rekey(k, T, sb, C * R * T) for k in S.tile_major_keys(n, R, T, sb))
    assert len(keys) == 4 and keys[0] // T != keys[1] // T and keys[1] == keys[2] == keys[3]
    assert keys[0] % T == T - 1 and keys[1] % T == 0 and (keys[0] // T) & ((1 << sb) - 1) == (keys[1] // T) & ((1 << sb) - 1) == 2


def test_rekeying_is_integer_arithmetic_and_orders_by_row_sample_tile():
    rng = np.random.default_rng(1)
    C, R, T, n_samples = 3, 5, 7, 11
    sb = S.sample_bits(n_samples)
    assert sb == 4 and S.sample_bits(15) == 4 and S.sample_bits(16) == 5 and S.sample_bits(0) == 1
    quads = [(int(c), int(r), int(t), int(s)) for c, r, t, s in zip(rng.integers(0, C, 200), rng.integers(0, R, 200), rng.integers(0, T, 200),
                                                                      rng.integers(0, n_samples, 200))]
    old = [(((c * R + r) * T + t) << sb) | s for c, r, t, s in quads]
    new = [S.rekey(k, T, sb, C * R * T) for k in old]
    assert new == [(((c * R + r) << sb) | s) * T + t for c, r, t, s in quads]
    assert [quads[i] for i in np.argsort(new, kind="stable")] == sorted(quads, key=lambda q: (q[0], q[1], q[3], q[2]))
    assert max(new) < (C * R * T) << sb
    for bad in (-1, -(1 << 62), S.NO_KEY, (C * R * T) << sb):
        assert S.rekey(bad, T, sb, C * R * T) == S.NO_KEY


# ---- the library: bindings and refusals, no device -----------------------------------------------------------------------------
def test_header_bindings_and_twins():
    header = open(os.path.join(ROOT, "include", "dig_hip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        for sym in (name, name + "_host"):
            assert sym + "(" in header and sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym)
        assert _lib._SIGNATURES[name][-1] is ctypes.c_void_p and _lib._SIGNATURES[name + "_host"][-1] is ctypes.c_int
        assert _lib._SIGNATURES[name + "_host"][:-1] == _lib._SIGNATURES[name][:-1]
    assert [len(_lib._SIGNATURES[n]) for n in NAMES] == [8, 10]
    assert lib.dig_abi_version() == 12
    makefile = open(os.path.join(ROOT, "digdriver_amd", "csrc", "Makefile")).read()
    assert "dig_tilewindowsamples.hip" in makefile


def _samples_twin(n, C, R, T, n_samples, width, keys=None):
    keys = np.zeros(64, np.int64) if keys is None else keys
    buf = np.zeros(64, np.int32)
    return _lib.load().dig_tile_window_samples_host(_lib.host_ptr(keys), n, _lib.host_ptr(buf), C, R, T, n_samples, width, _lib.host_ptr(buf), 0)


@pytest.mark.parametrize("args,fragment", [((1, 1, 1, 1, 1, 0), "1 <= width"), ((1, 1, 1, 1, 1, W.MAX_WIDTH + 1), "1 <= width"),
                                           ((1, 1 << 16, 1 << 15, 1, 1, 1), "C R below 2^31"), ((1, 1, 1, 1 << 31, 1, 1), "fewer than 2^31 tiles"),
                                           ((1 << 31, 1, 1, 1, 1, 1), "0 <= n < 2^31"), ((-1, 1, 1, 1, 1, 1), "0 <= n < 2^31"),
                                           ((1, 1, 1, 1, 1 << 31, 1), "below 2^31"),
                                           ((1, 1 << 20, 1 << 10, 1 << 20, 1 << 20, 1), "does not fit 63 bits")])
def test_samples_twin_refuses_before_any_device_work(args, fragment):
    assert _samples_twin(*args) == -1
    msg = _lib.last_error()
    assert "dig_tile_window_samples_host" in msg and "requirement failed" in msg and fragment in msg, msg


def test_samples_twin_refuses_descending_keys():
    keys = np.array([5, 9, 7, 12], np.int64)
    assert _samples_twin(4, 1, 2, 8, 3, 2, keys) == -1
    msg = _lib.last_error()
    assert "dig_tile_window_samples_host" in msg and "keys ascending" in msg, msg


def test_keys_twin_refusals_and_empty_calls():
    lib = _lib.load()
    p = _lib.host_ptr(np.zeros(8, np.int64))
    assert lib.dig_tile_window_sample_keys_host(p, -1, 1, 1, 1, 1, p, 0) == -1 and "n >= 0" in _lib.last_error()
    assert lib.dig_tile_window_sample_keys_host(p, 4, 1 << 20, 1 << 10, 1 << 20, 1 << 20, p, 0) == -1
    assert "dig_tile_window_sample_keys_host" in _lib.last_error() and "does not fit 63 bits" in _lib.last_error()
    assert lib.dig_tile_window_sample_keys_host(p, 4, 1, 1, 1 << 31, 1, p, 0) == -1 and "below 2^31" in _lib.last_error()
    # nothing to do: DIG_OK before any device call
    assert lib.dig_tile_window_sample_keys_host(p, 0, 3, 4, 5, 6, p, 0) == 0
    for sizes in ((0, 5, 7), (4, 0, 7), (4, 5, 0)):
        assert _samples_twin(3, *sizes, 2, 2) == 0


def test_engine_refusals_are_value_errors():
    keys, n_valid = np.zeros(3, np.int64), np.array([3, 3], np.int32)
    for width in (0, -1, W.MAX_WIDTH + 1):
        with pytest.raises(ValueError, match="1 <= width"):
            engine.tile_window_samples(keys, n_valid, 1, 2, 3, 4, width)
    for width in (1.5, True):
        with pytest.raises(ValueError, match="an integer >= 1"):
            engine.tile_window_samples(keys, n_valid, 1, 2, 3, 4, width)
    with pytest.raises(ValueError, match=r"\[C, R, T\]"):
        engine.tile_window_samples(keys, n_valid, 1, 2, 3, 4, 1, out=np.zeros((1, 2, 2), np.int32))
    with pytest.raises(ValueError, match="keys ascending"):
        engine.tile_window_samples(np.array([4, 2], np.int64), n_valid, 1, 2, 3, 4, 1)
    with pytest.raises(ValueError, match="does not fit 63 bits"):
        engine.tile_window_sample_keys(keys, 1 << 20, 1 << 10, 1 << 20, 1 << 20)


def _hits(**kw):
    args = dict(pval_max=0.1, widths=[2])
    args.update(kw)
    return nb_model.nb_model_window_hits([{}], np.zeros((0, 3)), [[]], [[]], ["no such file"], "no such fasta", n_up=1, n_down=1, **args)


@pytest.mark.parametrize("kw,match", [(dict(window_samples=True, by_sample=True), "by_sample"), (dict(cut_on="PVAL_SAMPLE"), "cut_on"),
                                      (dict(cut_on="PVAL_SAMPLE"), "window_samples=True"), (dict(by_sample=True), "window_samples=True"),
                                      (dict(window_samples=True, cut_on="OBS"), "cut_on: PVAL or PVAL_SAMPLE"),
                                      (dict(window_samples=True, widths=[]), "at least one"),
                                      (dict(window_samples=True, max_muts_per_tile_per_sample=0), "max_muts_per_tile_per_sample")])
def test_window_hits_refuses_before_a_genome_is_packed_or_a_device_is_touched(kw, match):
    with pytest.raises(ValueError, match=match):
        _hits(**kw)


def test_window_hits_takes_the_sample_score_only_with_the_keyword():
    """With window_samples the refusal is passed: the call goes on to the genome, which does not exist."""
    with pytest.raises(Exception) as exc:
        _hits(window_samples=True, cut_on="PVAL_SAMPLE")
    assert "windows take no" not in str(exc.value) and "cut_on" not in str(exc.value)


# ---- the command line ----------------------------------------------------------------------------------------------------------
def _cli():
    spec = importlib.util.spec_from_file_location("dig_driver_cli_window_samples", os.path.join(ROOT, "scripts", "DigDriver.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BASE = "tileDriver g.fa --mutation-files a.bed b.bed --maps ma mb --outdir out --outpfx A B --fdr 0.1 "


def test_command_line_parses_the_option():
    cli = _cli()
    assert cli.parse_args(BASE).window_samples is False and cli.parse_args(BASE + "--window-tiles 2").window_samples is False
    a = cli.parse_args(BASE + "--window-tiles 3 1 --window-samples --cut-on PVAL_SAMPLE")
    assert a.window_samples is True and a.window_tiles == [3, 1] and a.cut_on == "PVAL_SAMPLE" and a.func is cli.cmd_tile
    with pytest.raises(SystemExit):
        cli.parse_args(BASE + "--window-tiles 2 --window-samples yes")


@pytest.mark.parametrize("options,match", [("--window-samples", "--window-samples needs --window-tiles"),
                                           ("--window-samples --by-sample", "--window-samples needs --window-tiles"),
                                           ("--window-samples --sparse", "--window-samples needs --window-tiles"),
                                           ("--window-tiles 2 --window-samples --sparse", "--window-tiles is not part of --sparse"),
                                           ("--window-tiles 2 --window-samples --by-sample", "--window-tiles does not take --by-sample"),
                                           ("--window-tiles 2 --cut-on PVAL_SAMPLE", "--window-samples"),
                                           ("--window-tiles 2 2 --window-samples", "distinct integers >= 1")])
def test_command_line_refusals_come_before_any_file_is_read(options, match):
    cli = _cli()
    with pytest.raises(SystemExit, match=match):
        cli.main(BASE + options)
    assert not os.path.exists("out")


def test_command_line_takes_the_sample_score_with_the_option():
    """--window-tiles 2 --window-samples --cut-on PVAL_SAMPLE passes every refusal: the command goes on to its maps, which do not exist."""
    cli = _cli()
    with pytest.raises(BaseException) as exc:
        cli.main(BASE + "--window-tiles 2 --window-samples --cut-on PVAL_SAMPLE")
    assert "--window-tiles" not in str(exc.value) and "--cut-on" not in str(exc.value)
    assert not os.path.exists("out")
