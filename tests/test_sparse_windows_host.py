"""The sparse sliding-window scan, the parts that need no GPU: the plain-Python statement (hand-worked rows, the two interval
arguments against brute force, n_positive_w on the hand-worked genome), the bindings, every refusal of the `_host` twins and of
nb_model_window_hits_sparse before any device work or file, and the command line's errors."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
import sparse_tiles_statement as S1
import sparse_windows_statement as S
import tile_samples_cases as K
from digdriver_amd import _lib
from digdriver_amd.engine import SparseWindows, tile_window_census                            # the route the statement below states
from digdriver_amd.sequence_model.nb_model import nb_model_window_hits_sparse, zero_tile_floor


# ---- the statement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.HAND_ROWS))
def test_hand_worked_rows(name):
    h = S.HAND_ROWS[name]
    nv, m = h["nv"], h["m"]
    assert S.mutated_windows(h["tiles"], nv, m) == h["windows"]
    tiles = sorted(t for t in h["tiles"] if t < nv)
    assert [S.owned(p, t, nv, m) for p, t in zip([-1] + tiles, tiles)] == h["owned"]
    assert S.windows_by_owner(h["tiles"], nv, m) == sorted(h["windows"])
    assert {w: S.k_window(h["k"], w, nv, m) for w in h["windows"]} == h["k_w"]


def test_the_last_tile_of_a_row_next_to_the_first_tile_of_the_next():
    h = S.HAND_NEIGHBOUR_ROWS
    counts, flat = S.counts_from_keys(h["keys"], h["T"], h["nv"], h["m"])
    assert counts == h["counts"] and flat == h["windows"]
    # a run of equal keys counts once, at its head; keys outside the rows and tiles at or past nv count nowhere
    counts, flat = S.counts_from_keys([-3, 7, 7, 7, 8, 12, 16, 2 ** 63 - 1], 8, [8, 4], 3)
    assert counts == [0, 1, 0, 0, 1, 0, 0, 0] and flat == [(0, 5), (1, 0)]


def test_owners_name_every_mutated_window_once_and_the_run_form_counts_the_positive_windows():
    """Both interval arguments against brute force over random rows, nv < m among them."""
    rng = np.random.default_rng(5)
    short = 0
    for _ in range(3000):
        nv, m = int(rng.integers(0, 40)), int(rng.integers(1, 12))
        tiles = [int(t) for t in rng.integers(0, max(nv, 1) + 2, int(rng.integers(0, 10)))]          # (some at or past nv)
        want = S.mutated_windows(tiles, nv, m)
        assert S.windows_by_owner(tiles, nv, m) == sorted(want), (nv, m, tiles)
        assert S.positive_windows_runs(tiles, nv, m) == S.positive_windows_brute(tiles, nv, m) == len(want), (nv, m, tiles)
        short += 0 < nv < m
    assert short > 100


@pytest.mark.parametrize("binsize,n_tiles,width,n_win,n_pos_w", [
    # ACGNACGTAC, region 1:0-10: positions 1 .. 8, valid windows at 1, 5, 6, 7, 8; cohort 0 is positive at 1 and 5, cohort 1 at all five
    (2, 4, 1, 4, [2, 3]), (2, 4, 2, 3, [3, 3]), (2, 4, 4, 1, [1, 1]),
    # tiles = positions: cohort 0 has the tiles {0, 4}, cohort 1 {0, 4, 5, 6, 7}; the runs 1 .. 3 and 5 .. 7 hold two windows of 2 each
    (1, 8, 1, 8, [2, 5]), (1, 8, 2, 7, [3, 5]), (1, 8, 4, 5, [5, 5]),
    # room for two tiles of 3 only: fewer tiles than the width 4, one window
    (3, 2, 4, 1, [1, 1]), (3, 2, 2, 1, [1, 1]), (3, 2, 1, 2, [2, 2])])
def test_positive_windows_of_the_hand_worked_genome(binsize, n_tiles, width, n_win, n_pos_w):
    h = S1.HAND
    nwin, npw = S.window_census(h["seqs"], h["regions"], h["tables"], h["n_up"], binsize, n_tiles, width)
    assert nwin == [n_win] and [row[0] for row in npw] == n_pos_w
    if width == 1:
        assert [row[0] for row in npw] == [row[0] for row in S1.census(h["seqs"], h["regions"], h["tables"], h["n_up"], binsize, n_tiles)[3]]
    # the floor of a width is the sparse route's at binsize * width: no empty window's pt exceeds min(1, width binsize smax / denom)
    denom = S1.census(h["seqs"], h["regions"], h["tables"], h["n_up"], binsize, n_tiles)[2]
    smax = [max(t.values()) for t in h["tables"]]
    smin = [min(v for v in t.values() if v > 0) for t in h["tables"]]
    floor, _ = zero_tile_floor(denom, smax, smin, h["mu"], h["sigma"], binsize * width)
    want = [S1.zero_floor(denom[c], smax[c], h["mu"][c], h["sigma"][c], binsize * width) for c in range(2)]
    assert list(floor) == pytest.approx(want, rel=1e-14)
    for c in range(2):                                                     # and it is below every window's closed-form p-value
        alpha, theta = S1.gamma(h["mu"][c][0], h["sigma"][c][0])
        nv = min(-(-8 // binsize), n_tiles)
        for w in range(S.n_windows(nv, width)):
            pt = S.window_sum(h["seqs"], h["regions"][0], h["tables"][c], h["n_up"], binsize, w, nv, width) / denom[c][0]
            assert floor[c] <= (1.0 + theta * pt) ** -alpha * (1 + 1e-12)


def test_mutated_windows_of_the_hand_worked_genome():
    h = S1.HAND
    assert SparseWindows.NAMES == ("cohort", "region", "window", "k", "pt", "exp", "pval") and callable(tile_window_census)
    a = (h["seqs"], h["regions"], h["rows"], h["tables"], h["n_up"], h["binsize"], h["n_tiles"])
    # width 1: the mutated tiles themselves
    assert S.mutated_window_table(*a, 1) == h["tiles"]
    # width 2 at binsize 2 (tiles {1,2} {3,4} {5,6} {7,8}): cohort 0 has tile 2 -> windows 1, 2 with the C-centred windows at 5 (1 of
    # denom 2); cohort 1 has tile 1 -> windows 0 (positions 1 .. 4: one valid window, 2 of 10), 1 (3 .. 6: two)
    assert S.mutated_window_table(*a, 2) == {(0, 0, 1): (2, 0.5), (0, 0, 2): (2, 0.5), (1, 0, 0): (1, 0.2), (1, 0, 1): (1, 0.4)}
    # width 4 and more: one window over everything
    assert S.mutated_window_table(*a, 4) == S.mutated_window_table(*a, 5) == {(0, 0, 0): (2, 1.0), (1, 0, 0): (1, 1.0)}


# ---- the library: bindings and refusals, no device -----------------------------------------------------------------------------
NEW = ("dig_tile_window_census", "dig_sparse_window_count", "dig_sparse_window_test")


def test_bindings_mirror_the_header():
    header = open(os.path.join(ROOT, "include", "dig_hip.h")).read()
    for name in NEW:
        assert name + "(" in header and name + "_host(" in header
        assert _lib._SIGNATURES[name][-1] is ctypes.c_void_p and _lib._SIGNATURES[name + "_host"][-1] is ctypes.c_int
        assert name in _lib.EXPORTED_SYMBOLS and name + "_host" in _lib.EXPORTED_SYMBOLS
    # a twin takes its entry point's arguments without the stream (and, for the census, without the workspace pair)
    assert _lib._SIGNATURES["dig_tile_window_census_host"][:-1] == _lib._SIGNATURES["dig_tile_window_census"][:-3]
    for name in NEW[1:]:
        assert _lib._SIGNATURES[name + "_host"][:-1] == _lib._SIGNATURES[name][:-1]
    assert [len(_lib._SIGNATURES[n]) for n in NEW] == [21, 9, 31]
    # the 14 genome, region and table arguments are those of dig_tile_census / dig_sparse_tile_test
    assert _lib._SIGNATURES["dig_tile_window_census"][:14] == _lib._SIGNATURES["dig_tile_census"][:14]
    assert _lib._SIGNATURES["dig_sparse_window_test"][:19] == _lib._SIGNATURES["dig_sparse_tile_test"][:19]
    lib = _lib.load()
    assert lib.dig_abi_version() == 12 and "#define DIG_ABI_VERSION 12 " in header
    for name in NEW:
        assert hasattr(lib, name) and hasattr(lib, name + "_host")


def _refused(name, args, fragment):
    rc = getattr(_lib.load(), name)(*[_lib.host_ptr(a) if isinstance(a, np.ndarray) else a for a in args])
    msg = _lib.last_error()
    assert rc == -1 and name in msg and "requirement failed" in msg and fragment in msg, (name, rc, msg)


def test_host_twins_refuse_before_any_device_work():
    buf, i32, i64 = np.zeros(64, np.int64), lambda *v: np.array(v, np.int32), lambda *v: np.array(v, np.int64)
    words = np.zeros(8, np.uint32)
    # genome (words, n_words, off, len, n_chrom), regions (chrom, start, end, R), s_prob, C, n_up, binsize, n_tiles
    def genome(reg=(i32(0), i64(0), i64(40)), n_words=8, C=1, n_up=1, binsize=1, n_tiles=40, length=40):
        return [words, n_words, i64(0), i64(length), 1, reg[0], reg[1], reg[2], 1, buf.view(np.float64), C, n_up, binsize, n_tiles]
    census = lambda width=2, **kw: genome(**kw) + [width, buf, buf, buf, 0]
    test = lambda keys=i64(0), n=1, offsets=i64(0, 1), width=2, w_begin=0, w_count=1, **kw: \
        genome(**kw) + [buf, buf, buf, keys, n, offsets, width, w_begin, w_count] + [buf] * 7 + [0]
    for name, make in (("dig_tile_window_census_host", census), ("dig_sparse_window_test_host", test)):
        _refused(name, make(n_up=3), "n_up = n_down = 1 or 2")
        _refused(name, make(binsize=0), "binsize >= 1")
        _refused(name, make(n_words=1), "n_words >= 2")
        _refused(name, make(C=1 << 31), "below 2^31")
        _refused(name, make(reg=(i32(1), i64(0), i64(40))), "regions inside the genome table")
        _refused(name, make(length=100), "chromosomes inside the genome array")
        _refused(name, make(n_up=2, reg=(i32(0), i64(1), i64(30))), "would fetch from a negative position")
        _refused(name, make(n_up=2, reg=(i32(0), i64(0), i64(20000)), length=40), "at most 16 384 positions")
        for width in (0, -1, 2049):
            _refused(name, make(width=width), "1 <= width <= DIG_TILE_WINDOW_MAX_WIDTH")
    _refused("dig_sparse_window_test_host", test(n=-1), "n, w_begin >= 0")
    _refused("dig_sparse_window_test_host", test(w_begin=-1), "n, w_begin >= 0")
    _refused("dig_sparse_window_test_host", test(w_count=1 << 31), "w_count < 2^31")
    _refused("dig_sparse_window_test_host", test(keys=i64(5, 3), n=2, offsets=i64(0, 1, 2), w_count=2), "keys ascending")
    _refused("dig_sparse_window_test_host", test(offsets=i64(1, 2)), "offsets: the exclusive prefix sum")
    _refused("dig_sparse_window_test_host", test(keys=i64(3, 5), n=2, offsets=i64(0, 2, 1)), "offsets: the exclusive prefix sum")
    count = lambda keys=i64(0), n=1, C=1, R=1, T=40, width=2: [keys, n, i32(40), C, R, T, width, buf, 0]
    for width in (0, 2049):
        _refused("dig_sparse_window_count_host", count(width=width), "1 <= width <= DIG_TILE_WINDOW_MAX_WIDTH")
    _refused("dig_sparse_window_count_host", count(n=-1), "n >= 0")
    _refused("dig_sparse_window_count_host", count(T=1 << 31), "fewer than 2^31 tiles")
    _refused("dig_sparse_window_count_host", count(C=1 << 16, R=1 << 16), "C R below 2^31")
    _refused("dig_sparse_window_count_host", count(keys=i64(5, 3), n=2), "keys ascending")
    # the accepting side without a device: nothing to do
    lib, p = _lib.load(), _lib.host_ptr(buf)
    assert lib.dig_sparse_window_count_host(p, 0, p, 1 << 10, 1 << 10, 1 << 20, 2048, p, 0) == 0
    assert lib.dig_sparse_window_test_host(*[_lib.host_ptr(a) if isinstance(a, np.ndarray) else a for a in test(w_count=0)]) == 0
    empty = genome()
    empty[8] = 0                                                           # R = 0
    assert lib.dig_tile_window_census_host(*[_lib.host_ptr(a) if isinstance(a, np.ndarray) else a for a in empty + [3, buf, buf, buf, 0]]) == 0


# ---- refusals of nb_model_window_hits_sparse, all before a genome is packed or a file is opened ----------------------------------
def _hits(**kw):
    args = dict(d_prs=[K.s_prob(0)], idx=np.array([[1, 100, 500]]), mu=[[1.0]], sigma=[[1.0]], f_muts=["no such file"], f_fasta="no such fasta",
                n_up=1, n_down=1)
    args.update(kw)
    return nb_model_window_hits_sparse(**args)


def test_refusals_of_the_function():
    from digdriver_amd import engine
    for cuts in ({}, dict(pval_max=0.1, fdr=0.1), dict(fdr=0.1, bonferroni=0.05), dict(pval_max=0.1, fdr=0.1, bonferroni=0.05)):
        with pytest.raises(ValueError, match="exactly one of pval_max, fdr and bonferroni"):
            _hits(**cuts)
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"bonferroni: a level within \(0, 1\]"):
            _hits(bonferroni=bad)
    with pytest.raises(ValueError, match="at least one window width"):
        _hits(pval_max=0.1, widths=())
    for bad in ((0,), (2, -1), (1.5,), (True,), ("3",), (float("nan"),)):
        with pytest.raises(ValueError, match="every width an integer >= 1"):
            _hits(pval_max=0.1, widths=bad)
    with pytest.raises(ValueError, match="width 3 is given twice"):
        _hits(pval_max=0.1, widths=(3, 2, 3))
    assert engine.TILE_WINDOW_MAX_WIDTH == 2048
    with pytest.raises(ValueError, match="at most 2048 tiles"):
        _hits(pval_max=0.1, widths=(2, 2049))
    negative = dict(K.s_prob(0), ACG=-1e-4)
    with pytest.raises(ValueError, match="negative entry"):
        _hits(d_prs=[negative], pval_max=0.1)
    for up, down in ((1, 2), (3, 3), (0, 0)):
        with pytest.raises(ValueError, match="n_up = n_down = 1 or 2"):
            _hits(n_up=up, n_down=down, pval_max=0.1)
    for option in ("by_sample", "max_muts_per_sample", "max_muts_per_tile_per_sample", "cut_on", "window_samples"):
        with pytest.raises(TypeError):
            _hits(pval_max=0.1, **{option: 1})                               # the sample options are no keywords of this function


# ---- the command line ----------------------------------------------------------------------------------------------------------
def _cli():
    spec = importlib.util.spec_from_file_location("dig_driver_cli_sparse_windows", os.path.join(ROOT, "scripts", "DigDriver.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BASE = "tileDriver g.fa --mutation-files a.bed b.bed --maps ma mb --outdir out --outpfx A B "


def test_command_line_parses_the_option():
    cli = _cli()
    assert cli.parse_args(BASE + "--fdr 0.1").sparse_windows is None
    a = cli.parse_args(BASE + "--sparse --sparse-windows 3 1 10 --bonferroni 0.05 --binsize 1")
    assert a.sparse_windows == [3, 1, 10] and a.sparse is True and a.window_tiles is None and a.func is cli.cmd_tile
    for bad in ("--sparse-windows", "--sparse-windows 1.5", "--sparse-windows x"):
        with pytest.raises(SystemExit):
            cli.parse_args(BASE + "--sparse --pval-max 0.1 " + bad)


@pytest.mark.parametrize("options,match", [
    ("--sparse-windows 2 --pval-max 0.1", "--sparse-windows needs --sparse"),
    ("--sparse --sparse-windows 2 --window-tiles 2 --pval-max 0.1", "--sparse-windows does not go with --window-tiles"),
    ("--sparse-windows 2 --window-tiles 2 --pval-max 0.1", "--sparse-windows needs --sparse"),
    ("--sparse --sparse-windows 2 --window-samples --pval-max 0.1", "--sparse-windows does not take --window-samples"),
    ("--sparse --sparse-windows 2 --pval-max 0.1 --max-muts-per-sample 500", "--sparse-windows does not take the sample options"),
    ("--sparse --sparse-windows 2 --pval-max 0.1 --max-muts-per-tile-per-sample 2", "--sparse-windows does not take the sample options"),
    ("--sparse --sparse-windows 2 --pval-max 0.1 --by-sample", "--sparse-windows does not take the sample options"),
    ("--sparse --sparse-windows 2 --pval-max 0.1 --cut-on PVAL_SAMPLE", "--sparse-windows does not take the sample options"),
    ("--sparse --sparse-windows 2 0 --pval-max 0.1", "--sparse-windows takes distinct integers >= 1"),
    ("--sparse --sparse-windows 2 2 --pval-max 0.1", "--sparse-windows takes distinct integers >= 1"),
    ("--sparse --sparse-windows 2", "exactly one of --pval-max, --fdr and --bonferroni"),
    ("--sparse --sparse-windows 2 --fdr 0.1 --bonferroni 0.05", "exactly one of --pval-max, --fdr and --bonferroni"),
    ("--sparse --sparse-windows 2 --bonferroni 2", r"--bonferroni takes a level within \(0, 1\]")])
def test_command_line_refusals_come_before_any_file_is_read(options, match):
    with pytest.raises(SystemExit, match=match):
        _cli().main(BASE + options)
    assert not os.path.exists("out")


def test_window_tiles_with_sparse_is_refused_with_the_text_of_before():
    with pytest.raises(SystemExit) as exc:
        _cli().main(BASE + "--sparse --window-tiles 2 --pval-max 0.1")
    assert str(exc.value).startswith("ERROR: --window-tiles is not part of --sparse (the sparse scan tests single tiles)")
    assert "--sparse-windows" in str(exc.value) and not os.path.exists("out")
