"""The sparse per-base scan, the parts that need no GPU: the plain-Python statement's hand-worked cases, the zero-tile floor against
the oracle's empty tiles, every refusal of nb_model_hits_sparse and of the `_host` twins before any device work, the bindings, and
the command line's errors."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
import sparse_tiles_cases as P
import sparse_tiles_statement as S
import tile_samples_cases as K
from digdriver_amd import _lib
from digdriver_amd.sequence_model import nb_model
from oracle import dig_oracle as O


# ---- the statement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.HAND_CASES))
def test_statement_hand_cases(name):
    h = S.HAND_CASES[name]
    a = (h["seqs"], h["regions"])
    first, nval, denom, npos = S.census(*a, h["tables"], h["n_up"], h["binsize"], h["n_tiles"])
    assert (first, nval, npos) == (h["first_pos"], h["n_valid"], h["n_positive"])
    assert denom == h["denom"]                                            # (sums of a few 1s and 2s: exact)
    assert S.mutated_tiles(*a, h["rows"], h["tables"], h["n_up"], h["binsize"], h["n_tiles"]) == h["tiles"]
    C = len(h["tables"])
    smax = [max(t.values()) for t in h["tables"]]
    floor = [S.zero_floor(denom[c], smax[c], h["mu"][c], h["sigma"][c], h["binsize"]) for c in range(C)]
    assert floor == pytest.approx(h["floor"], rel=1e-14)
    assert S.n_testable(*a, h["rows"], h["tables"], h["mu"], h["sigma"], h["n_up"], h["binsize"], h["n_tiles"]) == h["n_testable"]
    # the library's host-side floor is the statement's
    smin = [min([v for v in t.values() if v > 0] or [np.inf]) for t in h["tables"]]
    got, testable = nb_model.zero_tile_floor(denom, smax, smin, h["mu"], h["sigma"], h["binsize"], npos)
    assert list(got) == pytest.approx(h["floor"], rel=1e-14)
    assert testable.tolist() == [[S.testable_region(m, s) for m, s in zip(h["mu"][c], h["sigma"][c])] for c in range(C)]


def test_testable_regions_follow_the_nan_rule_of_the_test_at_k_zero():
    mu = np.array([[50.0, np.nan, 0.0, -3.0, 5.0, 5.0, 5.0, np.inf]])
    sigma = np.array([[5.0, 1.0, 1.0, 1.0, 0.0, np.nan, np.inf, 1.0]])
    want = [[True, False, False, False, False, False, False, False]]
    assert nb_model.testable_regions(mu, sigma).tolist() == want
    assert [[S.testable_region(m, s) for m, s in zip(mu[0], sigma[0])]] == want


def test_floor_refuses_a_region_whose_smallest_tile_rounds_p_to_one():
    # theta pt = 1e-19 / 1: 1 / (theta pt + 1) == 1, the dense p-value of such a tile is NaN although pt > 0
    with pytest.raises(ValueError, match="cannot be counted"):
        nb_model.zero_tile_floor([[1.0]], [1.0], [1e-3], [[1e16]], [[1e-3]], 1, [[5]])
    floor, _ = nb_model.zero_tile_floor([[1.0]], [1.0], [1e-3], [[1e16]], [[1e-3]], 1, [[0]])      # (no tile with pt > 0: nothing to count)
    assert floor[0] <= 1.0


# ---- the floor against the oracle's empty tiles -------------------------------------------------------------------------------
def _problem(which):
    seqs = K.genome_sequences()
    if which == "tile_samples":
        rows = [[r[:3] for r in rows] for rows in K.cohort_rows()]
        mu, sigma = K.mu_sigma()
        return seqs, K.IDX, [K.s_prob(c) for c in range(K.C)], rows, mu, sigma
    C = 4
    mu, sigma = P.mu_sigma(C)
    return seqs, P.IDX, [P.s_prob(c) for c in range(C)], P.cohort_rows(C), mu, sigma


@pytest.mark.parametrize("binsize", P.BINSIZES)
@pytest.mark.parametrize("which", ["tile_samples", "new"])
def test_floor_is_below_every_empty_testable_tile_of_the_oracle(which, binsize):
    seqs, idx, tables, rows, mu, sigma = _problem(which)
    regions = P.regions(idx)
    C = len(tables)
    n_tiles = max(1, -(-int((idx[:, 2] - idx[:, 1]).max()) // binsize))
    _, _, denom, _ = S.census(seqs, regions, tables, 1, binsize, n_tiles)
    keys = sorted(tables[0])
    seen = 0
    for c in range(C):
        floor = S.zero_floor(denom[c], max(tables[c].values()), mu[c], sigma[c], binsize)
        lowest = np.inf
        for r, (chrom, start, end) in enumerate(regions):
            if first_positions(seqs, regions[r]) == 0:
                continue
            starts = [s for ch, s, _ in rows[c] if ch == chrom]
            pv, _, obs, _, _ = O.apply_nb_to_region(seqs[chrom], np.array([tables[c][k] for k in keys]), start, end, mu[c][r], sigma[c][r],
                                                    starts, binsize)
            empty = pv[(obs == 0) & ~np.isnan(pv)]
            if len(empty):
                lowest = min(lowest, float(empty.min()))
                seen += len(empty)
        print("%s binsize %d cohort %d: floor %.6g, smallest empty-tile p-value %.6g" % (which, binsize, c, floor, lowest))
        assert floor <= lowest * (1 + 1e-12)
        if which == "tile_samples" and binsize == 1:
            assert floor == pytest.approx([0.745, 0.580, 0.669][c], abs=6e-4)      # (the floors the issue states for this problem)
    assert seen > 0 or binsize == 50                                              # (tile_samples at 50: every tile carries a row)


def first_positions(seqs, region):
    return S.region_positions(seqs, region, 1)[1]


# ---- refusals of nb_model_hits_sparse, all before a genome is packed or a device is touched -----------------------------------
def _hits(**kw):
    args = dict(d_prs=[K.s_prob(0)], idx=np.array([[1, 100, 500]]), mu=[[1.0]], sigma=[[1.0]], f_muts=["no such file"], f_fasta="no such fasta",
                n_up=1, n_down=1)
    args.update(kw)
    return nb_model.nb_model_hits_sparse(**args)


def test_refusals_of_the_function():
    for cuts in ({}, dict(pval_max=0.1, fdr=0.1), dict(fdr=0.1, bonferroni=0.05), dict(pval_max=0.1, fdr=0.1, bonferroni=0.05)):
        with pytest.raises(ValueError, match="exactly one of pval_max, fdr and bonferroni"):
            _hits(**cuts)
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"bonferroni: a level within \(0, 1\]"):
            _hits(bonferroni=bad)
    negative = dict(K.s_prob(0), ACG=-1e-4)
    with pytest.raises(ValueError, match="negative entry"):
        _hits(d_prs=[negative], pval_max=0.1)
    for up, down in ((1, 2), (3, 3), (0, 0)):
        with pytest.raises(NotImplementedError, match="n_up = n_down = 1 or 2"):
            _hits(n_up=up, n_down=down, pval_max=0.1)
    # what engine.check_tile_regions refuses (penta-nucleotide regions): too long, or starting inside (0, n_up)
    import itertools
    penta = {"".join(k): 1e-3 for k in itertools.product("ACGT", repeat=5)}
    with pytest.raises(ValueError, match="at most 16384 positions"):
        _hits(d_prs=[penta], n_up=2, n_down=2, idx=np.array([[1, 0, 20000]]), pval_max=0.1)
    with pytest.raises(ValueError, match="negative position"):
        _hits(d_prs=[penta], n_up=2, n_down=2, idx=np.array([[1, 1, 300]]), pval_max=0.1)
    with pytest.raises(TypeError):
        _hits(pval_max=0.1, by_sample=True)                                  # the sample options are no keywords of this function


# ---- the library: bindings and refusals, no device -----------------------------------------------------------------------------
NEW = ("dig_tile_census", "dig_sparse_tile_keys", "dig_sparse_tile_test")


def test_bindings_mirror_the_header():
    header = open(os.path.join(ROOT, "include", "dig_hip.h")).read()
    for name in NEW:
        assert name + "(" in header and name + "_host(" in header
        assert _lib._SIGNATURES[name][-1] is ctypes.c_void_p and _lib._SIGNATURES[name + "_host"][-1] is ctypes.c_int
        assert name in _lib.EXPORTED_SYMBOLS and name + "_host" in _lib.EXPORTED_SYMBOLS
    # a twin takes its entry point's arguments without the stream (and, for the census, without the workspace pair)
    assert _lib._SIGNATURES["dig_tile_census_host"][:-1] == _lib._SIGNATURES["dig_tile_census"][:-3]
    for name in NEW[1:]:
        assert _lib._SIGNATURES[name + "_host"][:-1] == _lib._SIGNATURES[name][:-1]
    assert [len(_lib._SIGNATURES[n]) for n in NEW] == [21, 14, 27]
    assert "dig_tile_census_workspace(" in header and "dig_tile_census_workspace" in _lib._SIZE_QUERIES
    lib = _lib.load()
    assert lib.dig_abi_version() == 12
    assert [lib.dig_tile_census_workspace(c, u) for c, u in ((0, 1), (3, 1), (64, 1), (65, 1), (37, 2), (65, 2), (3, 3), (-1, 1))] == \
        [512, 512, 512, 1024, 8192, 16384, 0, 0]


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
    census = lambda **kw: genome(**kw) + [buf, buf, buf, buf, 0]
    test = lambda keys=i64(0), n=1, **kw: genome(**kw) + [buf, buf, buf, keys, n] + [buf] * 7 + [0]
    for name, make in (("dig_tile_census_host", census), ("dig_sparse_tile_test_host", test)):
        _refused(name, make(n_up=3), "n_up = n_down = 1 or 2")
        _refused(name, make(binsize=0), "binsize >= 1")
        _refused(name, make(n_words=1), "n_words >= 2")
        _refused(name, make(C=1 << 31), "below 2^31")
        _refused(name, make(reg=(i32(1), i64(0), i64(40))), "regions inside the genome table")
        _refused(name, make(reg=(i32(0), i64(-5), i64(40))), "regions inside the genome table")
        _refused(name, make(length=100), "chromosomes inside the genome array")
        _refused(name, make(n_up=2, reg=(i32(0), i64(1), i64(30))), "would fetch from a negative position")
        _refused(name, make(n_up=2, reg=(i32(0), i64(0), i64(20000)), length=40), "at most 16 384 positions")
    _refused("dig_sparse_tile_test_host", test(n=-1), "0 <= n < 2^31")
    _refused("dig_sparse_tile_test_host", test(keys=i64(5, 3), n=2), "keys ascending")
    keys = lambda over: [buf, buf, 1, buf, 1, buf, buf, buf, 50] + over + [buf, 0]                   # ..., n_tiles, R, C, keys, device
    _refused("dig_sparse_tile_keys_host", keys([1 << 22, 1 << 22, 1 << 22]), "does not fit 62 bits")
    _refused("dig_sparse_tile_keys_host", keys([1 << 31, 1, 1]), "below 2^31")
    _refused("dig_sparse_tile_keys_host", keys([8, -1, 1]), "C, R, n_tiles >= 0")
    rows = [i64(0, 10), 2, i32(0, 0), buf, i32(1), 50, 8, 1, 1, buf, 0]
    _refused("dig_sparse_tile_keys_host", [i32(3), i32(0), 1] + rows, "pairs inside the mutation / region tables")
    _refused("dig_sparse_tile_keys_host", [i32(1), i32(4), 1] + rows, "pairs inside the mutation / region tables")
    rows[5] = 0
    _refused("dig_sparse_tile_keys_host", [i32(1), i32(0), 1] + rows, "binsize >= 1")
    # the accepting side without a device: nothing to do
    lib, p = _lib.load(), _lib.host_ptr(buf)
    assert lib.dig_sparse_tile_keys_host(p, p, 0, p, 1, p, p, p, 50, 1 << 20, 1 << 20, 1 << 20, p, 0) == 0


# ---- the command line ----------------------------------------------------------------------------------------------------------
def _cli():
    spec = importlib.util.spec_from_file_location("dig_driver_cli_sparse_tiles", os.path.join(ROOT, "scripts", "DigDriver.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BASE = "tileDriver g.fa --mutation-files a.bed b.bed --maps ma mb --outdir out --outpfx A B "


def test_command_line_parses_the_two_options():
    cli = _cli()
    a = cli.parse_args(BASE + "--fdr 0.1")
    assert a.sparse is False and a.bonferroni is None
    a = cli.parse_args(BASE + "--sparse --bonferroni 0.05 --binsize 1")
    assert a.sparse is True and a.bonferroni == 0.05 and a.pval_max is None and a.fdr is None and a.func is cli.cmd_tile


def test_command_line_refusals_come_before_any_file_is_read():
    cli = _cli()
    with pytest.raises(SystemExit, match="--bonferroni is valid only with --sparse"):
        cli.main(BASE + "--bonferroni 0.05")
    with pytest.raises(SystemExit, match="--bonferroni is valid only with --sparse"):
        cli.main(BASE + "--bonferroni 0.05 --pval-max 0.1")
    with pytest.raises(SystemExit, match="exactly one of --pval-max, --fdr and --bonferroni"):
        cli.main(BASE + "--sparse --fdr 0.1 --bonferroni 0.05")
    with pytest.raises(SystemExit, match="exactly one of --pval-max, --fdr and --bonferroni"):
        cli.main(BASE + "--sparse")
    with pytest.raises(SystemExit, match=r"--bonferroni takes a level within \(0, 1\]"):
        cli.main(BASE + "--sparse --bonferroni 2")
    for option in ("--max-muts-per-sample 500", "--max-muts-per-tile-per-sample 2", "--by-sample"):
        with pytest.raises(SystemExit, match="--sparse does not take the sample options"):
            cli.main(BASE + "--sparse --pval-max 0.1 " + option)
    with pytest.raises(SystemExit, match="exactly one of --pval-max and --fdr"):   # (without --sparse the text of before)
        cli.main(BASE + "--pval-max 0.1 --fdr 0.1")
    assert not os.path.exists("out")
