"""The pairs of the element route, the parts that need no GPU: the binding of dig_pair_bits, dig_pair_fisher, dig_pair_counts and
their `_host` twins, every refusal of the contract (include/dig_hip.h) before a device is touched, the numpy statement
(tests/pair_fisher_statement.py) against the exact values of tests/golden/pair_fisher_golden.npz and against scipy, pair_index
against a double loop, the plan and the ValueErrors of engine.pair_bits / engine.pair_fisher."""
import ctypes
import os

import numpy as np
import pytest

import pair_fisher_statement as S
from conftest import ROOT
from digdriver_amd import _lib, engine

NAMES = ("dig_pair_bits", "dig_pair_fisher", "dig_pair_counts")


def test_binding_facts():
    """The entry points and their twins are exported, declared and bound; a twin's signature is the entry point's with `device` for
    `stream`; the ABI version is the one of before; the constants are the header's."""
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dig_hip.h")).read()
    for name, n_args in zip(NAMES, (7, 18, 15)):
        for sym in (name, name + "_host"):
            assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym) and sym + "(" in header
        assert _lib._SIGNATURES[name][-1] is ctypes.c_void_p and _lib._SIGNATURES[name + "_host"][-1] is ctypes.c_int
        assert _lib._SIGNATURES[name + "_host"][:-1] == _lib._SIGNATURES[name][:-1] and len(_lib._SIGNATURES[name]) == n_args
    assert _lib._SIGNATURES["dig_pair_fisher"][10] is ctypes.c_int32 and _lib._SIGNATURES["dig_pair_fisher"][11] is ctypes.c_int32
    assert lib.dig_abi_version() == 12 and "#define DIG_ABI_VERSION 12" in header and _lib.ABI_VERSION == 12
    for name, value in (("MAX_SAMPLES", 65536), ("MAX_ROWS", 8192), ("TILE", 64), ("CHUNK_BITS", 2048)):
        assert getattr(engine, "PAIR_" + name) == value and "#define DIG_PAIR_%s %d\n" % (name, value) in header


def _aligned(n_words, offset=0):
    """A u64 array of n_words words whose first byte lies at `offset` (mod 16)."""
    raw = np.zeros(8 * n_words + 32, np.uint8)
    start = (-raw.ctypes.data) % 16 + offset
    return raw[start:start + 8 * n_words].view(np.uint64)


def _bits(suffix, row="r", sample="r", n_keys=1, H_total=1, W=2, bits="b"):
    arrays = dict(r=np.zeros(1, np.int32), b=_aligned(2), m=_aligned(2, 8))
    p = lambda v: None if v is None else _lib.host_ptr(arrays[v])
    return getattr(_lib.load(), "dig_pair_bits" + suffix)(p(row), p(sample), n_keys, H_total, W, p(bits), None if suffix == "" else 0)


def _fisher(name, suffix, bits="b", H_total=2, W=2, row_ptr="rp", n_samples="ns", pair_ptr="pp", C=1, tiles="t", n_tiles=1, n_pairs=1,
            n_max=64, h_max=2, lnfact="f", n_row="i", n_both="i", pval_cooccur="f", pval_exclusive="f"):
    arrays = dict(b=_aligned(4), m=_aligned(4, 8), rp=np.array([0, 2]), ns=np.array([64], np.int32), pp=np.array([0, 1]),
                  t=np.zeros(3, np.int32), f=np.zeros(65), i=np.zeros(2, np.int32))
    p = lambda v: None if v is None else _lib.host_ptr(arrays[v])
    head = (p(bits), H_total, W, p(row_ptr), p(n_samples), p(pair_ptr), C, p(tiles), n_tiles, n_pairs, n_max, h_max)
    outs = (p(lnfact), p(n_row), p(n_both), p(pval_cooccur), p(pval_exclusive)) if name == "dig_pair_fisher" else (p(n_row), p(n_both))
    return getattr(_lib.load(), name + suffix)(*head, *outs, None if suffix == "" else 0)


BITS_REFUSALS = [(dict(n_keys=-1), "n_keys, H_total >= 0"), (dict(H_total=-1), "n_keys, H_total >= 0"), (dict(W=3), "W even"), (dict(W=0), "W even"),
                 (dict(W=1026), "W even"), (dict(H_total=1 << 31), "fewer than 2^31 rows"), (dict(bits=None), "bits non-null and 16-byte aligned"),
                 (dict(bits="m"), "bits non-null and 16-byte aligned"), (dict(n_keys=1 << 39), "fewer than 2^39 rows or pairs"),
                 (dict(row=None), "non-null row, sample"), (dict(sample=None), "non-null row, sample")]

FISHER_REFUSALS = [(dict(H_total=-1), "n_max, h_max >= 0"), (dict(n_pairs=-1), "n_max, h_max >= 0"), (dict(n_max=-1), "n_max, h_max >= 0"),
                   (dict(n_max=65537, W=1026), "n_max <= 65 536 samples"), (dict(n_max=65537, W=1024), "n_max <= 65 536 samples"),
                   (dict(h_max=8193), "h_max <= 8 192 rows per cohort"), (dict(n_pairs=1 << 31), "fewer than 2^31 pairs per call"),
                   (dict(n_tiles=1 << 31), "fewer than 2^31 tiles"), (dict(W=3), "W even"), (dict(W=2, n_max=129), "W * 64 >= n_max"),
                   (dict(W=1026), "W even"), (dict(bits=None), "bits non-null and 16-byte aligned"),
                   (dict(bits="m"), "bits non-null and 16-byte aligned"), (dict(n_row=None), "non-null n_row"),
                   (dict(n_both=None), "non-null n_both")]
FISHER_ONLY = [(dict(lnfact=None), "non-null lnfact"), (dict(pval_cooccur=None), "non-null n_both, pval_cooccur, pval_exclusive"),
               (dict(pval_exclusive=None), "non-null n_both, pval_cooccur, pval_exclusive")]
PLAN_NULLS = [(dict(row_ptr=None), "non-null row_ptr"), (dict(n_samples=None), "non-null row_ptr"), (dict(pair_ptr=None), "non-null row_ptr"),
              (dict(tiles=None), "non-null")]


@pytest.mark.parametrize("suffix", ["", "_host"])
def test_every_refusal_comes_before_a_device_is_touched(suffix):
    """(Neither form gets as far as a launch or a staging copy: the pointers are host arrays, and this test runs without a GPU.)"""
    for kw, fragment in BITS_REFUSALS:
        assert _bits(suffix, **kw) == -1, kw
        assert fragment in _lib.last_error() and _lib.last_error().startswith("dig_pair_bits%s:" % suffix), (kw, _lib.last_error())
    assert _bits(suffix, H_total=0, bits=None, row=None, sample=None) == 0                  # nothing to do
    for name in ("dig_pair_fisher", "dig_pair_counts"):
        for kw, fragment in FISHER_REFUSALS + PLAN_NULLS + (FISHER_ONLY if name == "dig_pair_fisher" else []):
            assert _fisher(name, suffix, **kw) == -1, (name, kw)
            assert fragment in _lib.last_error() and _lib.last_error().startswith(name + suffix + ":"), (name, kw, _lib.last_error())


def test_the_twins_check_the_plan_arrays():
    lib = _lib.load()
    p = _lib.host_ptr
    bits, f, i = _aligned(6), np.zeros(65), np.zeros(3, np.int32)
    good = dict(rp=np.array([0, 3]), ns=np.array([64], np.int32), pp=np.array([0, 3]), t=np.zeros(3, np.int32))
    for bad, fragment in ((dict(rp=np.array([1, 3])), "row_ptr: 0 first"), (dict(rp=np.array([0, 2])), "row_ptr: 0 first"),
                          (dict(pp=np.array([0, 2])), "pair_ptr: 0 first"), (dict(ns=np.array([65], np.int32)), "0 <= n_samples <= n_max"),
                          (dict(ns=np.array([-1], np.int32)), "0 <= n_samples <= n_max"), (dict(t=np.array([1, 0, 0], np.int32)), "tiles:"),
                          (dict(t=np.array([0, 1, 0], np.int32)), "tiles:"), (dict(t=np.array([0, 0, 1], np.int32)), "tiles:")):
        a = dict(good, **bad)
        for name, outs in (("dig_pair_fisher_host", (p(f), p(i), p(i), p(f), p(f))), ("dig_pair_counts_host", (p(i), p(i)))):
            assert getattr(lib, name)(p(bits), 3, 2, p(a["rp"]), p(a["ns"]), p(a["pp"]), 1, p(a["t"]), 1, 3, 64, 3, *outs, 0) == -1
            assert fragment in _lib.last_error() and _lib.last_error().startswith(name + ":"), (bad, _lib.last_error())
    # a cohort with more rows than declared; pairs that are not H (H - 1) / 2
    for kw, fragment in ((dict(h_max=2), "rows of a cohort <= h_max"),):
        assert lib.dig_pair_counts_host(p(bits), 3, 2, p(good["rp"]), p(good["ns"]), p(good["pp"]), 1, p(good["t"]), 1, 3, 64, kw["h_max"],
                                        p(i), p(i), 0) == -1 and fragment in _lib.last_error()
    pp = np.array([0, 2, 3])
    assert lib.dig_pair_counts_host(p(bits), 3, 2, p(np.array([0, 2, 3])), p(np.array([64, 64], np.int32)), p(pp), 2, p(good["t"]), 1, 3, 64, 3,
                                    p(i), p(i), 0) == -1 and "H (H - 1) / 2 pairs per cohort" in _lib.last_error()


def test_the_statement_meets_the_golden_file_and_scipy():
    """The rule's evaluation in plain double against the exact integer values: the accuracy bound of the kernel test, on every table;
    scipy's two functions on the same tables; the special cases of the rule."""
    from scipy.stats import hypergeom
    g = np.load(os.path.join(ROOT, "tests", "golden", "pair_fisher_golden.npz"))
    n, r, k, a = (g[c].astype(np.int64) for c in "nrka")
    assert len(n) == 2119 and (n <= 12).sum() == 1819 and set(n[n > 12].tolist()) == {64, 100, 2800, 16384, 65536}
    lo, hi, mode = np.maximum(0, r + k - n), np.minimum(r, k), (r + 1) * (k + 1) // (n + 2)
    big = n > 12
    for what, sel in (("a = lo", a == lo), ("a = hi", a == hi), ("a at the mode", a == mode), ("a below the mode", a == mode - 1),
                      ("a above the mode", a == mode + 1), ("r = 0", r == 0), ("r = n", r == n), ("k = 0", k == 0), ("k = n", k == n),
                      ("a tail below 1e-250", np.minimum(g["pval_cooccur"], g["pval_exclusive"]) < 1e-250)):
        assert (sel & big).any() and sel.any(), what
    st = np.array([S.tails(*map(int, t)) for t in zip(n, r, k, a)])
    S.check_pvalues(st[:, 0], g["pval_cooccur"], "statement, PVAL_COOCCUR")
    S.check_pvalues(st[:, 1], g["pval_exclusive"], "statement, PVAL_EXCLUSIVE")
    S.check_pvalues(hypergeom.sf(a - 1, n, k, r), g["pval_cooccur"], "scipy hypergeom.sf")
    S.check_pvalues(hypergeom.cdf(a, n, k, r), g["pval_exclusive"], "scipy hypergeom.cdf")
    degenerate = (r == 0) | (k == 0) | (r == n) | (k == n)
    assert (st[degenerate] == 1.0).all() and (g["pval_cooccur"][degenerate] == 1.0).all() and (g["pval_exclusive"][degenerate] == 1.0).all()
    # a few tables again from scratch (the file is what the generator writes)
    for i in (0, 500, 1818, 1819, 1900, 2000, 2118):
        assert S.exact_tails(int(n[i]), int(r[i]), int(k[i]), int(a[i])) == (g["pval_cooccur"][i], g["pval_exclusive"][i])


def test_the_statement_builds_rows_and_counts():
    rng = np.random.default_rng(1)
    m = rng.random((7, 150)) < 0.3
    row, sample = np.nonzero(m)
    bits = S.bits_from_keys(np.concatenate([row, row[:9], [-1, 7]]), np.concatenate([sample, sample[:9], [3, 3]]), 7, 4)
    assert np.array_equal(bits, S.bits_from_bool(m, 4)) and np.array_equal(S.popcount(bits), m.sum(1))
    n_row, both, nrk = S.pair_counts(bits, [3, 0, 4], [150, 5, 160])
    want = [(m[i] & m[j]).sum() for lo, hi in ((0, 3), (3, 7)) for i in range(lo, hi) for j in range(i + 1, hi)]
    assert both.tolist() == want and nrk[:, 0].tolist() == [150] * 3 + [160] * 6 and nrk[3, 1] == m[3].sum() and nrk[3, 2] == m[4].sum()
    for t in ((10, 4, 5, 2), (10, 7, 8, 5), (1, 1, 1, 1), (12, 0, 3, 0)):
        rows = S.rows_of_table(*t)
        assert (rows.shape[1], rows[0].sum(), rows[1].sum(), (rows[0] & rows[1]).sum()) == t


def test_pair_index_against_a_double_loop():
    from digdriver_amd.sequence_model import nb_model
    for H in (2, 3, 64, 65, 129):
        slot = 0
        for i in range(H):
            for j in range(i + 1, H):
                assert engine.pair_index(i, j, H) == S.pair_index(i, j, H) == slot
                slot += 1
        assert slot == H * (H - 1) // 2
        i, j = np.triu_indices(H, 1)
        assert np.array_equal(engine.pair_index(i, j, H), np.arange(slot))
        t = nb_model.PairTests(H, 10, dict(n_row=None, n_both=None, pval_cooccur=None, pval_exclusive=None))
        assert np.array_equal(t.pair_index(j, i), np.arange(slot)) and t.pair_index(1, 0) == 0
        for bad in ((0, 0), (-1, 1), (0, H)):
            with pytest.raises(IndexError):
                t.pair_index(*bad)
    assert engine.pair_index(8190, 8191, 8192) == 8192 * 8191 // 2 - 1


def test_the_plan_and_the_engines_value_errors():
    plan = engine.pair_plan([65, 0, 1, 130], [70, 129, 40, 200])
    assert plan["row_ptr"].tolist() == [0, 65, 65, 66, 196] and plan["pair_ptr"].tolist() == [0, 2080, 2080, 2080, 2080 + 8385]
    assert (plan["n_max"], plan["h_max"], plan["W"], plan["n_pairs"]) == (200, 130, 4, 10465) and plan["tiles"].dtype == np.int32
    assert plan["tiles"].tolist() == [[0, 0, 0], [0, 0, 1], [0, 1, 1], [3, 0, 0], [3, 0, 1], [3, 0, 2], [3, 1, 1], [3, 1, 2], [3, 2, 2]]
    assert [engine.pair_words(n) for n in (0, 1, 64, 128, 129, 256, 257, 65536)] == [2, 2, 2, 2, 4, 4, 6, 1024]
    assert len(engine.pair_plan([8192], [64])["tiles"]) == 128 * 129 // 2
    with pytest.raises(ValueError, match="n_max <= 65 536 samples"):
        engine.pair_plan([3], [65537])
    with pytest.raises(ValueError, match="h_max <= 8 192 rows per cohort: a higher min_samples or a stricter cut"):
        engine.pair_plan([8193], [64])
    with pytest.raises(ValueError, match="fewer than 2\\^31 pairs per call"):
        engine.pair_plan([8192] * 65, [64] * 65)
    with pytest.raises(ValueError, match="one number >= 0 per cohort"):
        engine.pair_plan([3, 4], [64])
    with pytest.raises(ValueError, match="bits must be \\[3, 2\\]"):
        engine.pair_fisher(np.zeros((3, 4), np.uint64), [3], [64])
    with pytest.raises(ValueError, match="bits non-null and 16-byte aligned"):
        engine.pair_fisher(_aligned(6, 8).reshape(3, 2), [3], [64])
    for W in (0, 3, 1026):
        with pytest.raises(ValueError, match="W even, 2 <= W <= 1024"):
            engine.pair_bits([0], [0], 1, W)
    with pytest.raises(ValueError, match="one of each per key"):
        engine.pair_bits([0, 1], [0], 2, 2)
    # nothing to do: empty results of the right types, no device needed
    got = engine.pair_fisher(np.zeros((0, 2), np.uint64), [0, 0], [10, 20])
    assert got["n_row"].shape == (0,) and got["n_both"].dtype == np.int32 and got["pval_cooccur"].shape == (0,) and got["pair_ptr"].tolist() == [0, 0, 0]
    assert engine.pair_bits(np.zeros(0, np.int32), np.zeros(0, np.int32), 0, 2).shape == (0, 2)
    from digdriver_amd.sequence_model import nb_model
    with pytest.raises(ValueError, match="n_samples must be at least"):
        nb_model.pair_fisher_exact(np.zeros((2, 9), bool), n_samples=8)
    with pytest.raises(ValueError, match="a bit matrix needs n_samples"):
        nb_model.pair_fisher_exact(np.zeros((2, 2), np.uint64))
    assert nb_model.pair_fisher_exact(np.zeros((0, 9), bool)).pval_cooccur.shape == (0,)


def test_run_element_pairs_refuses_its_arguments_before_a_file_is_read():
    from digdriver_amd.driver_model import cohort_batch
    args = (["/nonexistent/a.txt", "/nonexistent/b.txt"], ["/nonexistent/a.h5", "/nonexistent/b.h5"], "/nonexistent/ed.h5", "elts")
    run = cohort_batch.run_element_pairs
    for kw in (dict(pair_fdr=0.1), dict(pair_fdr=0.1, pval_max=0.1, fdr=0.1)):
        with pytest.raises(ValueError, match="exactly one of pval_max and fdr"):
            run(*args, **kw)
    for kw in ({}, dict(pair_fdr=0.1, pair_pval_max=0.1)):
        with pytest.raises(ValueError, match="exactly one of pair_pval_max and pair_fdr"):
            run(*args, fdr=0.1, **kw)
    with pytest.raises(ValueError, match="cut_on: one of PVAL_SNV_BURDEN"):
        run(*args, fdr=0.1, pair_fdr=0.1, cut_on="PVAL")
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="min_samples: an integer >= 1"):
            run(*args, fdr=0.1, pair_fdr=0.1, min_samples=bad)
    for bad in ([10], [10, 0], [10, 2.5]):
        with pytest.raises(ValueError, match="n_samples: one integer >= 1 per cohort"):
            run(*args, fdr=0.1, pair_fdr=0.1, n_samples=bad)


def test_overlapping_pairs_and_the_inverse_of_pair_index():
    from digdriver_amd.driver_model import cohort_batch
    # elements 0 .. 5: blocks on chromosomes 1, 1, 1, 2, 2, 1; 2 shares one base with 0 and covers 1; 1 touches 0 without sharing a base;
    # 3 and 4 overlap on chromosome 2 through 3's second block; 5 lies in 0's gap, over the end of 1 and inside 2
    chrom = np.array([1, 1, 1, 2, 2, 1])
    blk_ptr = np.array([0, 2, 3, 4, 6, 7, 8])
    blk_start = np.array([100, 400, 200, 199, 100, 500, 550, 250])
    blk_end = np.array([200, 500, 300, 401, 150, 600, 560, 390])
    want = {(0, 2), (1, 2), (1, 5), (2, 5), (3, 4)}
    for listed in ([0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0], [2, 4, 0]):
        got = cohort_batch.overlapping_pairs(chrom, blk_ptr, blk_start, blk_end, listed)
        brute = sorted((i, j) for i in range(len(listed)) for j in range(i + 1, len(listed))
                       if tuple(sorted((listed[i], listed[j]))) in want)
        assert got.dtype == np.int64 and got.tolist() == [list(x) for x in brute], (listed, got)
    assert cohort_batch.overlapping_pairs(chrom, blk_ptr, blk_start, blk_end, [3]).shape == (0, 2)
    for H in (2, 3, 65, 8192):
        slot = np.arange(H * (H - 1) // 2) if H < 100 else np.array([0, 1, 8190, 8191, 33550335, 33550334, 12345678])
        i, j = cohort_batch._pair_rows_of(slot, H)
        assert ((0 <= i) & (i < j) & (j < H)).all() and np.array_equal(engine.pair_index(i, j, H), slot)


def test_element_cohorts_pairs_is_refused_before_a_cohort_file_is_read():
    from test_row_select_host import _cli
    cli = _cli()
    base = "elementCohorts /nonexistent/ed.h5 elts --outdir /nonexistent/out --mutation-files a.txt b.txt --maps a.h5 b.h5 --outpfx A B "
    a = cli.parse_args(base + "--pairs --fdr 0.1 --pairs-fdr 0.05 --pairs-min-samples 3 --pairs-n-samples 100 200")
    assert cli._pairs_options(a, 2) == dict(pair_pval_max=None, pair_fdr=0.05, min_samples=3, n_samples=[100, 200])
    a = cli.parse_args(base + "--pairs --pval-max 1e-3")
    assert cli._pairs_options(a, 2) == dict(pair_pval_max=None, pair_fdr=0.1, min_samples=1, n_samples=None)
    a = cli.parse_args(base + "--pairs --pval-max 1e-3 --pairs-pval-max 0.01")
    assert cli._pairs_options(a, 2) == dict(pair_pval_max=0.01, pair_fdr=None, min_samples=1, n_samples=None)
    assert cli._pairs_options(cli.parse_args(base), 2) is None
    for extra, match in (("--pairs", "--pairs needs exactly one of --fdr and --pval-max"),
                         ("--pairs --bonferroni 0.05 --power", "--pairs needs exactly one of --fdr and --pval-max"),
                         ("--pairs --fdr 0.1 --pval-max 0.1", "at most one of --pval-max and --fdr"),
                         ("--fdr 0.1 --pairs-fdr 0.1", "need --pairs"), ("--pairs-pval-max 0.1", "need --pairs"),
                         ("--fdr 0.1 --pairs-min-samples 2", "need --pairs"), ("--fdr 0.1 --pairs-n-samples 5 5", "need --pairs"),
                         ("--pairs --fdr 0.1 --pairs-fdr 0.1 --pairs-pval-max 0.1", "at most one of --pairs-fdr and --pairs-pval-max"),
                         ("--pairs --fdr 0.1 --pairs-fdr 0", "take a level within"), ("--pairs --fdr 0.1 --pairs-pval-max 1.5", "take a level within"),
                         ("--pairs --fdr 0.1 --pairs-min-samples 0", "--pairs-min-samples takes a count"),
                         ("--pairs --fdr 0.1 --pairs-n-samples 5", "--pairs-n-samples takes one sample count"),
                         ("--pairs --fdr 0.1 --pairs-n-samples 5 0", "--pairs-n-samples takes one sample count")):
        with pytest.raises(SystemExit, match=match):
            cli.main(base + extra)
    assert not os.path.exists("/nonexistent/out")
