"""dig_tile_window_census / dig_sparse_window_count / dig_sparse_window_test and their `_host` twins called through `_lib.call` with
pointers carved from a guarded arena (tests/guarded_arena.py): every argument at exactly the alignment of its element and no more (the
census workspace at 8 bytes, with exactly the bytes its size query returns), outputs of exactly their sizes, 64 KiB of typed poison
around every buffer, twice (poison A / B): no band touched, outputs bit-identical between A and B and to the call on ordinary tensors,
and equal to the plain-Python statement.  R = 6 regions (tile_samples_cases), C = 3 and C = 65 (a second mask word in the census); the
window census with the census' n_positive (the shortcut) and without (the walk)."""
import numpy as np
import pytest

import guarded_arena as GA
from guarded_arena import guarded_runs, out
import sparse_tiles_cases as P
import sparse_tiles_statement as S1
import sparse_windows_statement as S
import tile_samples_cases as K

pytestmark = pytest.mark.gpu

NOKEY = np.iinfo(np.int64).max
R = len(K.IDX)


@pytest.fixture(scope="module")
def dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    return torch.device("cuda:0")


def arr(dtype, data, **kw):
    return GA.inp(dtype, np.ascontiguousarray(data, GA._NP[dtype]), **kw)


@pytest.mark.parametrize("C,n_up,binsize,width", [(3, 1, 50, 3), (65, 1, 50, 2), (3, 2, 1, 7), (65, 2, 7, 58), (3, 1, 1, 150)])
def test_every_entry_point_at_its_documented_alignments(C, n_up, binsize, width, dev):
    from digdriver_amd import _lib
    from digdriver_amd.data_tools.genome import PackedGenome
    seqs = K.genome_sequences()
    g = PackedGenome.from_sequences(seqs)
    regions = P.regions(K.IDX)
    tables = [P.s_prob(c, n_up) for c in range(C)]
    s_prob = np.array([[t[k] for k in sorted(t)] for t in tables])
    T = -(-400 // binsize)
    mu = np.random.default_rng(3).uniform(20.0, 90.0, (C, R))
    mu[0, 1] = np.nan
    sigma = 0.25 * mu
    rows = P.statement_rows(P.stacked(P.cohort_rows(C)))
    n_chrom = len(g.names)
    first, nval, denom, npos = S1.census(seqs, regions, tables, n_up, binsize, T)
    genome = dict(words=arr("u32", g.words), off=arr("i64", g.offsets, index=(0, int(g.offsets.max()))),
                  len=arr("i64", g.lengths, index=(0, int(g.lengths.max()))), reg_chrom=arr("i32", g.chrom_index([r[0] for r in regions]), index=(0, n_chrom - 1)),
                  reg_start=arr("i64", K.IDX[:, 1], index=(0, 2000)), reg_end=arr("i64", K.IDX[:, 2], index=(0, 2000)), s_prob=arr("f64", s_prob))
    head = lambda a: [a.ptr("words"), len(g.words), a.ptr("off"), a.ptr("len"), n_chrom, a.ptr("reg_chrom"), a.ptr("reg_start"),
                      a.ptr("reg_end"), R, a.ptr("s_prob"), C, n_up, binsize, T]
    wsb = int(_lib.load().dig_tile_census_workspace(C, n_up))
    assert wsb == (4 ** (2 * n_up + 1)) * 8 * -(-C // 64)
    want_nwin, want_npw = S.window_census(seqs, regions, tables, n_up, binsize, T, width)
    # the sorted keys of the mutated tiles, with what must be passed over: negative keys in front, a row >= C R and the all-ones key behind
    tiles = S1.mutated_tiles(seqs, regions, rows, tables, n_up, binsize, T)
    real = sorted((c * R + r) * T + t for (c, r, t), (k, _) in tiles.items() for _ in range(k))
    keys = np.array([-(1 << 62), -5] + real + [C * R * T + 3, NOKEY, NOKEY], np.int64)
    n = len(keys)
    want_counts, flat = S.counts_from_keys([int(k) for k in keys], T, [nval[row % R] for row in range(C * R)], width)
    offsets = np.concatenate([[0], np.cumsum(want_counts)]).astype(np.int64)
    total = int(offsets[-1])
    ref = S.mutated_window_table(seqs, regions, rows, tables, n_up, binsize, T, width)
    assert [(row // R, row % R, w) for row, w in flat] == sorted(ref) and total == len(ref) > 0
    begin, count = (3, total - 5) if total > 16 else (0, total)             # a chunk that starts and ends inside the list
    ints, reals = ("cohort", "region", "window", "k"), ("pt", "exp", "pval")
    for suffix, where in (("", dev), ("_host", "cpu")):
        device = where is dev
        last = (lambda: _lib.stream_ptr()) if device else (lambda: 0)
        # ---- the window census: with n_positive (the shortcut where it applies) and without (every region walked)
        for with_census in (True, False):
            bufs = dict(genome, n_windows=out("i32", R), n_positive_w=out("i32", (C, R)))
            if with_census:
                bufs["n_positive"] = arr("i32", npos, index=(0, T))
            if device:
                bufs["ws"] = GA.ws(wsb, align=8)
            got = guarded_runs(bufs, lambda a: _lib.call("dig_tile_window_census" + suffix, *head(a), width, a.ptr("n_positive"), a.ptr("n_windows"),
                                                         a.ptr("n_positive_w"), *([a.ptr("ws"), wsb] if device else []), last()),
                               device=where, what="dig_tile_window_census" + suffix, plain=True)
            assert got["n_windows"].tolist() == want_nwin and got["n_positive_w"].tolist() == want_npw, (suffix, with_census)
        # ---- the counts
        bufs = dict(keys=arr("i64", keys, index=(-5, int(NOKEY))), n_valid=arr("i32", nval, index=(0, T)), counts=out("i64", n))
        got = guarded_runs(bufs, lambda a: _lib.call("dig_sparse_window_count" + suffix, a.ptr("keys"), n, a.ptr("n_valid"), C, R, T, width,
                                                     a.ptr("counts"), last()),
                           device=where, what="dig_sparse_window_count" + suffix, plain=True)
        assert got["counts"].tolist() == want_counts, suffix
        # ---- the test of a chunk
        bufs = dict(genome, denom=arr("f64", np.array(denom)), mu=arr("f64", mu), sigma=arr("f64", sigma),
                    keys=arr("i64", keys, index=(-5, int(NOKEY))), offsets=arr("i64", offsets, index=(0, total)),
                    **{k: out("i32", count) for k in ints}, **{k: out("f64", count) for k in reals})
        got = guarded_runs(bufs, lambda a: _lib.call("dig_sparse_window_test" + suffix, *head(a), a.ptr("denom"), a.ptr("mu"), a.ptr("sigma"),
                                                     a.ptr("keys"), n, a.ptr("offsets"), width, begin, count, *[a.ptr(k) for k in ints + reals],
                                                     last()),
                           device=where, what="dig_sparse_window_test" + suffix, plain=True)
        wins = sorted(ref)[begin:begin + count]
        assert [(int(c), int(r), int(w)) for c, r, w in zip(got["cohort"], got["region"], got["window"])] == wins, suffix
        assert got["k"].tolist() == [ref[w][0] for w in wins]
        np.testing.assert_allclose(got["pt"], np.array([ref[w][1] for w in wins]), rtol=1e-12, atol=0, equal_nan=True)
        exp = got["pt"] * mu[[w[0] for w in wins], [w[1] for w in wins]]
        assert np.array_equal(got["exp"], exp, equal_nan=True)
        assert np.isfinite(got["pval"]).any()
    assert 1 <= max(want_counts) <= width and sum(c > 0 for c in want_counts) <= len(tiles)
    assert any(0 < p < v for row in npos for p, v in zip(row, nval)) or binsize == 50       # a region the shortcut does not take
