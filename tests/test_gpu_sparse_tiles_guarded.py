"""dig_tile_census / dig_sparse_tile_keys / dig_sparse_tile_test called through `_lib.call` with pointers carved from a guarded
arena (tests/guarded_arena.py): every argument at exactly the alignment of its element and no more (the census workspace at 8 bytes,
with exactly the bytes its size query returns), outputs of exactly their sizes, 64 KiB of typed poison around every buffer, twice
(poison A / B): no band touched, outputs bit-identical between A and B and to the call on ordinary tensors, and equal to the
plain-Python statement.  R = 6 regions (tile_samples_cases), C = 3 and C = 65 (a second mask word in the census)."""
import numpy as np
import pytest

import guarded_arena as GA
from guarded_arena import guarded_runs, out
import sparse_tiles_cases as P
import sparse_tiles_statement as S
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


def _pairs(st):
    """The (row, region) pairs of the join, row-major, made on the host."""
    pm, pr = [], []
    for i in range(len(st["start"])):
        for r, (c, s, e) in enumerate(K.IDX):
            if st["chrom"][i] == str(c) and st["start"][i] < e and st["end"][i] > s:
                pm.append(i), pr.append(r)
    return np.array(pm, np.int32), np.array(pr, np.int32)


@pytest.mark.parametrize("C,n_up,binsize", [(3, 1, 50), (65, 1, 50), (3, 2, 1), (65, 2, 7)])
def test_every_entry_point_at_its_documented_alignments(C, n_up, binsize, dev):
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
    st = P.stacked(P.cohort_rows(C))
    n_mut = len(st["start"])
    n_chrom = len(g.names)
    genome = dict(words=arr("u32", g.words), off=arr("i64", g.offsets, index=(0, int(g.offsets.max()))),
                  len=arr("i64", g.lengths, index=(0, int(g.lengths.max()))), reg_chrom=arr("i32", g.chrom_index([r[0] for r in regions]), index=(0, n_chrom - 1)),
                  reg_start=arr("i64", K.IDX[:, 1], index=(0, 2000)), reg_end=arr("i64", K.IDX[:, 2], index=(0, 2000)), s_prob=arr("f64", s_prob))
    head = lambda a: [a.ptr("words"), len(g.words), a.ptr("off"), a.ptr("len"), n_chrom, a.ptr("reg_chrom"), a.ptr("reg_start"),
                      a.ptr("reg_end"), R, a.ptr("s_prob"), C, n_up, binsize, T]
    # ---- census: the workspace has exactly the bytes of the size query, at 8 bytes and no more
    wsb = int(_lib.load().dig_tile_census_workspace(C, n_up))
    assert wsb == (4 ** (2 * n_up + 1)) * 8 * -(-C // 64)
    bufs = dict(genome, first_pos=out("i64", R), n_valid=out("i32", R), denom=out("f64", (C, R)), n_positive=out("i32", (C, R)),
                ws=GA.ws(wsb, align=8))
    got = guarded_runs(bufs, lambda a: _lib.call("dig_tile_census", *head(a), a.ptr("first_pos"), a.ptr("n_valid"), a.ptr("denom"),
                                                 a.ptr("n_positive"), a.ptr("ws"), wsb, _lib.stream_ptr()),
                       device=dev, what="dig_tile_census", plain=True)
    first, nval, denom, npos = S.census(seqs, regions, tables, n_up, binsize, T)
    assert got["first_pos"].tolist() == first and got["n_valid"].tolist() == nval and got["n_positive"].tolist() == npos
    np.testing.assert_allclose(got["denom"], np.array(denom), rtol=1e-12, atol=0)
    # ---- keys
    pm, pr = _pairs(st)
    n = len(pm)
    rows = P.statement_rows(st)
    want_keys = np.full(n, NOKEY, np.int64)
    for i, (m, r) in enumerate(zip(pm, pr)):
        at = S.pair_tile(rows[m], regions[r], first[r], nval[r], binsize, T, C)
        if at is not None:
            want_keys[i] = (at[0] * R + r) * T + at[1]
    bufs = dict(pair_mut=arr("i32", pm, index=(0, n_mut - 1)), pair_reg=arr("i32", pr, index=(0, R - 1)), mut_start=arr("i64", st["start"]),
                mut_cohort=arr("i32", st["cohort"], index=(0, C - 1)), first_pos=arr("i64", first), n_valid=arr("i32", nval, index=(0, T)),
                keys=out("i64", n))
    got = guarded_runs(bufs, lambda a: _lib.call("dig_sparse_tile_keys", a.ptr("pair_mut"), a.ptr("pair_reg"), n, a.ptr("mut_start"), n_mut,
                                                 a.ptr("mut_cohort"), a.ptr("first_pos"), a.ptr("n_valid"), binsize, T, R, C, a.ptr("keys"),
                                                 _lib.stream_ptr()),
                       device=dev, what="dig_sparse_tile_keys", plain=True)
    assert np.array_equal(got["keys"], want_keys) and (want_keys == NOKEY).sum() >= 2
    # ---- test: sorted keys with one negative key in front (passed over like the all-ones keys behind)
    keys = np.concatenate([[-5], np.sort(want_keys)]).astype(np.int64)
    n = len(keys)
    ints, reals = ("cohort", "region", "tile", "k"), ("pt", "exp", "pval")
    bufs = dict(genome, denom=arr("f64", got_denom := np.array(denom)), mu=arr("f64", mu), sigma=arr("f64", sigma),
                keys=arr("i64", keys, index=(-5, int(NOKEY))), **{k: out("i32", n) for k in ints}, **{k: out("f64", n) for k in reals})
    got = guarded_runs(bufs, lambda a: _lib.call("dig_sparse_tile_test", *head(a), a.ptr("denom"), a.ptr("mu"), a.ptr("sigma"), a.ptr("keys"), n,
                                                 *[a.ptr(k) for k in ints + reals], _lib.stream_ptr()),
                       device=dev, what="dig_sparse_tile_test", plain=True)
    ref = S.mutated_tiles(seqs, regions, rows, tables, n_up, binsize, T)
    heads = np.flatnonzero(got["k"] > 0)
    tiles = [(int(got["cohort"][i]), int(got["region"][i]), int(got["tile"][i])) for i in heads]
    assert tiles == sorted(ref) and got["k"][heads].tolist() == [ref[t][0] for t in tiles]
    assert [int(keys[i]) for i in heads] == [(c * R + r) * T + t for c, r, t in tiles]           # written at the run head's own index
    np.testing.assert_allclose(got["pt"][heads], np.array([ref[t][1] for t in tiles]), rtol=1e-12, atol=0)
    rest = np.setdiff1d(np.arange(n), heads)
    assert len(rest) > 0 and all((got[k][rest] == -1).all() for k in ints[:3]) and (got["k"][rest] == 0).all()
    assert all(np.isnan(got[k][rest]).all() for k in reals)
    exp = got["pt"][heads] * mu[[t[0] for t in tiles], [t[1] for t in tiles]]
    assert np.array_equal(got["exp"][heads], exp, equal_nan=True)
    assert got_denom.shape == (C, R) and got["k"].max() >= 300
