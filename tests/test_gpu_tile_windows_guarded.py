"""dig_tile_window_test and its `_host` twin called through `_lib.call` with pointers carved from a guarded arena
(tests/guarded_arena.py; the twin's arena lies in host memory): every argument at exactly the alignment of its element and no more,
planes of exactly C R T elements (the entry point takes no scratch), 64 KiB of typed poison around every buffer, twice (poison A /
B): no band touched, outputs bit-identical between A and B and to the call on ordinary buffers; pt_w, k_w, n_windows equal the
plain-Python statement, pval_w and exp_w are dig_tiled_nb_test of them; with outputs NULL the others are what they were with all.
The shapes take both paths of tile_window_kernel: whole rows per workgroup with a last workgroup that is not full (T = 8, 200), and
chunks of a row with a halo that is cut at the row's end (T = 2 500: three chunks; width 1 024: the last chunk's halo does not exist)."""
import numpy as np
import pytest

import guarded_arena as GA
from guarded_arena import guarded_runs, out
import tile_windows_statement as S

pytestmark = pytest.mark.gpu

OUTS = ("pt_w", "k_w", "exp_w", "pval_w", "n_windows")


@pytest.fixture(scope="module")
def dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    return torch.device("cuda:0")


def arr(dtype, data, **kw):
    return GA.inp(dtype, np.ascontiguousarray(data, GA._NP[dtype]), **kw)


def _planes(C, R, T, seed):
    """Base planes as the front half leaves them: pt NaN and k 0 behind n_valid; regions without tiles, with all and with some."""
    rng = np.random.default_rng(seed)
    n_valid = rng.integers(1, T + 1, R).astype(np.int32)
    n_valid[0], n_valid[-1] = T, T - 1
    if R > 2:
        n_valid[1] = 0
    if R > 3:
        n_valid[2] = -2
    pt = rng.uniform(1e-4, 1e-2, (C, R, T))
    k = (rng.uniform(0, 1, (C, R, T)) < 0.05).astype(np.int32) * rng.integers(1, 4, (C, R, T)).astype(np.int32)
    behind = np.arange(T)[None, :] >= np.maximum(n_valid, 0)[:, None]
    pt[:, behind], k[:, behind] = np.nan, 0
    mu = rng.uniform(5.0, 50.0, (C, R))
    return pt, k, mu, 0.3 * mu, n_valid


@pytest.mark.parametrize("C,R,T,width", [(3, 6, 8, 3), (3, 6, 8, 9), (1, 7, 200, 10), (2, 3, 2500, 7), (1, 2, 2500, 1024)])
def test_both_entry_points_at_their_documented_alignments(C, R, T, width, dev):
    import torch
    from digdriver_amd import _lib, engine
    pt, k, mu, sigma, n_valid = _planes(C, R, T, seed=C * 1000 + T + width)
    want_pt, want_k, want_n = S.window_planes(pt, k, n_valid, width)
    up = lambda x: torch.as_tensor(x, device=dev)
    want_pval, want_exp = (x.cpu().numpy() for x in engine.tiled_nb_test(up(want_pt), up(want_k), up(mu), up(sigma)))
    ins = dict(pt=arr("f64", pt), k=arr("i32", k), mu=arr("f64", mu), sigma=arr("f64", sigma), n_valid=arr("i32", n_valid, index=(-2, T)))
    shapes = dict(pt_w=("f64", (C, R, T)), k_w=("i32", (C, R, T)), exp_w=("f64", (C, R, T)), pval_w=("f64", (C, R, T)), n_windows=("i32", (R,)))
    for entry, where in (("dig_tile_window_test", dev), ("dig_tile_window_test_host", "cpu")):
        last = (lambda: _lib.stream_ptr()) if where is dev else (lambda: 0)
        full = None
        for names in (OUTS, ("pval_w",), ("pt_w", "k_w"), ("n_windows",), ("exp_w", "k_w")):
            bufs = dict(ins, **{n: out(*shapes[n]) for n in names})
            got = guarded_runs(bufs, lambda g: _lib.call(entry, g.ptr("pt"), g.ptr("k"), g.ptr("mu"), g.ptr("sigma"), g.ptr("n_valid"), C, R, T,
                                                         width, *[g.ptr(n) for n in OUTS], last()),
                               device=where, what=entry + " " + "+".join(names), plain=True)
            if full is None:
                full = got
                assert GA.same_bits(got["pt_w"], want_pt) and GA.same_bits(got["k_w"], want_k) and GA.same_bits(got["n_windows"], want_n), entry
                assert GA.same_bits(got["pval_w"], want_pval) and GA.same_bits(got["exp_w"], want_exp), entry
            for n in names:
                assert GA.same_bits(got[n], full[n]), (entry, names, n)
    assert want_k.sum() > 0 and np.isfinite(want_pval).sum() > 0 and np.isnan(want_pt).sum() > 0 and (want_n[:-1] != want_n[1:]).any()
