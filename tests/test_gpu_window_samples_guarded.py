"""dig_tile_window_sample_keys, dig_tile_window_samples and their `_host` twins called through `_lib.call` with pointers carved from
a guarded arena (tests/guarded_arena.py; a twin's arena lies in host memory): every argument at exactly the alignment of its element
and no more, keys of exactly n and a plane of exactly C R T elements (the entry points take no scratch), 64 KiB of typed poison
around every buffer, twice (poison A / B): no band touched, outputs bit-identical between A and B and to the call on ordinary
buffers, and -- the fourth run of guarded_runs -- once on a side stream with the same bits.  The outputs equal the plain-Python
statement.  At the arena's alignment (4 mod 8) the scan takes its 4-byte form; on the ordinary buffers it takes the 16-byte form when
T is a multiple of 4 (T = 8, 200, 2 500) and the 4-byte form when not (T = 201, 2 501): both compiled forms, against each other.  The
keys hold what the kernels must pass over: negative keys, INT64_MAX, keys of a row >= C R and of tiles at or past n_valid; a run of
300 equal keys; a tile hit by every sample."""
import numpy as np
import pytest

import guarded_arena as GA
from guarded_arena import guarded_runs, out
import window_samples_statement as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    return torch.device("cuda:0")


def _case(C, R, T, n_samples, seed):
    """(n_valid i32 [R], n: dict (cohort, region, tile, sample) -> rows, the tile-major keys i64 -- unsorted, hostile ones among them)."""
    rng = np.random.default_rng(seed)
    n_valid = rng.integers(1, T + 1, R).astype(np.int32)
    n_valid[0], n_valid[-1] = T, T - 1
    if R > 2:
        n_valid[1] = 0
    if R > 3:
        n_valid[2] = -2
    n = {}
    for _ in range(40 * C * R):
        key = (int(rng.integers(0, C)), int(rng.integers(0, R)), int(rng.integers(0, T)), int(rng.integers(0, n_samples)))       # (tiles at or past n_valid too)
        n[key] = n.get(key, 0) + int(rng.integers(1, 4))
    n[(0, 0, min(3, T - 1), 0)] = 300                                    # a run longer than a wave and a workgroup
    for s in range(n_samples):                                           # one tile hit by every sample, and a burst of one sample
        n[(C - 1, 0, T // 2, s)] = 1
    for t in range(max(T - 12, 0), T):
        n[(C - 1, R - 1, t, n_samples - 1)] = 2
    sb = S.sample_bits(n_samples)
    keys = S.tile_major_keys(n, R, T, sb) + [-1, -(1 << 62), S.NO_KEY, S.NO_KEY, ((C * R * T) << sb) | 1]
    keys = np.array(keys, np.int64)[rng.permutation(len(keys))]
    return n_valid, n, keys


SHAPES = [(3, 6, 8, 3, 70), (3, 6, 8, 9, 5), (2, 5, 200, 2, 100), (1, 7, 201, 10, 6), (2, 3, 2500, 7, 9), (1, 2, 2501, 1024, 4)]


@pytest.mark.parametrize("C,R,T,width,n_samples", SHAPES)
def test_both_entry_points_at_their_documented_alignments(C, R, T, width, n_samples, dev):
    from digdriver_amd import _lib
    n_valid, n, keys = _case(C, R, T, n_samples, seed=C * 1000 + T + width)
    sb, slots = S.sample_bits(n_samples), C * R * T
    want_keys = np.array([S.rekey(int(k), T, sb, slots) for k in keys], np.int64)
    want = S.window_sample_planes(n, C, [int(v) for v in n_valid], T, width, marked=T > 300)
    # what dig_tile_window_samples must pass over, beside the real keys: a negative key, INT64_MAX, a row >= C R
    rows = C * R
    hostile = np.array([-5, -(1 << 62), (((rows + 1) << sb) | 1) * T, S.NO_KEY], np.int64)
    sorted_keys = np.sort(np.concatenate([want_keys, hostile]))
    top = int(S.NO_KEY)
    for suffix, where in (("", dev), ("_host", "cpu")):
        last = (lambda: _lib.stream_ptr()) if where is dev else (lambda: 0)
        bufs = dict(keys=GA.inp("i64", keys, index=(0, top)), keys_out=out("i64", (len(keys),), index=(0, top)))
        got = guarded_runs(bufs, lambda g: _lib.call("dig_tile_window_sample_keys" + suffix, g.ptr("keys"), len(keys), C, R, T, n_samples,
                                                     g.ptr("keys_out"), last()),
                           device=where, what="dig_tile_window_sample_keys" + suffix, plain=True)
        assert GA.same_bits(got["keys_out"], want_keys), suffix
        bufs = dict(keys=GA.inp("i64", sorted_keys, index=(0, top)), n_valid=GA.inp("i32", n_valid, index=(-2, T)), s_w=out("i32", (C, R, T)))
        got = guarded_runs(bufs, lambda g: _lib.call("dig_tile_window_samples" + suffix, g.ptr("keys"), len(sorted_keys), g.ptr("n_valid"), C, R, T,
                                                     n_samples, width, g.ptr("s_w"), last()),
                           device=where, what="dig_tile_window_samples" + suffix, plain=True)
        assert GA.same_bits(got["s_w"], want), (suffix, np.argwhere(got["s_w"] != want)[:5])
    assert want.max() >= n_samples and (want_keys == S.NO_KEY).sum() == 5 and (R <= 2 or not want[:, 1].any())
    nw_last = max(int(n_valid[-1]) - width + 1, 1)
    assert want[C - 1, R - 1, nw_last - 1] >= 1 and not want[:, R - 1, nw_last:].any()   # the burst reaches the last window; behind it: 0
