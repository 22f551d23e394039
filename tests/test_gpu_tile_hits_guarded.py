"""dig_tile_select_count / dig_tile_select_fill called through `_lib.call` with pointers carved from a guarded arena
(tests/guarded_arena.py, as tests/test_gpu_guarded_calls.py does for the other entry points): every argument at exactly the
alignment of its element and no more -- the score plane at 8 (mod 16), where the count pass's 16-byte loads start one element in --
64 KiB of typed poison around every buffer, twice (poison A / B): no band touched, outputs bit-identical between A and B and equal
to the call on ordinary tensors and to the numpy statement of the hit rule.  And offsets that are NOT the prefix sum: nothing
outside [0, total) may change."""
import numpy as np
import pytest

import guarded_arena as GA
from guarded_arena import GuardedArena, guarded_runs, out
from test_gpu_tile_hits import _expected, _plane

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    return torch.device("cuda:0")


def arr(dtype, data, **kw):
    return GA.inp(dtype, np.ascontiguousarray(data, GA._NP[dtype]), **kw)


def _inputs(shape, cut):
    C, R, T = shape
    score, nv, planes = _plane(shape, seed=7 + sum(shape))
    cut = np.asarray(cut, float)
    want, counts = _expected(score, nv, cut, planes)
    head = dict(score=arr("f64", score), n_valid=arr("i32", nv, index=(-1, T)), cut=arr("f64", cut))
    return head, planes, want, counts


def _fill_bufs(head, planes, offsets, total, n_slots):
    bufs = dict(head)
    bufs["offsets"] = arr("i64", offsets, index=(0, max(total, 1)))
    bufs.update(pt=arr("f64", planes["pt"]), exp_in=arr("f64", planes["exp"]), k=arr("i32", planes["k"]))
    bufs.update(hit_region=out("i32", n_slots), hit_tile=out("i32", n_slots), hit_score=out("f64", n_slots),
                hit_pt=out("f64", n_slots), hit_exp=out("f64", n_slots), hit_k=out("i32", n_slots))
    return bufs


def _call_fill(a, shape, total, skip=()):
    from digdriver_amd import _lib
    names = ("offsets", None, "pt", "exp_in", "k", "hit_region", "hit_tile", "hit_score", "hit_pt", "hit_exp", "hit_k")
    args = [total if n is None else (None if n in skip else a.ptr(n)) for n in names]
    _lib.call("dig_tile_select_fill", a.ptr("score"), a.ptr("n_valid"), a.ptr("cut"), *shape, *args, _lib.stream_ptr())


CASES = [((3, 70, 130), [0.3, np.inf, -1.0]), ((2, 9, 65), [np.nan, 0.3]), ((1, 3, 4100), [np.inf]), ((2, 9, 64), [0.3, 0.3])]


@pytest.mark.parametrize("shape,cut", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_count_and_fill_at_their_documented_alignments(shape, cut, dev):
    from digdriver_amd import _lib
    C, R, T = shape
    head, planes, want, want_counts = _inputs(shape, cut)
    bufs = dict(head, counts=out("i32", C * R))
    got = guarded_runs(bufs, lambda a: _lib.call("dig_tile_select_count", a.ptr("score"), a.ptr("n_valid"), a.ptr("cut"), C, R, T,
                                                 a.ptr("counts"), _lib.stream_ptr()),
                       device=dev, what="dig_tile_select_count", plain=True)
    assert np.array_equal(got["counts"], want_counts)
    offsets = np.cumsum(want_counts, dtype=np.int64) - want_counts
    total = int(want_counts.sum())
    assert total > 0
    bufs = _fill_bufs(head, planes, offsets, total, total)
    got = guarded_runs(bufs, lambda a: _call_fill(a, shape, total), device=dev, what="dig_tile_select_fill", plain=True)
    for name, key in (("hit_region", "region"), ("hit_tile", "tile"), ("hit_score", "score"), ("hit_pt", "pt"), ("hit_exp", "exp"), ("hit_k", "k")):
        assert got[name].tobytes() == want[key].tobytes(), name
    # planes and outputs that are NULL are skipped: the outputs left out keep their poison, the others are as before
    for variant in "AB":
        a = GuardedArena(bufs, variant, dev)
        _call_fill(a, shape, total, skip=("pt", "hit_exp", "hit_tile"))
        a.assert_intact("dig_tile_select_fill with NULL arguments (poison %s)" % variant)
        for name, key in (("hit_region", "region"), ("hit_score", "score"), ("hit_k", "k")):
            assert a.read(name).tobytes() == want[key].tobytes(), name
        for name in ("hit_pt", "hit_exp", "hit_tile"):
            b = bufs[name]
            assert GA.same_bits(a.read(name), np.full(b.shape, b.fill(variant), b.np)), name


def test_fill_with_offsets_that_are_not_the_prefix_sum_writes_only_inside_total(dev):
    """Offsets reversed, shifted below 0 and past total, constant and random, and a total smaller than the hits there are: no
    band around any buffer changes (the outputs hold exactly `total` slots, so a store outside [0, total) lands in a band)."""
    shape = (3, 70, 130)
    C, R, T = shape
    head, planes, want, want_counts = _inputs(shape, [0.3, np.inf, 0.3])
    right = np.cumsum(want_counts, dtype=np.int64) - want_counts
    total = int(want_counts.sum())
    rng = np.random.default_rng(2)
    wrong = [right[::-1].copy(), right - 1000, right + total - 50, np.zeros_like(right), np.full_like(right, total - 1),
             rng.integers(-5000, total + 5000, right.size), np.full_like(right, -(1 << 62)), np.full_like(right, (1 << 62))]
    for i, offsets in enumerate(wrong):
        for tot in (total, total // 3, 1):
            bufs = _fill_bufs(head, planes, offsets, tot, tot)
            bufs["offsets"] = arr("i64", offsets)                   # (values outside any domain, on purpose: no index poison)
            a = GuardedArena(bufs, "AB"[i % 2], dev)
            _call_fill(a, shape, tot)
            a.assert_intact("dig_tile_select_fill with wrong offsets (set %d, total %d)" % (i, tot))
    # the right offsets with a total that cuts the list short: the head of the list, nothing behind it
    cut_short = total // 2
    bufs = _fill_bufs(head, planes, right, cut_short, cut_short)
    a = GuardedArena(bufs, "A", dev)
    _call_fill(a, shape, cut_short)
    a.assert_intact("dig_tile_select_fill with a short total")
    assert a.read("hit_tile").tobytes() == want["tile"][:cut_short].tobytes()
    assert a.read("hit_score").tobytes() == want["score"][:cut_short].tobytes()
