"""dig_row_select_count / dig_row_select_fill / dig_row_scatter and their `_host` twins called through `_lib.call` with pointers carved
from a guarded arena (tests/guarded_arena.py; the twins' arena lies in host memory), on a side stream as well: every argument at
exactly the alignment of its element and no more -- the score plane and the output plane at 8 (mod 16), where the 16-byte loads and
stores start one element in --, counts and offsets of exactly the elements dig_row_select_counts_size returns, the lists of exactly
`total` slots, 64 KiB of typed poison around every buffer, twice (poison A / B): no band touched, outputs bit-identical between A and
B, equal to the call on ordinary buffers and to the numpy statement (tests/row_select_statement.py).  And, for the device entry
points, offsets that are NOT the prefix sum: nothing outside [0, total) may change."""
import numpy as np
import pytest

import guarded_arena as GA
import row_select_statement as S
from guarded_arena import GuardedArena, guarded_runs, out
from test_tile_hits_host import _random_list

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    return torch.device("cuda:0")


def arr(dtype, data, **kw):
    return GA.inp(dtype, np.ascontiguousarray(data, GA._NP[dtype]), **kw)


def _case(rows, n, cut, seed):
    rng = np.random.default_rng(seed)
    score = np.stack([_random_list(rng, n) for _ in range(rows)])
    cut = np.asarray(cut, float)
    return score, cut, dict(score=arr("f64", score), cut=arr("f64", cut))


def _K():
    from digdriver_amd import _lib
    return int(_lib.load().dig_row_select_chunk())


CASES = [(3, "2K+7", [0.3, np.inf, -1.0]), (2, 65, [np.nan, 0.3]), (1, "K+1", [np.inf]), (4, "K", [0.3, 0.3, np.inf, 0.05])]


@pytest.mark.parametrize("rows,n,cut", CASES, ids=lambda v: str(v) if not isinstance(v, list) else None)
def test_the_three_entry_points_and_their_twins_at_their_documented_alignments(rows, n, cut, dev):
    from digdriver_amd import _lib
    K = _K()
    n = {"2K+7": 2 * K + 7, "K+1": K + 1, "K": K}.get(n, n)
    score, cut, head = _case(rows, n, cut, 5 + rows)
    slots = int(_lib.load().dig_row_select_counts_size(rows, n))
    assert slots == rows * -(-n // K)
    want_counts = S.counts(score, cut, K)
    want_index, want_score, _ = S.fill(score, cut)
    offsets = np.cumsum(want_counts, dtype=np.int64) - want_counts
    total = int(want_counts.sum())
    assert total > 0
    values = np.arange(total, dtype=np.float64) + 0.5
    for suffix, where in (("", dev), ("_host", "cpu")):
        last = (lambda: _lib.stream_ptr()) if where is dev else (lambda: 0)
        bufs = dict(head, counts=out("i32", slots))
        got = guarded_runs(bufs, lambda a: _lib.call("dig_row_select_count" + suffix, a.ptr("score"), a.ptr("cut"), rows, n, a.ptr("counts"),
                                                     last()),
                           device=where, what="dig_row_select_count" + suffix, plain=True)
        assert np.array_equal(got["counts"], want_counts)
        bufs = dict(head, offsets=arr("i64", offsets, index=(0, total)), hit_index=out("i32", total), hit_score=out("f64", total))
        got = guarded_runs(bufs, lambda a: _lib.call("dig_row_select_fill" + suffix, a.ptr("score"), a.ptr("cut"), rows, n, a.ptr("offsets"),
                                                     total, a.ptr("hit_index"), a.ptr("hit_score"), last()),
                           device=where, what="dig_row_select_fill" + suffix, plain=True)
        assert np.array_equal(got["hit_index"], want_index) and got["hit_score"].tobytes() == want_score.tobytes()
        bufs = dict(head, offsets=arr("i64", offsets, index=(0, total)), values=arr("f64", values), out=out("f64", (rows, n)))
        got = guarded_runs(bufs, lambda a: _lib.call("dig_row_scatter" + suffix, a.ptr("score"), a.ptr("cut"), rows, n, a.ptr("offsets"),
                                                     total, a.ptr("values"), -2.0, a.ptr("out"), last()),
                           device=where, what="dig_row_scatter" + suffix, plain=True)
        assert got["out"].tobytes() == S.scatter(score, cut, values, -2.0).tobytes()
    # an output of the fill that is NULL is skipped: the other one is as before
    for variant in "AB":
        bufs = dict(head, offsets=arr("i64", offsets, index=(0, total)), hit_index=out("i32", total), hit_score=out("f64", total))
        a = GuardedArena(bufs, variant, dev)
        _lib.call("dig_row_select_fill", a.ptr("score"), a.ptr("cut"), rows, n, a.ptr("offsets"), total, None, a.ptr("hit_score"), _lib.stream_ptr())
        a.assert_intact("dig_row_select_fill without hit_index (poison %s)" % variant)
        assert a.read("hit_score").tobytes() == want_score.tobytes()
        b = bufs["hit_index"]
        assert GA.same_bits(a.read("hit_index"), np.full(b.shape, b.fill(variant), b.np))


def test_fill_and_scatter_with_offsets_that_are_not_the_prefix_sum_touch_only_their_arguments(dev):
    """Offsets reversed, shifted below 0 and past total, constant and random, and a total smaller than the selection: no band around
    any buffer changes (the lists hold exactly `total` slots, so a store or a load outside [0, total) lies in a band), and the
    scatter still writes every element of out: a value of the list or the fill."""
    from digdriver_amd import _lib
    K = _K()
    rows, n = 3, 2 * K + 7
    score, cut, head = _case(rows, n, [0.3, np.inf, 0.3], 11)
    want_counts = S.counts(score, cut, K)
    right = np.cumsum(want_counts, dtype=np.int64) - want_counts
    total = int(want_counts.sum())
    rng = np.random.default_rng(2)
    wrong = [right[::-1].copy(), right - 1000, right + total - 50, np.zeros_like(right), np.full_like(right, total - 1),
             rng.integers(-5000, total + 5000, right.size), np.full_like(right, -(1 << 62)), np.full_like(right, (1 << 62))]
    for i, offsets in enumerate(wrong):
        for tot in (total, total // 3, 1):
            values = np.arange(tot, dtype=np.float64) + 1.0
            bufs = dict(head, offsets=arr("i64", offsets), hit_index=out("i32", tot), hit_score=out("f64", tot))   # (no index poison: on purpose)
            a = GuardedArena(bufs, "AB"[i % 2], dev)
            _lib.call("dig_row_select_fill", a.ptr("score"), a.ptr("cut"), rows, n, a.ptr("offsets"), tot, a.ptr("hit_index"),
                      a.ptr("hit_score"), _lib.stream_ptr())
            a.assert_intact("dig_row_select_fill with wrong offsets (set %d, total %d)" % (i, tot))
            bufs = dict(head, offsets=arr("i64", offsets), values=arr("f64", values), out=out("f64", (rows, n)))
            a = GuardedArena(bufs, "AB"[i % 2], dev)
            _lib.call("dig_row_scatter", a.ptr("score"), a.ptr("cut"), rows, n, a.ptr("offsets"), tot, a.ptr("values"), -2.0, a.ptr("out"),
                      _lib.stream_ptr())
            a.assert_intact("dig_row_scatter with wrong offsets (set %d, total %d)" % (i, tot))
            got = a.read("out")
            assert np.isin(got, np.concatenate([values, [-2.0]])).all()
    # the right offsets with a total that cuts the list short: the head of the list, nothing behind it
    want_index, want_score, _ = S.fill(score, cut)
    short = total // 2
    bufs = dict(head, offsets=arr("i64", right), hit_index=out("i32", short), hit_score=out("f64", short))
    a = GuardedArena(bufs, "A", dev)
    _lib.call("dig_row_select_fill", a.ptr("score"), a.ptr("cut"), rows, n, a.ptr("offsets"), short, a.ptr("hit_index"), a.ptr("hit_score"),
              _lib.stream_ptr())
    a.assert_intact("dig_row_select_fill with a short total")
    assert a.read("hit_index").tobytes() == want_index[:short].tobytes() and a.read("hit_score").tobytes() == want_score[:short].tobytes()
