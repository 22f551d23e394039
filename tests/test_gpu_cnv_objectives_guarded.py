"""dig_cnv_segment_deltas, dig_cnv_window_means and their `_host` twins called through `_lib.call` with pointers carved from a guarded
arena (tests/guarded_arena.py; the twins' arena lies in host memory), on a side stream as well: every argument at exactly the alignment
of its element and no more, the difference array and the carries of exactly the bytes their size queries return, 64 KiB of typed
poison around every buffer, twice (poison A / B): no band touched, outputs bit-identical between A and B and to the call on ordinary
buffers.  The difference array sums to zero along every row and its prefix sums / W are the per-base statement
(cnv_windows_statement.py); the labels are the statement's, [C, N, 3].
Shapes: 7 windows that overlap each other on two chromosomes (every window partial for some segment, the last window's -v in element
N); 2 049 tiling windows = one chunk of the scan and one window, the chromosomes' border in the first chunk."""
import numpy as np
import pytest

import guarded_arena as GA
from guarded_arena import guarded_runs, out
import cnv_windows_statement as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    return torch.device("cuda:0")


def arr(dtype, data, **kw):
    return GA.inp(dtype, np.ascontiguousarray(data, GA._NP[dtype]), **kw)


def _case(name):
    rng = np.random.default_rng(len(name))
    if name == "overlapping":
        W, C, n = 100, 3, 60
        win = np.array([(2, 0), (2, 40), (2, 80), (2, 300), (9, 10), (9, 50), (9, 130)], np.int64)
        span = 500
    else:
        W, C, n = 10, 2, 400
        win = np.array([(2, W * i) for i in range(1_500)] + [(9, W * i) for i in range(549)], np.int64)
        span = 15_000
    start = rng.integers(0, span, n)
    length = np.exp(rng.uniform(0, np.log(span), n)).astype(np.int64) + 1
    chrom = rng.choice([2, 9, 4], n, p=[0.5, 0.4, 0.1])
    cp = rng.choice([0, 1, 2, 3, 8], n)
    cohort = rng.integers(0, C, n)
    h = 3 * C                                                                             # everything, once per class and cohort
    start[:h], length[:h], chrom[:h] = 0, span, np.resize([2, 9], h)
    cp[:h], cohort[:h] = np.repeat([3, 2, 1], C), np.resize(np.arange(C), h)
    return W, C, win, (chrom.astype(np.int64), start, start + length, cp, cohort)


@pytest.mark.parametrize("name", ["overlapping", "one chunk and a window"])
def test_both_entry_points_and_their_twins_at_their_documented_alignments(name, dev):
    from digdriver_amd import _lib
    lib = _lib.load()
    W, C, win, segs = _case(name)
    N, n = len(win), len(segs[0])
    want = S.window_means(win[:, 0], win[:, 1], W, *segs, C)                              # [N, 3, C]; win is sorted and distinct
    klass, weight = S.class_and_weight(segs[3])
    chrom_id, first = np.unique(win[:, 0], return_index=True)
    chrom_off = np.concatenate([first, [N]])
    delta_bytes, carry_bytes = int(lib.dig_cnv_segment_deltas_size(C, N)), int(lib.dig_cnv_window_means_size(C, N))
    assert delta_bytes == C * 3 * (N + 1) * 8 and carry_bytes == C * 3 * -(-N // _lib.DIG_CNV_SCAN_CHUNK) * 8
    ins = dict(win_start=arr("i64", win[:, 1]), chrom_id=arr("i64", chrom_id), chrom_off=arr("i64", chrom_off, index=(0, N)),
               seg_chrom=arr("i64", segs[0]), seg_start=arr("i64", segs[1]), seg_end=arr("i64", segs[2]),
               seg_class=arr("u8", klass, index=(0, 2)), seg_weight=arr("i32", weight), seg_cohort=arr("i32", segs[4], index=(0, C - 1)))
    for suffix, where in (("", dev), ("_host", "cpu")):
        last = (lambda: _lib.stream_ptr()) if where is dev else (lambda: 0)
        bufs = dict(ins, deltas=out("i64", (delta_bytes // 8,)))
        got = guarded_runs(bufs, lambda g: _lib.call("dig_cnv_segment_deltas" + suffix, g.ptr("win_start"), g.ptr("chrom_id"), g.ptr("chrom_off"),
                                                     len(chrom_id), N, W, g.ptr("seg_chrom"), g.ptr("seg_start"), g.ptr("seg_end"),
                                                     g.ptr("seg_class"), g.ptr("seg_weight"), g.ptr("seg_cohort"), n, C, g.ptr("deltas"), last()),
                           device=where, what="dig_cnv_segment_deltas" + suffix, plain=True)
        deltas = got["deltas"].reshape(C, 3, N + 1)
        assert not deltas.sum(axis=2).any() and deltas[:, :, N].any()
        assert np.array_equal((np.cumsum(deltas[:, :, :N], axis=2) / float(W)).transpose(2, 1, 0), want)
        bufs = dict(deltas=arr("i64", got["deltas"]), labels=out("f64", (C, N, 3)))
        if where is dev:
            bufs["carries"] = GA.ws(carry_bytes, dtype="i64")
        got = guarded_runs(bufs, lambda g: _lib.call("dig_cnv_window_means" + suffix, g.ptr("deltas"), N, C, W, g.ptr("labels"),
                                                     *([g.ptr("carries")] if where is dev else []), last()),
                           device=where, what="dig_cnv_window_means" + suffix, plain=True)
        assert GA.same_bits(got["labels"], np.ascontiguousarray(want.transpose(2, 0, 1)))
    assert (want > 0).any(axis=0).all()


def test_engine_route_on_a_side_stream(dev):
    """engine.window_cnv_means on device tensors inside a side stream while the default stream is busy: the memset, the four kernels,
    the uploads of the window tables and the gather back to the windows' order all work on the current stream."""
    import torch
    from digdriver_amd import engine
    W, C, win, segs = _case("one chunk and a window")
    klass, weight = S.class_and_weight(segs[3])
    args = [torch.as_tensor(a, device=dev) for a in (segs[0], segs[1], segs[2], klass.astype(np.uint8), weight.astype(np.int32),
                                                     segs[4].astype(np.int32))]
    win = win[np.random.default_rng(1).permutation(len(win))]
    plain = GA.side_stream_call(lambda stream: engine.window_cnv_means(win[:, 0], win[:, 1], W, *args, C), dev, "window_cnv_means")
    assert np.array_equal(plain["result"], S.window_means(win[:, 0], win[:, 1], W, *segs, C))
