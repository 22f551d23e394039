"""dig_map_windows / dig_map_scores and their `_host` twins called through `_lib.call` with pointers carved from a guarded arena
(tests/guarded_arena.py): every argument at exactly the alignment of its element and no more, outputs of exactly their sizes, the
workspace of exactly dig_map_scores_workspace bytes, 64 KiB of typed poison around every buffer, twice (poison A / B): no band touched,
outputs bit-identical between A and B and to the call on ordinary tensors, equal to the numpy statement; one case with flag_cm = NULL;
engine.map_windows inside a side stream."""
import numpy as np
import pytest

import guarded_arena as GA
import map_report_cases as MC
from guarded_arena import guarded_runs, out
from map_report_cases import same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    return torch.device("cuda:0")


def arr(dtype, data, **kw):
    return GA.inp(dtype, np.ascontiguousarray(data, GA._NP[dtype]), **kw)


@pytest.mark.parametrize("twin", [False, True], ids=["device", "twin"])
@pytest.mark.parametrize("name,drop", [("37x301_s3", True), ("3x1003_s100", False), ("2x20011_chrom", True)])
def test_both_entry_points_at_their_documented_alignments(name, drop, twin, dev):
    from digdriver_amd import _lib
    case, s = MC.shape_case(name)
    want = MC.expected(case, s, drop, "upper")
    C, N = case["mu"].shape
    ptr = want["run_ptr"]
    M = len(ptr) - 1
    where = "cpu" if twin else dev
    last = (lambda: 0) if twin else _lib.stream_ptr
    sym = lambda n: n + "_host" if twin else n
    bufs = dict(mu=arr("f64", case["mu"]), sd=arr("f64", case["std"]), y=arr("i32", case["y"]), run_ptr=arr("i64", ptr, index=(0, N)),
                n_bins=out("i32", (C, M)), y_true=out("i64", (C, M)), y_pred=out("f64", (C, M)), std=out("f64", (C, M)), pval=out("f64", (C, M)))
    if drop:                                                            # (without drop_flagged flag_cm is NULL: it is not read)
        bufs["flag"] = arr("u8", case["flag"])
    got = guarded_runs(bufs, lambda g: _lib.call(sym("dig_map_windows"), g.ptr("mu"), g.ptr("sd"), g.ptr("y"), g.ptr("flag") if drop else None, C, N,
                                                 g.ptr("run_ptr"), M, int(drop), 0, g.ptr("n_bins"), g.ptr("y_true"), g.ptr("y_pred"),
                                                 g.ptr("std"), g.ptr("pval"), last()),
                       device=where, what=sym("dig_map_windows"), plain=True)
    P = want["planes"]
    assert np.array_equal(got["n_bins"], P["n_bins"]) and np.array_equal(got["y_true"], P["y_true"])
    assert same_bits(got["y_pred"], P["y_pred"]) and same_bits(got["std"], P["std"])
    nbytes = int(_lib.load().dig_map_scores_workspace(C, M))
    assert nbytes == C * (-(-M // 1024) * 88 + 16)
    bufs = dict(n_bins=arr("i32", got["n_bins"]), y_true=arr("i64", got["y_true"]), y_pred=arr("f64", got["y_pred"]), pval=arr("f64", got["pval"]),
                counts=out("i64", (C, 7)), sums=out("f64", (C, 4)))
    if not twin:
        bufs["ws"] = GA.ws(nbytes, align=8)
    tail = (lambda g: (0,)) if twin else (lambda g: (g.ptr("ws"), nbytes, _lib.stream_ptr()))
    sc = guarded_runs(bufs, lambda g: _lib.call(sym("dig_map_scores"), g.ptr("n_bins"), g.ptr("y_true"), g.ptr("y_pred"), g.ptr("pval"), C, M,
                                                g.ptr("counts"), g.ptr("sums"), *tail(g)),
                      device=where, what=sym("dig_map_scores"), plain=True)
    assert np.array_equal(sc["counts"], want["counts"]) and same_bits(sc["sums"], want["sums"])


def test_engine_map_windows_inside_a_side_stream(dev):
    import torch
    from digdriver_amd import engine
    case, s = MC.shape_case("2x20011_chrom")
    want = MC.expected(case, s, False, "side")
    on = lambda x: torch.as_tensor(x, device=dev)
    args = [on(case["mu"]), on(case["std"]), on(case["y"]), None, on(want["run_ptr"])]
    plain = GA.side_stream_call(lambda stream: engine.map_windows(*args, tail="side"), dev, "engine.map_windows")
    assert np.array_equal(plain["y_true"], want["planes"]["y_true"]) and same_bits(plain["y_pred"], want["planes"]["y_pred"])
    assert same_bits(plain["std"], want["planes"]["std"])
