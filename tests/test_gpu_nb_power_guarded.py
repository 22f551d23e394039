"""dig_nb_power and its `_host` twin called through `_lib.call` with pointers carved from a guarded arena (tests/guarded_arena.py; the
twin's arena lies in host memory), on a side stream as well: every argument at exactly the alignment the header states -- its
element's and no more: the planes, level, scale, folds and power at 8 (mod 16), k_crit at 4 (mod 8) --, outputs of exactly rows n and
n_folds rows n elements, 64 KiB of typed poison around every buffer, twice (poison A / B): no band touched, outputs bit-identical
between A and B, equal to the call on ordinary buffers; the counts and powers of the table's rows are the table's
(tests/test_nb_power_fixture.py).  And engine.nb_power inside a side stream while the default stream is busy."""
import numpy as np
import pytest

import guarded_arena as GA
import nb_power_statement as S
from guarded_arena import guarded_runs, out
from test_nb_power_fixture import blocks_of, check_counts, load_fixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


def arr(data):
    return GA.inp("f64", np.ascontiguousarray(data, np.float64))


# (rows, n, folds, with a scale): one element; a row that ends inside a workgroup's chunk; several chunks and rows; no fold at all
CASES = [(1, 1, 1, True), (3, 65, 6, True), (2, 200, 8, False), (3, 257, 0, True)]


@pytest.mark.parametrize("R,n,F,scaled", CASES, ids=lambda v: str(v))
def test_entry_point_and_twin_at_their_documented_alignments(R, n, F, scaled, dev, fx):
    from digdriver_amd import _lib
    b = blocks_of(fx)[:15]
    pick = [b[(4 * c % 5) * 3 + c] for c in range(R)]                    # rows of the plane: blocks of three levels and three scales
    rows = [np.resize(r, n) for r, _, _, _ in pick]                     # (a block's 200 rows, taken round again beyond them)
    planes = {c: np.stack([fx[c][r] for r in rows]) for c in ("alpha", "theta", "pi")}
    level, cj, k_max = np.array([l for _, l, _, _ in pick]), np.array([c for _, _, c, _ in pick]), pick[0][3]
    folds = (fx["folds"] + (3.0, 1.5))[:F]
    if not scaled:                                                       # (the scale folded into theta: the same product, formed here)
        planes["theta"] = planes["theta"] * cj[:, None]
    results = []
    for suffix, where in (("", dev), ("_host", "cpu")):
        last = (lambda: _lib.stream_ptr()) if where is dev else (lambda: 0)
        bufs = dict(alpha=arr(planes["alpha"]), theta=arr(planes["theta"]), pi=arr(planes["pi"]), level=arr(level),
                    k_crit=out("i32", (R, n)))
        if scaled:
            bufs["scale"] = arr(cj)
        if F:
            bufs.update(folds=arr(folds), power=out("f64", (F, R, n)))
        got = guarded_runs(bufs, lambda a: _lib.call("dig_nb_power" + suffix, a.ptr("alpha"), a.ptr("theta"), a.ptr("pi"), a.ptr("scale"),
                                                     a.ptr("level"), R, n, a.ptr("folds"), F, k_max, a.ptr("k_crit"), a.ptr("power"), last()),
                           device=where, what="dig_nb_power" + suffix, plain=True)
        for i, r in enumerate(rows):
            check_counts(got["k_crit"][i], fx, "dig_nb_power%s, guarded, row %d" % (suffix, i), rows=r)
            if F:
                S.check_power(got["power"][:min(F, 6), i], fx["power"][:min(F, 6), r], fx["k_crit"][r], "dig_nb_power%s, guarded" % suffix)
        results.append(got)
    assert all(results[0][k].tobytes() == results[1][k].tobytes() for k in results[0])


def test_the_engine_route_works_on_the_current_stream(dev, fx):
    """engine.nb_power -- the upload of the folds, the kernel -- inside a side stream while the default stream is busy
    (guarded_arena.side_stream_call): everything is issued on torch's current stream."""
    import torch
    from digdriver_amd import engine
    rows, level, cj, k_max = blocks_of(fx)[7]
    on = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    a, t, p = (on(fx[c][rows][None]) for c in ("alpha", "theta", "pi"))
    got = GA.side_stream_call(lambda stream: engine.nb_power(a, t, p, on(np.array([level])), scale=on(np.array([cj])), folds=fx["folds"],
                                                             k_max=k_max), dev, "engine.nb_power")
    check_counts(got["k_crit"][0], fx, "engine.nb_power on a side stream", rows=rows)
    S.check_power(got["power"][:, 0], fx["power"][:, rows], fx["k_crit"][rows], "engine.nb_power on a side stream")
