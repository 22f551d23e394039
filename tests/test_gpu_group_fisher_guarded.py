"""dig_group_fisher / dig_group_sums and their `_host` twins called through `_lib.call` with pointers carved from a guarded arena
(tests/guarded_arena.py; the twins' arena lies in host memory), on a side stream as well: every argument at exactly the alignment the
header states -- its element's and no more: the planes and the outputs at 8 (mod 16), where no 16-byte access may start at the first
element, out_n at 4 (mod 8), member at an odd address --, outputs of exactly R M E elements, 64 KiB of typed poison around every
buffer, twice (poison A / B): no band touched, outputs bit-identical between A and B, equal to the call on ordinary buffers and to the
numpy statement (tests/group_fisher_statement.py)."""
import numpy as np
import pytest

import group_fisher_statement as S
import guarded_arena as GA
from guarded_arena import guarded_runs, out
from test_gpu_group_fisher import group_set, hostile_plane

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    return torch.device("cuda:0")


def arr(dtype, data, **kw):
    return GA.inp(dtype, np.ascontiguousarray(data, GA._NP[dtype]), **kw)


# (R, C, E, M): an odd E with several rows (both load forms), an even one, one chunk and several, both compiled forms of M
CASES = [(2, 3, 129, 8), (1, 37, 64, 9), (4, 2, 517, 32), (1, 64, 1, 1)]


@pytest.mark.parametrize("R,C,E,M", CASES, ids=lambda v: str(v))
def test_both_entry_points_and_their_twins_at_their_documented_alignments(R, C, E, M, dev):
    from digdriver_amd import _lib
    from digdriver_amd.sequence_model import nb_model
    rng = np.random.default_rng(R + C + E + M)
    p, member = hostile_plane(rng, R, C, E), group_set(rng, C, M, 0)
    x = rng.integers(0, 50, size=p.shape) + rng.uniform(size=p.shape)
    want_n = S.n_used(p, member)
    small, known = S.small_groups(p, member, nb_model.fisher_combine)
    want_sums, want_gated = S.group_sums(x, member), S.group_sums(x, member, p)
    pvals = []
    for suffix, where in (("", dev), ("_host", "cpu")):
        last = (lambda: _lib.stream_ptr()) if where is dev else (lambda: 0)
        bufs = dict(p=arr("f64", p), member=arr("u8", member), out_p=out("f64", (R, M, E)), out_n=out("i32", (R, M, E)))
        got = guarded_runs(bufs, lambda a: _lib.call("dig_group_fisher" + suffix, a.ptr("p"), a.ptr("member"), R, C, E, M, a.ptr("out_p"),
                                                     a.ptr("out_n"), last()),
                           device=where, what="dig_group_fisher" + suffix, plain=True)
        assert got["out_n"].tobytes() == want_n.tobytes() and got["out_p"][known].tobytes() == small[known].tobytes()
        pvals.append(got["out_p"])
        # without out_n: the same p-values
        bufs = dict(p=arr("f64", p), member=arr("u8", member), out_p=out("f64", (R, M, E)))
        got = guarded_runs(bufs, lambda a: _lib.call("dig_group_fisher" + suffix, a.ptr("p"), a.ptr("member"), R, C, E, M, a.ptr("out_p"),
                                                     None, last()),
                           device=where, what="dig_group_fisher%s without out_n" % suffix, plain=True, side_stream=False)
        assert got["out_p"].tobytes() == pvals[-1].tobytes()
        for gate, want in ((None, want_sums), (p, want_gated)):
            bufs = dict(x=arr("f64", x), member=arr("u8", member), out=out("f64", (R, M, E)))
            if gate is not None:
                bufs = dict(bufs, gate=arr("f64", gate))
            got = guarded_runs(bufs, lambda a: _lib.call("dig_group_sums" + suffix, a.ptr("x"), a.ptr("gate"), a.ptr("member"), R, C, E, M,
                                                         a.ptr("out"), last()),
                               device=where, what="dig_group_sums%s%s" % (suffix, "" if gate is None else " (gated)"), plain=True)
            assert got["out"].tobytes() == want.tobytes()
    assert pvals[0].tobytes() == pvals[1].tobytes()


def test_the_engine_routes_work_on_the_current_stream(dev):
    """engine.group_fisher and engine.group_sums with 33 groups -- two launches each, the second one's slice copied into the result --
    inside a side stream while the default stream is busy (guarded_arena.side_stream_call): every kernel and copy of the route is
    issued on torch's current stream."""
    import torch
    from digdriver_amd import engine
    rng = np.random.default_rng(12)
    p, member = hostile_plane(rng, 2, 37, 517), group_set(rng, 37, 33, 0)
    tp, tm = torch.as_tensor(p, device=dev), torch.as_tensor(member, device=dev)
    got = GA.side_stream_call(lambda stream: engine.group_fisher(tp, tm), dev, "engine.group_fisher")
    assert got["n_used"].tobytes() == S.n_used(p, member).tobytes()
    got = GA.side_stream_call(lambda stream: engine.group_sums(tp, tm, gate=tp), dev, "engine.group_sums")
    assert got["result"].tobytes() == S.group_sums(p, member, p).tobytes()
