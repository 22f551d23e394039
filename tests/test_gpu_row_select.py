"""The calls of the element route on the GPU: dig_row_select_count / dig_row_select_fill / dig_row_scatter (engine.row_select_counts,
row_select, row_scatter; device form and `_host` twins) against the numpy statements of tests/row_select_statement.py, bit for bit,
with the chunk K taken from dig_row_select_chunk; and cohort_batch.plane_qvalues against get_q_vals of every row's NaN-dropped list.
Shapes: n around the wave (63, 64, 65), around the chunk (K - 1, K, K + 1), two chunks and a rest with a lead and a tail element
(2 K + 7), one element and none; one row and three (with an odd n the rows start at 0 and at 8 (mod 16) in turn).  Values as
test_tile_hits_host._random_list draws them -- ties, exact zeros, ones, NaNs --, of three rows one all NaN and one without a NaN.
Cuts: +inf, NaN, a cut equal to a score (inclusive) and a cut below every score, every row in turn.
The launches do not cap their grid (a wave per chunk, rows * chunks < 2^31), so there is no second trip to test."""
import numpy as np
import pytest

import row_select_statement as S
from test_tile_hits_host import _random_list

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    from digdriver_amd import _lib
    _lib.require_device()
    return int(_lib.load().dig_row_select_chunk())


def _plane(rows, n, seed):
    rng = np.random.default_rng(seed)
    score = np.stack([_random_list(rng, n) for _ in range(rows)]).reshape(rows, n)
    if rows == 3:
        score[1] = np.nan
        score[2] = np.where(np.isnan(score[2]), 0.25, score[2])
        assert n == 0 or (not np.isnan(score[2]).any() and np.isnan(score[1]).all())
    return score


def _cuts(score, kind, rng):
    """cut [rows]: row r takes kind (kind + r) % 4 of (+inf, NaN, equal to one of its scores, below every score)."""
    rows, n = score.shape
    cut = np.empty(rows)
    for r in range(rows):
        k = (kind + r) % 4
        numbers = score[r][~np.isnan(score[r])]
        cut[r] = (np.inf, np.nan, float(rng.choice(numbers)) if numbers.size else 0.5, -1.0)[k]
    return cut


def _at(score, parity):
    """The plane as a device tensor whose first element lies at 8 * parity (mod 16)."""
    import torch
    raw = torch.empty(score.size + 2, dtype=torch.float64, device="cuda:0")
    off = (parity - (raw.data_ptr() >> 3)) & 1
    view = raw[off:off + score.size].view(score.shape)
    view.copy_(torch.from_numpy(score))
    assert score.size == 0 or view.data_ptr() % 16 == 8 * parity           # (an empty tensor has no address)
    return view


def _n_of(name, K):
    return {"K-1": K - 1, "K": K, "K+1": K + 1, "2K+7": 2 * K + 7}.get(name, name)


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n_name", [0, 1, 63, 64, 65, "K-1", "K", "K+1", "2K+7"])
def test_device_entry_points_and_host_twins_against_the_statement(n_name, rows, K):
    import torch
    from digdriver_amd import engine
    n = _n_of(n_name, K)
    score = _plane(rows, n, 100 * rows + (n % 97))
    rng = np.random.default_rng(n + rows)
    seen = 0
    for kind in range(4):
        cut = _cuts(score, kind, rng)
        want_counts = S.counts(score, cut, K)
        want_index, want_score, want_ptr = S.fill(score, cut)
        seen += len(want_index)
        for parity in ((0, 1) if kind == 0 else (kind & 1,)):                  # both bases at cut = +inf first, then in turn
            for be_score in (_at(score, parity), score):
                host = lambda x: x.cpu().numpy() if isinstance(x, torch.Tensor) else x
                counts = engine.row_select_counts(be_score, cut)
                assert counts.shape == (rows, -(-n // K)) and np.array_equal(host(counts).reshape(-1), want_counts)
                got = engine.row_select(be_score, cut)
                assert np.array_equal(got["row_ptr"], want_ptr) and got["row_ptr"].dtype == np.int64
                assert np.array_equal(host(got["index"]), want_index) and host(got["index"]).dtype == np.int32
                assert host(got["score"]).tobytes() == want_score.tobytes()
                lists = engine.row_select(be_score, cut, index=False)
                assert set(lists) == {"score", "row_ptr"} and host(lists["score"]).tobytes() == want_score.tobytes()
                # the round trip: the scores put back at the selected places, the fill elsewhere
                back = host(engine.row_scatter(be_score, cut, got["score"], fill=-3.0))
                assert back.tobytes() == S.scatter(score, cut, want_score, -3.0).tobytes()
                sel = S.selected(score, cut)
                assert back.shape == (rows, n) and back[sel].tobytes() == score[sel].tobytes() and (back[~sel] == -3.0).all()
                # other values, and the default fill
                other = np.arange(len(want_index), dtype=np.float64) * 0.5 + 1.0
                back = host(engine.row_scatter(be_score, cut, torch.as_tensor(other, device="cuda:0") if be_score is not score else other))
                assert back.tobytes() == S.scatter(score, cut, other, np.nan).tobytes()
    assert n == 0 or seen > 0
    with pytest.raises(ValueError, match="values for"):
        engine.row_scatter(score, np.inf, np.zeros(score.size + 1))


def test_a_single_cut_stands_for_every_row_and_inclusive_edge(K):
    """cut given as one number; a cut equal to the plane's smallest and largest number takes exactly the ties of the first and every
    number; one just below the smallest takes nothing."""
    from digdriver_amd import engine
    score = _plane(3, K + 1, 7)
    numbers = score[~np.isnan(score)]
    lo, hi = numbers.min(), numbers.max()
    for cut, want in ((lo, (numbers == lo).sum()), (hi, numbers.size), (np.nextafter(lo, -1.0), 0)):
        for be_score in (_at(score, 1), score):
            got = engine.row_select(be_score, float(cut))
            assert int(got["row_ptr"][-1]) == want == len(got["index"])


def test_plane_qvalues_equals_the_statement(K):
    """[2, 3, 2 K + 7]: six rows over two chunks and a rest; one row all NaN (every q NaN), one without a NaN."""
    import torch
    from digdriver_amd.driver_model import cohort_batch
    rng = np.random.default_rng(17)
    n = 2 * K + 7
    p = np.stack([_random_list(rng, n) for _ in range(6)]).reshape(2, 3, n)
    p[0, 1] = np.nan
    p[1, 2] = np.where(np.isnan(p[1, 2]), 1.0, p[1, 2])
    assert np.isnan(p[0, 0]).any() and (p == 0.0).any() and (p == 1.0).any()
    got = cohort_batch.plane_qvalues(torch.as_tensor(p, device="cuda:0"))
    assert got.shape == (2, 3, n) and got.dtype == torch.float64
    assert got.cpu().numpy().tobytes() == S.plane_qvalues(p).tobytes()
    empty = cohort_batch.plane_qvalues(torch.full((2, 5), float("nan"), dtype=torch.float64, device="cuda:0"))
    assert bool(torch.isnan(empty).all()) and empty.shape == (2, 5)


def test_empty_inputs_launch_nothing_and_null_outputs_are_skipped(K):
    import torch
    from digdriver_amd import _lib
    p, s = _lib.dev_ptr, _lib.stream_ptr()
    one, o1 = (torch.zeros(1, dtype=dt, device="cuda:0") for dt in (torch.float64, torch.int64))
    i1 = torch.full((1,), 5, dtype=torch.int32, device="cuda:0")
    _lib.call("dig_row_select_count", None, None, 0, 5, None, s)
    _lib.call("dig_row_select_count", None, None, 5, 0, None, s)
    _lib.call("dig_row_select_fill", None, None, 3, 3, None, 0, None, None, s)
    _lib.call("dig_row_scatter", None, None, 0, 3, None, 0, None, 0.0, None, s)
    _lib.call("dig_row_select_fill", p(one), p(one), 1, 1, p(o1), 1, None, None, s)              # both outputs NULL
    _lib.call("dig_row_select_fill", p(one), p(one), 1, 1, p(o1), 1, p(i1), None, s)
    torch.cuda.synchronize()
    assert int(i1) == 0
    for name, args in (("dig_row_select_count", (p(one), p(one), 1, 1 << 31, p(i1), s)),
                       ("dig_row_select_fill", (p(one), p(one), 1, 1, p(o1), -1, p(i1), p(one), s))):
        with pytest.raises(_lib.DigHipError, match="requirement failed"):
            _lib.call(name, *args)
