"""dig_panel_row_keys / dig_panel_counts called through `_lib.call` with pointers carved from a guarded arena
(tests/guarded_arena.py): every argument at exactly the alignment of its element and no more, outputs of exactly their sizes (the
entry points take no scratch), 64 KiB of typed poison around every buffer, twice (poison A / B): no band touched, outputs
bit-identical between A and B and to the call on ordinary tensors, and equal to the plain-Python statement."""
import numpy as np
import pytest

import guarded_arena as GA
from guarded_arena import guarded_runs, out
import target_cohort_cases as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lanes():
    return T.kernel_cases()["lanes600"][0]


def arr(dtype, data, **kw):
    return GA.inp(dtype, np.ascontiguousarray(data, GA._NP[dtype]), **kw)


@pytest.mark.parametrize("n", [1, 255, 257, 600])
def test_both_entry_points_at_their_documented_alignments(n, lanes, dev):
    from digdriver_amd import _lib
    a = T.first_rows(lanes, n)
    want = T.statement_of(a)
    off, mask, P = a["sample_offsets"], a["label_mask"], a["P"]
    C, S, L = len(off) - 1, int(off[-1]), len(mask)
    assert C == 3 and int(np.diff(off).min()) == 5 and a["skip"] is not None
    tables = dict(sample_off=arr("i64", off, index=(0, S)), label_mask=arr("u32", mask))
    bufs = dict(label=arr("i32", a["label"], index=(0, L)), sample=arr("i32", a["sample"], index=(0, 4)), annot=arr("u8", a["annot"]),
                cohort=arr("i32", a["cohort"], index=(0, C - 1)), skip=arr("u8", a["skip"]), keys=out("i64", n), n_cds=out("i64", C), **tables)
    got = guarded_runs(bufs, lambda g: _lib.call("dig_panel_row_keys", g.ptr("label"), g.ptr("sample"), g.ptr("annot"), g.ptr("cohort"),
                                                 g.ptr("sample_off"), g.ptr("skip"), g.ptr("label_mask"), n, L, P, C, S, g.ptr("keys"),
                                                 g.ptr("n_cds"), _lib.stream_ptr()),
                       device=dev, what="dig_panel_row_keys", plain=True)
    assert np.array_equal(got["n_cds"], want["n_cds"])
    lb = max(1, int(L - 1).bit_length())
    keys = got["keys"]
    assert keys.min() >= -1 and keys.max() < (S << lb)
    made = keys[keys >= 0]
    assert ((made & ((1 << lb) - 1)) < L).all() and len(made) == int(want["n_mut"].sum() - _double_counted(a, want))
    keys = np.sort(keys)
    bufs = dict(keys=arr("i64", keys, index=(-1, ((S - 1) << lb) | (L - 1))), n_mut=out("i64", (C, P)), n_pairs=out("i64", (C, P)),
                n_sample=out("i64", (C, P)), **tables)
    got = guarded_runs(bufs, lambda g: _lib.call("dig_panel_counts", g.ptr("keys"), n, g.ptr("label_mask"), g.ptr("sample_off"), L, P, C, S,
                                                 g.ptr("n_mut"), g.ptr("n_pairs"), g.ptr("n_sample"), _lib.stream_ptr()),
                       device=dev, what="dig_panel_counts", plain=True)
    for k in ("n_mut", "n_pairs", "n_sample"):
        assert np.array_equal(got[k], want[k]), k


def _double_counted(a, want):
    """Rows that count in both panels appear twice in the sum of n_mut and once among the keys."""
    both = np.flatnonzero(a["label_mask"] == 3)
    counted = np.isin(a["annot"], (1, 2, 4, 5)) & np.isin(a["label"], both)
    if a["skip"] is not None:
        counted &= a["skip"][a["sample_offsets"][a["cohort"]] + a["sample"]] == 0
    return int(counted.sum())
