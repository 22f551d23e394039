"""dig_tile_sample_keys / dig_tile_sample_counts called through `_lib.call` with pointers carved from a guarded arena
(tests/guarded_arena.py): every argument at exactly the alignment of its element and no more, outputs of exactly their sizes (the
entry points take no scratch), 64 KiB of typed poison around every buffer, twice (poison A / B): no band touched, outputs
bit-identical between A and B and to the call on ordinary tensors, and equal to the plain-Python statement; with one output plane
NULL the other one is what it was with both."""
import numpy as np
import pytest

import guarded_arena as GA
from guarded_arena import guarded_runs, out
import tile_samples_cases as K
import tile_samples_statement as S

pytestmark = pytest.mark.gpu

BINSIZE, T = 50, 8
FIRST, NVALID = [100, 500, 1000, 1850, 200, 899], [8, 7, 8, 3, 8, 0]      # what base_tile_probs says (test_gpu_tile_samples.py checks it)
NOKEY = np.iinfo(np.int64).max


@pytest.fixture(scope="module")
def dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def stack():
    return K.stacked(K.cohort_rows())


def arr(dtype, data, **kw):
    return GA.inp(dtype, np.ascontiguousarray(data, GA._NP[dtype]), **kw)


def _pairs(st, n_rows):
    """The (row, region) pairs of the join of the first n_rows rows, row-major, made on the host."""
    pm, pr = [], []
    for i in range(n_rows):
        for r, (c, s, e) in enumerate(K.IDX):
            if st["chrom"][i] == str(c) and st["start"][i] < e and st["end"][i] > s:
                pm.append(i), pr.append(r)
    return np.array(pm, np.int32), np.array(pr, np.int32)


@pytest.mark.parametrize("n_rows", [1, 255, 1181, 2782])
def test_both_entry_points_at_their_documented_alignments(n_rows, stack, dev):
    from digdriver_amd import _lib
    st = stack
    R, S_all = len(K.IDX), int(st["sample_offsets"][-1])
    assert n_rows <= len(st["start"])
    keep = np.array(S.keep_from_max_muts([int(s) for s in st["sample"]], S_all, K.MAX_MUTS_PER_SAMPLE), np.uint8)
    pm, pr = _pairs(st, n_rows)
    n = len(pm)
    assert n > 0 or n_rows == 1
    regions, rows = K.statement_regions(FIRST, NVALID), K.statement_rows(st)
    sb = int(S_all).bit_length()                                        # bits that hold 0 .. S
    want_keys = np.full(n, NOKEY, np.int64)
    for i, (m, r) in enumerate(zip(pm, pr)):
        at = S.pair_tile(rows[m], regions[r], BINSIZE, T, K.C, list(keep))
        if at is not None:
            want_keys[i] = (((at[0] * R + r) * T + at[1]) << sb) | rows[m][4]
    want_cap, want_samples = (np.array(x, np.int32) for x in S.tile_sample_counts(regions, rows[:n_rows], K.C, BINSIZE, T, list(keep), K.CAP))
    if n:
        bufs = dict(pair_mut=arr("i32", pm, index=(0, n_rows - 1)) if n_rows > 1 else arr("i32", pm), pair_reg=arr("i32", pr, index=(0, R - 1)),
                    mut_start=arr("i64", st["start"][:n_rows]), mut_cohort=arr("i32", st["cohort"][:n_rows], index=(0, K.C - 1)),
                    mut_sample=arr("i32", st["sample"][:n_rows], index=(0, S_all - 1)), keep=arr("u8", keep),
                    first_pos=arr("i64", FIRST), n_valid=arr("i32", NVALID, index=(0, T)), keys=out("i64", n))
        got = guarded_runs(bufs, lambda g: _lib.call("dig_tile_sample_keys", g.ptr("pair_mut"), g.ptr("pair_reg"), n, g.ptr("mut_start"), n_rows,
                                                     g.ptr("mut_cohort"), g.ptr("mut_sample"), g.ptr("keep"), g.ptr("first_pos"), g.ptr("n_valid"),
                                                     BINSIZE, T, R, K.C, S_all, g.ptr("keys"), _lib.stream_ptr()),
                           device=dev, what="dig_tile_sample_keys", plain=True)
        assert np.array_equal(got["keys"], want_keys)
    keys = np.sort(want_keys)
    both = None
    for planes in (("k_cap", "k_samples"), ("k_cap",), ("k_samples",)):
        bufs = dict(keys=arr("i64", keys, index=(0, int(NOKEY))) if n else arr("i64", np.zeros(1, np.int64)),
                    **{p: out("i32", (K.C, R, T)) for p in planes})
        got = guarded_runs(bufs, lambda g: _lib.call("dig_tile_sample_counts", g.ptr("keys"), n, K.C, R, T, S_all, K.CAP, g.ptr("k_cap"),
                                                     g.ptr("k_samples"), _lib.stream_ptr()),
                           device=dev, what="dig_tile_sample_counts " + "+".join(planes), plain=True)
        if both is None:
            both = got
            assert np.array_equal(got["k_cap"], want_cap) and np.array_equal(got["k_samples"], want_samples)
        for p in planes:
            assert np.array_equal(got[p], both[p]), planes
    if n_rows >= 1181:
        assert want_cap[0, 0, 1] >= K.CAP and want_samples[0, 0, 4] >= 70 and (keys == NOKEY).sum() > 100
