"""The two helpers the per-base kernels share, at their edges, through every entry point that uses them, device form and `_host` twin.
  tile_slot (dig_tiles.hpp)     which tile a (mutation, region) pair counts in: dig_tile_mut_counts, dig_sparse_tile_keys,
                                dig_tile_sample_keys against a numpy statement written here, and against each other
  run_length (dig_keyruns.hpp)  the length of a run of equal sorted keys: dig_tile_sample_counts and dig_sparse_tile_test on one key
                                array whose runs start on the lanes 0, 1 and 63 of a wave, end at a wave's last lane, and cross waves
                                and 256-thread workgroups
Everything is an integer and compared exactly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NO_KEY = np.iinfo(np.int64).max
C, R, T, BINSIZE = 2, 3, 4, 7


def _backends():
    from digdriver_amd import _marshal
    return [_marshal.device_backend("cuda:0"), _marshal.HostBackend(0)]


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


# ---- the tile rule -------------------------------------------------------------------------------------------------------------
FIRST_POS = np.array([100, 200, 300], np.int64)
N_VALID = np.array([6, 0, -1], np.int32)          # region 0: more than n_tiles; region 1: no positions; region 2: the "too long" mark
# (START, cohort, region): one mutation row and one pair each
PAIRS = [
    (99, 0, 0), (100, 0, 0), (100, 0, 0), (100, 1, 0), (106, 0, 0), (107, 1, 0), (113, 0, 0), (114, 0, 0), (120, 1, 0),      # tiles 0 .. 2
    (121, 0, 0), (127, 0, 0), (127, 1, 0), (127, 1, 0),                                  # tile 3, the last counted one, to its last position
    (128, 0, 0), (128, 0, 0), (134, 0, 0), (135, 0, 0), (141, 0, 0), (128, 1, 0), (135, 1, 0),      # tiles 4 and 5: below n_valid, past n_tiles
    (142, 0, 0), (148, 1, 0), (100000, 0, 0),                                            # tile n_valid and beyond
    (100, -1, 0), (100, C, 0), (127, -1, 0), (121, C, 0), (128, -1, 0),                  # cohorts outside [0, C)
    (199, 0, 1), (200, 0, 1), (200, 1, 1), (207, 0, 1), (227, 1, 1), (228, 0, 1), (200, -1, 1),      # n_valid = 0: no tile counts
    (299, 0, 2), (300, 0, 2), (300, 1, 2), (313, 0, 2), (327, 1, 2), (328, 0, 2), (300, C, 2),       # n_valid = -1
]
N_SAMPLES = 5


def _rule_statement():
    """Per pair the slot (cohort R + region) T + tile, or -1; the tests in the library's order."""
    slot = np.full(len(PAIRS), -1, np.int64)
    for i, (start, c, r) in enumerate(PAIRS):
        off = start - FIRST_POS[r]
        if off < 0:
            continue
        t = off // BINSIZE
        if t >= N_VALID[r] or t >= T:
            continue
        if not 0 <= c < C:
            continue
        slot[i] = (c * R + r) * T + t
    return slot


def test_tile_rule_at_its_edges_through_its_three_consumers():
    slot = _rule_statement()
    counts = np.bincount(slot[slot >= 0], minlength=C * R * T).astype(np.int32).reshape(C, R, T)
    # what the pairs were written to hold: only region 0 counts, all four of its tiles, and nothing of the tiles 4 and 5
    assert counts[:, 1:].sum() == 0 and (counts[:, 0] > 0).all() and counts[0, 0, 0] == 3 and counts[1, 0, 3] == 2
    assert counts.sum() == 12 and (slot >= 0).sum() == 12
    sb = 3                                                   # bits for the N_SAMPLES + 1 values of the sample field
    assert (1 << sb) >= N_SAMPLES + 1 > (1 << (sb - 1))
    n = len(PAIRS)
    sample = (np.arange(n) % N_SAMPLES).astype(np.int32)
    for be in _backends():
        p = be.ptr
        pm, pr = be.arr(np.arange(n), "i32"), be.arr([q[2] for q in PAIRS], "i32")
        ms, co, sa = be.arr([q[0] for q in PAIRS], "i64"), be.arr([q[1] for q in PAIRS], "i32"), be.arr(sample, "i32")
        first, nval = be.arr(FIRST_POS, "i64"), be.arr(N_VALID, "i32")
        k, keys, skeys = be.empty((C, R, T), "i32"), be.empty(n, "i64"), be.empty(n, "i64")
        be.call("dig_tile_mut_counts", p(pm), p(pr), n, p(ms), *([] if be.is_device else [n]), p(co), p(first), p(nval), BINSIZE, T, R, C, p(k))
        be.call("dig_sparse_tile_keys", p(pm), p(pr), n, p(ms), n, p(co), p(first), p(nval), BINSIZE, T, R, C, p(keys))
        be.call("dig_tile_sample_keys", p(pm), p(pr), n, p(ms), n, p(co), p(sa), None, p(first), p(nval), BINSIZE, T, R, C, N_SAMPLES, p(skeys))
        k, keys, skeys = _host(k), _host(keys), _host(skeys)
        assert np.array_equal(k, counts), (be.is_device, np.argwhere(k != counts))
        real, sreal = keys != NO_KEY, skeys != NO_KEY
        k_sparse = np.bincount(keys[real], minlength=C * R * T).astype(np.int32).reshape(C, R, T)
        k_sample = np.bincount(skeys[sreal] >> sb, minlength=C * R * T).astype(np.int32).reshape(C, R, T)
        assert np.array_equal(k_sparse, counts) and np.array_equal(k_sample, counts)
        assert np.array_equal(k, k_sparse) and np.array_equal(k_sparse, k_sample)
        # every skipped pair has the no-key value, every other its own slot (and its sample)
        assert np.array_equal(keys, np.where(slot >= 0, slot, NO_KEY))
        assert np.array_equal(skeys, np.where(slot >= 0, (slot << sb) | sample, NO_KEY))


# ---- run lengths ---------------------------------------------------------------------------------------------------------------
RUNS = [63, 64, 65, 1, 2, 300] + [2] * 7 + [1, 129, 128, 1]          # in the array's order, behind one entry that is no key
FRONT, BEHIND_PAST, BEHIND_NONE = 1, 3, 5                             # a negative key; keys past the last slot; INT64_MAX
SLOTS = C * R * T


def _run_layout():
    starts = FRONT + np.concatenate([[0], np.cumsum(RUNS)[:-1]])
    lens = np.array(RUNS)
    ends = starts + lens - 1
    n = FRONT + int(lens.sum()) + BEHIND_PAST + BEHIND_NONE
    assert n <= 2048 and set(RUNS) == {1, 2, 63, 64, 65, 128, 129, 300}
    assert {0, 1, 63} <= set(starts % 64)                             # heads on a wave's first, second and last lane
    assert ((starts // 256) != (ends // 256)).any()                   # a run that crosses a workgroup boundary
    assert ((ends % 64) == 63).any() and (((ends % 64) == 63) & ((starts % 64) != 0)).any()      # ends at a wave's last lane
    return starts, lens, n


def _run_keys(key_of_run, past):
    starts, lens, n = _run_layout()
    keys = np.concatenate([[-5] * FRONT, np.repeat([key_of_run(j) for j in range(len(RUNS))], lens), [past] * BEHIND_PAST,
                           [NO_KEY] * BEHIND_NONE]).astype(np.int64)
    assert keys.shape[0] == n and (np.diff(keys) >= 0).all()          # ascending: an entry without a key can only stand in front
    return keys                                                        # of the runs or behind them


@pytest.mark.parametrize("cap", [0, 2])
def test_run_lengths_through_the_sample_counts(cap):
    sb = 3                                                   # 7 samples and the all-ones field
    keys = _run_keys(lambda j: ((j // 3) << sb) | (j % 3), SLOTS << sb)      # three runs -- three samples -- per tile
    _, lens, n = _run_layout()
    want_cap, want_samples = np.zeros(SLOTS, np.int32), np.zeros(SLOTS, np.int32)
    for j, length in enumerate(lens):
        want_cap[j // 3] += min(length, cap) if cap else length
        want_samples[j // 3] += 1
    for be in _backends():
        p = be.ptr
        k_cap, k_samples = be.empty((C, R, T), "i32"), be.empty((C, R, T), "i32")
        be.call("dig_tile_sample_counts", p(be.arr(keys, "i64")), n, C, R, T, 7, cap, p(k_cap), p(k_samples))
        assert np.array_equal(_host(k_cap).ravel(), want_cap), (be.is_device, _host(k_cap).ravel(), want_cap)
        assert np.array_equal(_host(k_samples).ravel(), want_samples), (be.is_device, _host(k_samples).ravel(), want_samples)


def test_run_lengths_through_the_sparse_test():
    from digdriver_amd import engine
    from digdriver_amd.data_tools.genome import PackedGenome
    rng = np.random.default_rng(5)
    genome = PackedGenome.from_sequences({"1": "".join(rng.choice(list("ACGT"), 200))})
    chroms, starts, ends = ["1"] * R, np.array([10, 60, 110], np.int64), np.array([50, 100, 150], np.int64)      # 40 positions: T tiles each
    s_prob = rng.uniform(0.5, 1.5, (C, 64)) * 1e-3
    mu, sigma = rng.uniform(1.0, 3.0, (C, R)), rng.uniform(0.5, 1.0, (C, R))
    keys = _run_keys(lambda j: j, SLOTS)                    # run j is tile j of the [C, R, T] order
    run_starts, lens, n = _run_layout()
    assert len(RUNS) <= SLOTS
    want_k, want_tile = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    want_k[run_starts], want_tile[run_starts] = lens, np.arange(len(RUNS)) % T
    for be in _backends():
        p = be.ptr
        _, nval, denom, _ = engine.tile_census(genome, chroms, starts, ends, s_prob, BINSIZE, T, on_device=be.is_device)
        assert (_host(nval) == T).all()
        args, held, *_ = engine._tile_genome(be, genome, chroms, starts, ends, s_prob, BINSIZE, T)
        names = ("cohort", "region", "tile", "k", "pt", "exp", "pval")
        out = {k: be.empty(n, "i32" if i < 4 else "f64") for i, k in enumerate(names)}
        be.call("dig_sparse_tile_test", *args, p(be.arr(denom, "f64")), p(be.arr(mu, "f64")), p(be.arr(sigma, "f64")), p(be.arr(keys, "i64")), n,
                *[p(out[k]) for k in names])
        got_k, got_tile = _host(out["k"]), _host(out["tile"])
        assert np.array_equal(got_k, want_k), (be.is_device, np.argwhere(got_k != want_k)[:5])
        assert np.array_equal(got_tile, want_tile)
        assert np.isfinite(_host(out["pval"])[run_starts]).all() and np.isnan(_host(out["pval"])[want_k == 0]).all()
