"""GPU tests of elementDriver --f-sites for many cohorts: engine.site_counts (dig_site_match_count / keys + a key sort + dig_site_counts)
count for count against the plain statement sites_statement.py, in its device-tensor and its host-array form, on the golden cohorts, a
seeded fuzz and the edges of the search and of the counting kernel; the key layout at 63 and 64 bits; cohort_batch.run_sites_cohorts
against run_sites_region_model a cohort at a time; the written files against the elementDriver command line."""
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pandas as pd
import pytest

import sites_cohort_cases as K
import sites_statement as S
from conftest import ROOT

pytestmark = pytest.mark.gpu

W = 64


def three_ways(args):
    """engine.site_counts on device tensors and on host arrays, and the statement: equal count for count.  Returns the planes."""
    import torch
    from digdriver_amd import engine
    B = engine.SITE_COUNT_BLOCK
    assert B % W == 0
    arrays, (off, E, C) = args[:9], args[9:]
    dev = engine.site_counts(*[torch.as_tensor(np.ascontiguousarray(a), device="cuda:0") for a in arrays], off, E, C)
    assert all(v.is_cuda for v in dev.values())
    dev = {k: v.cpu().numpy() for k, v in dev.items()}
    host = engine.site_counts(*arrays, off, E, C)
    want = S.site_counts(*args)
    for k in ("obs_snv", "obs_samples"):
        assert dev[k].dtype == np.int32 and dev[k].shape == (E, C) and host[k].dtype == np.int32
        assert np.array_equal(dev[k], want[k]), k
        assert np.array_equal(host[k], want[k]), k
    return want


def test_golden_cohorts_three_ways(tmp_path):
    f_sites, f_muts = K.write_files(tmp_path)
    args, names, _ = K.encoded(f_sites, f_muts)
    got = three_ways(args)
    for c, name in enumerate(K.COHORTS):
        assert K.count_table(got, names, c) == K.golden_table(name), name


def test_seeded_fuzz_three_ways():
    rng = np.random.default_rng(20261020)
    S_, C, n_c, E = 3000, 3, 4000, 40
    place = np.sort(rng.choice(1 << 20, 500, replace=False)) + (np.int64(3) << 40)     # equal-position runs are common
    site_pos = np.sort(rng.choice(place, S_))
    site_end = site_pos + rng.integers(1, 3, S_)
    site_attr, site_elt = rng.integers(0, 6, S_), rng.integers(0, E, S_).astype(np.int32)
    off = np.array([0, 50, 90, 150], np.int64)
    cohort = np.repeat(np.arange(C), n_c).astype(np.int32)
    rng.shuffle(cohort)                                                                  # rows of the cohorts in any order
    row_pos = rng.choice(place, C * n_c)
    row_end = row_pos + rng.integers(1, 3, C * n_c)
    row_attr = rng.integers(-1, 6, C * n_c)
    sample = (off[cohort] + rng.integers(0, 1 << 30, C * n_c) % (off[cohort + 1] - off[cohort])).astype(np.int32)
    got = three_ways((site_pos, site_end, site_attr, site_elt, row_pos, row_end, row_attr, sample, cohort, off, E, C))
    assert got["obs_snv"].sum() > 3000 and (got["obs_samples"] < got["obs_snv"]).any() and (got["obs_snv"] > 0).all()


def _one_cohort(site, rows, E, n_samples=4):
    """site: (pos, end, attr, elt) rows, sorted here; rows: (pos, end, attr, sample) of one cohort."""
    site = sorted(site)
    col = lambda t, q, dt: np.array([r[q] for r in t], dt)
    return (col(site, 0, np.int64), col(site, 1, np.int64), col(site, 2, np.int64), col(site, 3, np.int32), col(rows, 0, np.int64),
            col(rows, 1, np.int64), col(rows, 2, np.int64), col(rows, 3, np.int32), np.zeros(len(rows), np.int32),
            np.array([0, n_samples], np.int64), E, 1)


def test_search_edges():
    # S = 1; a row below the first site, one above the last, and the hit
    got = three_ways(_one_cohort([(100, 101, 7, 0)], [(99, 101, 7, 0), (101, 101, 7, 1), (100, 101, 7, 2), (100, 101, 7, 2)], 1))
    assert got["obs_snv"].tolist() == [[2]] and got["obs_samples"].tolist() == [[1]]
    # an equal-position run of 9 site rows where only the last one matches; a position present with no attr match; rows outside
    run = [(500, 501, a, 0) for a in range(4)] + [(500, 502, 8, 0) for _ in range(4)] + [(500, 509, 8, 1)]
    site = [(10, 11, 0, 2)] + run + [(900, 901, 0, 2)]
    rows = [(500, 509, 8, 0), (500, 501, 8, 1), (500, 503, 8, 1), (500, 501, -1, 2), (5, 6, 0, 0), (10 ** 6, 10 ** 6 + 1, 0, 3)]
    got = three_ways(_one_cohort(site, rows, 3))
    assert got["obs_snv"][:, 0].tolist() == [0, 1, 0] and got["obs_samples"][:, 0].tolist() == [0, 1, 0]
    # n = 0, a call with zero matches, and no site at all
    for rows in ([], [(500, 501, 8, 1), (11, 11, 0, 0)]):
        got = three_ways(_one_cohort(site, rows, 3))
        assert not got["obs_snv"].any() and not got["obs_samples"].any()
    assert not three_ways(_one_cohort([], [(500, 501, 8, 1)], 3))["obs_snv"].any()


def _from_keys(tuples, E, C, off, rng):
    """Rows whose sorted keys are `tuples` ((cohort, element, global sample), ascending): one site per element, the rows shuffled."""
    assert tuples == sorted(tuples)
    site = (np.arange(E, dtype=np.int64) + 1000, np.arange(E, dtype=np.int64) + 1001, np.zeros(E, np.int64), np.arange(E, dtype=np.int32))
    order = rng.permutation(len(tuples))
    c, e, gs = (np.array([t[q] for t in tuples], np.int64)[order] for q in range(3))
    return site + (e + 1000, e + 1001, np.zeros(len(tuples), np.int64), gs.astype(np.int32), c.astype(np.int32),
                   np.asarray(off, np.int64), E, C)


def _expect(tuples, E, C):
    snv, samples = np.zeros((E, C), np.int32), np.zeros((E, C), np.int32)
    for (c, e, _), k in Counter(tuples).items():
        snv[e, c] += k
        samples[e, c] += 1
    return snv, samples


def test_counting_edges_at_wave_and_workgroup_boundaries():
    from digdriver_amd import engine
    B = engine.SITE_COUNT_BLOCK
    rng = np.random.default_rng(7)
    # one (element, cohort) with B + W + 1 keys of one sample
    got = three_ways(_from_keys([(0, 0, 2)] * (B + W + 1), 1, 1, [0, 4], rng))
    assert got["obs_snv"].tolist() == [[B + W + 1]] and got["obs_samples"].tolist() == [[1]]
    # runs of one (element, sample) that start at key W - 1 and at key B - 1; a cohort and an element boundary inside one wave; the
    # last key alone in its wave
    keys = [(0, 0, 0)] * (W - 1) + [(0, 0, 1)] * 5
    assert len(keys) - 5 == W - 1
    keys += [(0, 0, 2)] * (B - 1 - len(keys))
    assert len(keys) == B - 1
    keys += [(0, 0, 3)] * 4                                                               # across the workgroup boundary
    keys += [(0, 1, 0)] * 2 + [(0, 2, 5)] + [(1, 0, 10)] * 3 + [(1, 2, 11)] * 2           # inside the wave that starts at B
    assert len(keys) < B + W
    keys += [(1, 2, 12)] * (B + 2 * W - len(keys)) + [(1, 2, 13)]
    assert len(keys) % W == 1
    got = three_ways(_from_keys(keys, 3, 2, [0, 10, 20], rng))
    snv, samples = _expect(keys, 3, 2)
    assert np.array_equal(got["obs_snv"], snv) and np.array_equal(got["obs_samples"], samples)
    assert samples[0, 0] == 4 and snv[0, 0] == B + 3 and samples[2, 1] == 3


def test_key_layout_at_63_and_64_bits():
    """31 bits of global sample; cohort E + element needs 32 bits with C = 2 -- the key fits -- and 33 with C = 3: DIG_EINVAL, a
    ValueError from engine.site_counts before anything is allocated.  Argument validation only: tiny arrays."""
    import torch
    from digdriver_amd import _lib, engine
    E = n_samples = (1 << 31) - 1
    site = [np.array([5], np.int64), np.array([6], np.int64), np.array([0], np.int64), np.array([E - 1], np.int32)]
    row = [np.array([5], np.int64), np.array([6], np.int64), np.array([0], np.int64), np.array([n_samples - 1], np.int32),
           np.array([1], np.int32)]
    off, offsets = np.array([0, 1, n_samples], np.int64), np.zeros(1, np.int64)
    want = (((1 * E) + E - 1) << 31) | (n_samples - 1)
    assert want.bit_length() == 63
    h = _lib.host_ptr
    counts, keys = np.full(1, -5, np.int32), np.zeros(1, np.int64)
    _lib.call("dig_site_match_count_host", *map(h, site), 1, E, *map(h, row), h(off), 1, 2, n_samples, h(counts), 0)
    _lib.call("dig_site_match_keys_host", *map(h, site), 1, E, *map(h, row), h(off), 1, 2, n_samples, h(offsets), 1, h(keys), 0)
    assert counts.tolist() == [1] and keys.tolist() == [want]
    t = lambda a: torch.as_tensor(a, device="cuda:0")
    d = _lib.dev_ptr
    tens = [t(a) for a in site + row + [off, offsets]]
    dkeys = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    _lib.call("dig_site_match_keys", *map(d, tens[:4]), 1, E, *map(d, tens[4:9]), d(tens[9]), 1, 2, n_samples, d(tens[10]), 1, d(dkeys),
              _lib.stream_ptr())
    assert dkeys.cpu().tolist() == [want]
    off3 = np.array([0, 1, n_samples, n_samples], np.int64)
    for conv in (lambda a: a, t):
        with pytest.raises(ValueError, match="63 bits"):
            engine.site_counts(*[conv(a) for a in site + row], off3, E, 3)


@pytest.mark.parametrize("which, mode", [("full", "expectation"), ("hit", "factors")])
def test_run_sites_cohorts_equals_the_serial_route(tmp_path, which, mode):
    from digdriver_amd.driver_model import cohort_batch
    from digdriver_amd.driver_model import transfer_tools as tt
    f_sites, f_muts = K.write_files(tmp_path)
    maps = K.write_maps(tmp_path, which, len(f_muts))
    factors = [0.7, 1.3, 0.05]
    kw = dict(scale_by_expectation=True) if mode == "expectation" else dict(scale_factors=factors, scale_by_expectation=False)
    frames = cohort_batch.run_sites_cohorts(f_muts, f_sites, maps, K.KEY, **kw)
    for c, (name, frame) in enumerate(zip(K.COHORTS, frames)):
        serial = tt.run_sites_region_model(f_muts[c], f_sites, maps[c], K.KEY, scale_factor=None if mode == "expectation" else factors[c],
                                           scale_by_expectation=mode == "expectation")
        pd.testing.assert_frame_equal(frame, serial, check_exact=True)
        want = K.golden_table(name)
        assert [int(v) for v in frame.OBS_SNV] == [want.get(n, (0, 0))[1] for n in frame.index]
        assert [int(v) for v in frame.OBS_SAMPLES] == [want.get(n, (0, 0))[0] for n in frame.index]
    assert str(frames[2].OBS_SNV.dtype) == ("int64" if which == "hit" else "float64")


def test_written_files_are_the_command_lines_bytes(tmp_path):
    from digdriver_amd.driver_model import cohort_batch
    f_sites, f_muts = K.write_files(tmp_path)
    maps = K.write_maps(tmp_path, "full", len(f_muts))
    factors = [0.7, 1.3, 0.05]
    frames, paths = cohort_batch.run_and_write_sites_cohorts(f_muts, f_sites, maps, K.KEY, str(tmp_path / "batch"), K.COHORTS,
                                                             scale_factors=factors, scale_by_expectation=False)
    assert len(frames) == 3 and [os.path.basename(p) for p in paths] == [n + ".results.txt" for n in K.COHORTS]
    env = dict(os.environ, PYTHONPATH=ROOT)
    for c, name in enumerate(K.COHORTS):
        subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "DigDriver.py"), "elementDriver", f_muts[c], maps[c], K.KEY,
                               "--f-sites", f_sites, "--scale-factor-manual", repr(factors[c]), "--scale-factor-indel-manual", "1.0",
                               "--outdir", str(tmp_path / "serial"), "--outpfx", name], env=env)
        with open(tmp_path / "serial" / (name + ".results.txt"), "rb") as a, open(paths[c], "rb") as b:
            assert a.read() == b.read(), name
