"""DigPretrain sequenceModels on the GPU: engine.sequence_counts (dig_overlap_join_* + dig_sequence_counts) on device tensors, through
the `_host` twins and as the plain statement (sequence_counts_statement.py) must be equal, count for count; the golden cohorts also
equal the reference's tables (tests/golden/make_sequence_models_golden.py).  Everything is integer counting: equality is exact.

The counting kernel runs one thread per (row, window) pair in workgroups of 1 024 = 16 waves and keeps LDS counters for the cohort
of the workgroup's first pair; the shapes put cohort boundaries inside a wave, a row's pairs across waves and across a workgroup
boundary, and one counter past 65 535."""
import json
import os

import numpy as np
import pytest

import sequence_counts_statement as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = json.load(open(os.path.join(ROOT, "tests", "golden", "sequence_models_golden.json")))
IDX = np.array(FX["idx"], np.int64)
MAPP = np.array(FX["mappability"])
WINDOWS = [(1, 0, 100), (1, 100, 200), (1, 150, 260), (1, 400, 500), (1, 400, 500), (2, 0, 1000)]


def three_ways(windows, rows, K, C):
    """counts of the device route; the host twin and the statement must give the same."""
    import torch
    from digdriver_amd import engine
    win = np.array(windows, np.int64).reshape(-1, 3)
    chrom, start, end, typ, cohort = (np.ascontiguousarray(x) for x in rows)
    want = S.sequence_counts(win[:, 0], win[:, 1], win[:, 2], chrom, start, end, typ, cohort, K, C)
    host = engine.sequence_counts(win[:, 0], win[:, 1], win[:, 2], chrom, start, end, typ, cohort, K, C)
    dev = engine.sequence_counts(win[:, 0], win[:, 1], win[:, 2], *[torch.as_tensor(x, device="cuda") for x in (chrom, start, end, typ, cohort)],
                                 K, C)
    assert isinstance(host, np.ndarray) and host.dtype == np.int64 and host.shape == (C, K)
    assert dev.is_cuda and dev.dtype == torch.int64 and tuple(dev.shape) == (C, K)
    dev = dev.cpu().numpy()
    assert np.array_equal(host, want), np.argwhere(host != want)[:5]
    assert np.array_equal(dev, want), np.argwhere(dev != want)[:5]
    return dev


def one_base(chrom, start, typ, cohort):
    start = np.asarray(start, np.int64)
    return (np.full(len(start), chrom, np.int64) if np.isscalar(chrom) else np.asarray(chrom, np.int64), start, start + 1,
            np.asarray(typ, np.int32), np.asarray(cohort, np.int32))


def cat(*parts):
    return tuple(np.concatenate([p[j] for p in parts]) for j in range(5))


@pytest.fixture(scope="module")
def golden_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("sequence_models")
    files = []
    for name in ("none", "long", "big"):
        (d / (name + ".annot.txt")).write_text(FX["cohorts"][name])
        files.append(str(d / (name + ".annot.txt")))
    return files


def test_three_golden_cohorts_in_one_pass(golden_files):
    from digdriver_amd.sequence_model import sequence_tools as st
    keep = MAPP > FX["map_thresh"]
    white = IDX[keep]
    enc = [st.encode_sequence_rows(f, {"1": 1, "2": 2, "3": 3}) for f in golden_files]
    rows = tuple(np.concatenate([e[k] for e in enc]) for k in ("chrom", "start", "end", "type")) + \
        (np.repeat(np.arange(3, dtype=np.int32), [len(e["type"]) for e in enc]),)
    got = three_ways(white, rows, 192, 3)
    want = {m["cohort"]: m["COUNT"] for m in FX["models"]}
    assert got[0].tolist() == want["none"] and got[2].tolist() == want["big"]
    # `long` holds rows of several bases: the kernel's rule counts each once, the reference each distinct piece -- the public route
    # therefore counts that cohort on the host
    assert got[1].sum() < sum(want["long"])
    frame = S.genome_frame(len(IDX), list(st.mk_context_sequences(1, 1).keys()))
    for on_device in (True, False):
        models, counts, serial = st.train_sequence_models(golden_files, IDX, MAPP, frame, map_thresh=FX["map_thresh"], on_device=on_device)
        assert serial == [1]
        assert [c.tolist() for c in counts] == [want["none"], want["long"], want["big"]]
        assert [int(v) for v in models[2][0].COUNT] == want["big"]


def test_cohort_boundaries_inside_a_wave_and_cohorts_without_pairs():
    rng = np.random.default_rng(5)
    K = 192
    # cohort 0: 100 rows (its last pairs share a wave with cohort 2's first); cohort 1: no row; cohort 2: 150 rows, some in the
    # two overlapping and in the doubled windows; cohort 3: 37 rows, none in a window; 287 rows, no multiple of 64
    rows = cat(one_base(1, rng.integers(0, 260, 100), rng.integers(0, K + 1, 100), np.zeros(100)),
               one_base(1, rng.integers(100, 500, 150), rng.integers(0, K + 1, 150), np.full(150, 2)),
               one_base(np.r_[np.full(20, 1), np.full(17, 3)], np.r_[rng.integers(260, 400, 20), rng.integers(0, 100, 17)],
                        rng.integers(0, K, 37), np.full(37, 3)))
    got = three_ways(WINDOWS, rows, K, 4)
    assert got[0].sum() > 0 and got[2].sum() > 0 and got[1].sum() == 0 and got[3].sum() == 0
    # many small cohorts inside one workgroup, in an order that is not ascending: every pair but the home cohort's adds directly
    n = 333
    cohort = rng.permutation(np.repeat(np.arange(9), 37))
    three_ways(WINDOWS, one_base(1, rng.integers(0, 200, n), rng.integers(0, K + 1, n), cohort), K, 9)


@pytest.mark.parametrize("K", [192, 3072])
def test_one_counter_passes_65535(K):
    """70 000 rows of one type in one cohort: 69 workgroups flush the same address, and a 16-bit partial counter would wrap."""
    rng = np.random.default_rng(K)
    hot = K // 3 + 1
    rows = cat(one_base(2, rng.integers(0, 1000, 70_000), np.full(70_000, hot), np.zeros(70_000)),
               one_base(2, rng.integers(0, 1000, 5_000), np.arange(5_000) % K, np.zeros(5_000)))
    order = rng.permutation(75_000)
    got = three_ways(WINDOWS, tuple(x[order] for x in rows), K, 1)
    assert got[0, hot] > 65_535 + 5_000 // K and (got[0] > 0).all() and got.sum() == 75_000


def test_a_rows_pairs_across_waves_and_workgroups_count_once():
    """One row in 300 copies of a window, behind 900 one-pair rows: its pairs are 900 .. 1199 of the pair list -- waves 14 to 18,
    workgroups 0 and 1 -- and it is the last row of cohort 0; the first row of cohort 1 lies in the same 300 windows."""
    K = 192
    windows = [(1, 0, 1000)] * 300 + [(1, 2000, 3000)]
    rows = cat(one_base(1, 2000 + np.arange(900), np.arange(900) % K, np.zeros(900)),
               one_base(1, [500], [7], [0]), one_base(1, [600], [7], [1]), one_base(1, [2500, 700], [8, K], [1, 1]))
    got = three_ways(windows, rows, K, 2)
    assert got[0, 7] == 900 // K + 1 + 1 and got[1, 7] == 1 and got[1, 8] == 1 and got[1].sum() == 2


def test_rows_without_a_table_entry_and_no_pairs_give_zeros():
    K = 192
    rng = np.random.default_rng(1)
    assert three_ways(WINDOWS, one_base(1, rng.integers(0, 500, 700), np.full(700, K), rng.integers(0, 2, 700)), K, 2).sum() == 0
    # rows, but no pair; no row at all; no window at all
    assert three_ways(WINDOWS, one_base(3, rng.integers(0, 500, 70), rng.integers(0, K, 70), np.zeros(70)), K, 2).sum() == 0
    assert three_ways(WINDOWS, one_base(1, [], [], []), K, 2).sum() == 0
    assert three_ways([], one_base(1, [5, 6], [1, 2], [0, 1]), K, 2).sum() == 0


def test_refusals_come_as_value_errors_on_both_backends():
    import torch
    from digdriver_amd import engine
    win = np.array(WINDOWS, np.int64)
    good = one_base(1, [5, 6, 7], [0, 1, 2], [0, 1, 1])
    for conv in (lambda x: x, lambda x: torch.as_tensor(x, device="cuda")):
        call = lambda rows, K, C: engine.sequence_counts(win[:, 0], win[:, 1], win[:, 2], *[conv(x) for x in rows], K, C)
        assert call(good, 3, 2).sum() == 3
        with pytest.raises(ValueError, match="K"):
            call(good, 0, 2)
        with pytest.raises(ValueError, match="cohort within"):
            call(good, 3, 1)                                            # a cohort id = C
        with pytest.raises(ValueError, match="type within"):
            call(good, 1, 2)                                            # a type = K + 1
        with pytest.raises(ValueError, match="C"):
            call(good, 3, 0)
