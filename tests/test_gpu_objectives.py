"""DataExtractor addObjectives for many cohorts on the GPU: dig_overlap_join_* + dig_window_pair_keys + a key sort +
dig_window_sample_hits + dig_window_objectives, the device route and the `_host` twins, against the golden made with the reference's
own sample filters (tests/golden/make_objectives_golden.py) and the plain statement (objectives_statement.py).  Everything is integer
counting: equality is exact.

Shapes: 300 windows on 3 chromosomes (gaps on two, back to back on one, one chromosome listed in descending order), C = 3 cohorts in
one pass -- `none` (no row on a chromosome of idx), `single` (one sample: std = NaN), `big` (about 2 000 rows: a (sample, window) run of
700 keys, i.e. eleven waves and three workgroups of the counting kernels, repeated rows, repeats that disagree on ANNOT, indels across
window edges, rows on chromosomes idx does not hold, a sample exactly on and one a window above the plain limit, and loads one apart on
either side of the standard-deviation limit)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import objectives_statement as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "objectives_golden.json")))
IDX = np.array(GOLDEN["idx"], np.int32)
ORDER = ("none", "single", "big")


def _rows(name):
    return [tuple(r) for r in GOLDEN["cohorts"][name]]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("objectives")
    out = []
    for name in ORDER:
        path = d / (name + ".annot.txt")
        with open(path, "w") as f:
            for r in _rows(name):
                f.write("\t".join(str(v) for v in r) + "\n")
        out.append(str(path))
    return out


_STATEMENT = {}


def _statement(options):
    key = json.dumps(options, sort_keys=True)
    if key not in _STATEMENT:
        _STATEMENT[key] = np.array([S.window_labels(IDX, _rows(name), **options) for name in ORDER], np.float64).T
    return _STATEMENT[key]


@pytest.mark.parametrize("on_device", [True, False], ids=["device", "host_twin"])
def test_three_cohorts_in_one_pass_equal_the_golden_and_the_statement(files, on_device):
    from digdriver_amd.data_tools import objectives
    seen = set()
    for case in GOLDEN["cases"]:
        opts = case["options"]
        key = json.dumps(opts, sort_keys=True)
        if key not in seen:
            seen.add(key)
            names, labels = objectives.window_objectives(IDX, files, on_device=on_device, **opts)
            assert names == list(ORDER) and labels.shape == (len(IDX), 3) and labels.dtype == np.float64
            assert np.array_equal(labels, _statement(opts)), opts
        assert np.array_equal(labels[:, ORDER.index(case["cohort"])], np.array(case["labels"], np.float64)), case["options"]
    assert len(seen) >= 9


def test_one_file_is_the_column_of_the_batch_and_the_routes_agree(files):
    from digdriver_amd.data_tools import objectives
    m, k = GOLDEN["big_plain_limit"], GOLDEN["big_stdev_factor"]
    _, batch = objectives.window_objectives(IDX, files, max_muts_per_sample=m, sample_filter_stdev=k, on_device=True)
    names, one = objectives.window_objectives(IDX, files[2], max_muts_per_sample=m, sample_filter_stdev=k, on_device=True)
    _, host = objectives.window_objectives(IDX, files[2], max_muts_per_sample=m, sample_filter_stdev=k, on_device=False)
    assert names == ["big"] and np.array_equal(one[:, 0], batch[:, 2]) and np.array_equal(host, one)
    # windows listed twice carry one name in the reference's frame: both get the label, the sample's load counts them once
    twice = np.concatenate([IDX, IDX[:40]])
    _, lab2 = objectives.window_objectives(twice, files[2], max_muts_per_sample=m, sample_filter_stdev=k, on_device=True)
    assert np.array_equal(lab2[:len(IDX)], one) and np.array_equal(lab2[len(IDX):], one[:40])


def test_engine_operation_on_hand_made_rows():
    """The kernels on rows whose answer can be read off: duplicates, an indel, a row on a chromosome id the windows do not have,
    a sample that is not kept, a pair of windows in descending order."""
    import torch
    from digdriver_amd import engine
    win = np.array([[2, 100, 200], [1, 300, 400], [1, 100, 200]], np.int64)
    #        chrom start end sample uid indel
    rows = np.array([[1, 110, 111, 0, 0, 0], [1, 110, 111, 0, 0, 0],           # a repeated row: once
                     [1, 120, 121, 0, 1, 0],
                     [1, 130, 133, 1, 2, 1],                                   # an indel: a hit, no label
                     [1, 150, 350, 1, 3, 0],                                   # spans two windows: both
                     [2, 150, 151, 2, 0, 0], [2, 150, 151, 3, 0, 0],           # cohort 1 (samples 2, 3): the same uid, two samples
                     [9, 150, 151, 3, 1, 0],                                   # no such chromosome
                     [1, 390, 391, 3, 2, 0], [1, 190, 391, 3, 4, 0]], np.int64)
    offs = [0, 2, 4]
    want_hits = [1, 2, 1, 3]
    want = {True: [[0, 2], [1, 2], [3, 1]], False: [[0, 1], [1, 0], [3, 0]]}          # all samples kept | sample 3 dropped
    for dev in (True, False):
        cols = [rows[:, j] for j in range(6)]
        if dev:
            cols = [torch.as_tensor(c, device="cuda:0") for c in cols]
        for drop in (True, False):
            seen = []

            def keep(h, drop=drop):
                seen.append(h.tolist())
                return np.array([1, 1, 1, 0 if drop else 1], np.uint8)
            out = engine.window_objectives(win[:, 0], win[:, 1], win[:, 2], *cols, offs, 5, keep_from_hits=keep)
            labels = out["labels"].cpu().numpy() if dev else out["labels"]
            assert seen == [want_hits] and out["hits"].tolist() == want_hits
            assert labels.dtype == np.float64 and labels.tolist() == [[float(v) for v in r] for r in want[not drop]], (dev, drop)
    # no rows at all, and no windows at all
    empty = [np.zeros(0, np.int64)] * 6
    out = engine.window_objectives(win[:, 0], win[:, 1], win[:, 2], *empty, [0, 0], 1)
    assert out["labels"].tolist() == [[0.0]] * 3 and len(out["hits"]) == 0
    out = engine.window_objectives(*[np.zeros(0, np.int64)] * 3, *[rows[:, j] for j in range(6)], offs, 5)
    assert out["labels"].shape == (0, 2) and out["hits"].tolist() == [0, 0, 0, 0]


def test_command_line_on_a_directory_mirror_then_the_trainer_reads_the_labels(files, tmp_path):
    import torch
    from digdriver_amd.io import mapfile
    from digdriver_amd.region_model import kfold_mutations_main as kf
    data = str(tmp_path / "train.map")
    N = len(IDX)
    rng = np.random.default_rng(5)
    mapfile.write_array(data, "x_data", rng.integers(0, 100, (N, 10, 3)).astype(np.float32))
    mapfile.write_array(data, "idx", IDX)
    mapfile.write_array(data, "mappability", rng.uniform(0.6, 1.0, N))
    m = GOLDEN["big_plain_limit"]
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "DataExtractor.py"), "addObjectives", data, files[2], files[1],
           "--max-muts-per-sample", str(m), "--max-muts-per-elt-per-sample", "1", "--suffix", "_v1"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Saving dataset as big_v1" in r.stdout and "Saving dataset as single_v1" in r.stdout
    want = _statement({"max_muts_per_sample": m})
    args = kf.get_cmd_arguments("-c big_v1 single_v1 -d %s -o %s -k 2" % (data, tmp_path))
    loaded = kf.KFoldData(args, torch.device("cuda", 0))
    assert np.array_equal(loaded.labels[0], want[:, 2]) and np.array_equal(loaded.labels[1], want[:, 1])
    assert mapfile.read_array(data, "big_v1").dtype == np.float64
    # a second run under the same names is refused, as create_dataset refuses it
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode != 0 and "name already exists" in r.stderr
    # the HDF5 container is extended in place
    h5 = str(tmp_path / "train.h5")
    mapfile.write_array(h5, "idx", IDX)
    size = os.path.getsize(h5)
    head = open(h5, "rb").read()[96:size]
    r = subprocess.run(cmd[:3] + [h5, files[2]], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(mapfile.read_array(h5, "big"), _statement({})[:, 2]) and np.array_equal(mapfile.read_array(h5, "idx"), IDX)
    body = open(h5, "rb").read()[96:size]
    assert sum(a != b for a, b in zip(head, body)) <= 16              # the symbol-table message of the root header, nothing else
