"""Copy-number training labels (DataExtractor addCnvObjectives) without device tensors: the per-base statement
(cnv_windows_statement.py) against the golden made with the reference's own fetch_cnv_region_avg (tests/golden/make_cnv_golden.py), the
host-side pieces of the product (segment parsing, plain and gzip; the refusals that come before any device work; the exported symbols
and size queries; the command line's arguments), and -- on a machine with a GPU, where the `_host` twins can stage -- the twins against
the golden and the statement bit for bit, windows in any order, and the command line on an HDF5 container."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cnv_windows_statement as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.loads(gzip.open(os.path.join(ROOT, "tests", "golden", "cnv_objectives_golden.json.gz")).read())
IDX = np.array(GOLDEN["idx"], np.int64)
W = GOLDEN["W"]
ORDER = ("mixed", "sparse", "none")
WANT = np.stack([np.array(GOLDEN["labels"][name], np.float64) for name in ORDER], axis=2)         # [N, 3, C]
CHROM_IDS = {str(c): int(c) for c in np.unique(IDX[:, 0])}


def _write(path, rows, opener=open):
    with opener(path, "wt") as f:
        for r in rows:
            f.write("\t".join(str(v) for v in r) + "\n")
    return str(path)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("cnv")
    return [_write(d / (name + ".cnv.bed.txt"), GOLDEN["cohorts"][name]) for name in ORDER]


def _statement(idx=IDX, width=W):
    segs = S.rows_as_arrays([GOLDEN["cohorts"][name] for name in ORDER], CHROM_IDS)
    return S.window_means(idx[:, 0], idx[:, 1], width, *segs, len(ORDER))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- without a device --------------------------------------------------------------------------------------------------------------
def test_statement_reproduces_the_reference_golden_bit_for_bit():
    assert same_bits(_statement(), WANT)


def test_golden_holds_the_cases_it_is_for():
    rows = GOLDEN["cohorts"]["mixed"]
    assert WANT.shape == (60, 3, 3) and W == 100 and (IDX[:, 2] - IDX[:, 1] == W).all()
    assert {int(float(r[3])) for r in rows} >= {0, 1, 2, 3, 8} and any(r[3] == "3.0" for r in rows)
    assert len({tuple(r) for r in rows}) < len(rows)                                                  # duplicate rows
    assert not WANT[:, :, 2].any() and (WANT[:, :, 1].sum(axis=1) == 0).sum() > 40                    # a cohort without rows; windows without a segment
    starts = set(IDX[IDX[:, 0] == 1, 1].tolist())
    ch1 = [(int(r[1]), int(r[2])) for r in rows if r[0] == "1"]
    assert any(e in starts and e - W in starts for _, e in ch1)                                      # ends at a window's end = the next one's start
    assert any(s == max(starts) + W for s, _ in ch1) and any(e == min(starts) for _, e in ch1)       # touches a window from outside
    assert any(s < min(starts) < e for s, e in ch1)                                                  # starts before the first window
    assert any(s // W == (e - 1) // W and e - s < W and s >= min(starts) for s, e in ch1)             # inside a single window
    assert any(s <= min(starts) and e >= max(starts) + W for s, e in ch1)                             # the whole chromosome
    assert any(r[0] in ("3", "chr1") for r in rows)
    assert (WANT[:, :, 0] > 0).any(axis=0).all()                                                     # all three classes


def test_encoded_segments_plain_and_gzip(tmp_path):
    from digdriver_amd.data_tools import objectives
    rows = GOLDEN["cohorts"]["mixed"]
    plain = objectives.encode_cnv_rows(_write(tmp_path / "a.txt", rows), CHROM_IDS)
    zipped = objectives.encode_cnv_rows(_write(tmp_path / "a.txt.gz", rows, gzip.open), CHROM_IDS)
    # a bgzip file is a multi-member gzip file: two members here
    with open(tmp_path / "b.bed.gz", "wb") as f:
        for part in (rows[:30], rows[30:]):
            f.write(gzip.compress("".join("\t".join(r) + "\n" for r in part).encode()))
    members = objectives.encode_cnv_rows(str(tmp_path / "b.bed.gz"), CHROM_IDS)
    seen = [r for r in rows if r[0] in CHROM_IDS]
    assert len(seen) == len(rows) - 2                                                                 # '3' and 'chr1' are not in idx
    col, wt = S.class_and_weight([int(float(r[3])) for r in seen])
    for enc in (plain, zipped, members):
        assert [enc[k].dtype for k in ("chrom", "start", "end", "klass", "weight")] == [np.int64] * 3 + [np.uint8, np.int32]
        assert enc["chrom"].tolist() == [int(r[0]) for r in seen] and enc["start"].tolist() == [int(r[1]) for r in seen]
        assert enc["end"].tolist() == [int(r[2]) for r in seen]
        assert enc["klass"].tolist() == col.tolist() and enc["weight"].tolist() == wt.tolist()
    assert set(plain["klass"].tolist()) == {0, 1, 2} and plain["weight"].max() == 6
    (tmp_path / "empty.txt").write_text("")
    assert len(objectives.encode_cnv_rows(str(tmp_path / "empty.txt"), CHROM_IDS)["chrom"]) == 0
    # a blank line is no row, and the lines keep their numbers
    (tmp_path / "blank.txt").write_text("1\t5\t9\t3\t2\t1\tD\n\n1\t5\t9\t2.5\t2\t1\tD\n")
    with pytest.raises(ValueError, match=r"blank\.txt, line 3: cp_num"):
        objectives.encode_cnv_rows(str(tmp_path / "blank.txt"), CHROM_IDS)


@pytest.mark.parametrize("row, what", [
    (("1", 10, 20, "2.5", 1, 1, "D"), "cp_num"), (("1", 10, 20, "", 1, 1, "D"), "cp_num"), (("1", 10, 20, "-1", 1, 1, "D"), "cp_num"),
    (("1", 10, 20, "NA", 1, 1, "D"), "cp_num"), (("9", 10, 20, "1e-1", 1, 1, "D"), "cp_num"),
    (("1", 20, 20, "3", 1, 1, "D"), "end <= start"), (("1", 21, 20, "3", 1, 1, "D"), "end <= start"),
    (("1", "x", 20, "3", 1, 1, "D"), "start and end"), (("1", -5, 20, "3", 1, 1, "D"), "start and end"),
])
def test_bad_segments_are_refused_with_file_and_line_before_any_device_work(tmp_path, monkeypatch, row, what):
    from digdriver_amd import engine
    from digdriver_amd.data_tools import objectives

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(engine, "window_cnv_means", no_device)
    good = ("1", 1000, 1100, "3.0", 2, 1, "D")
    f = _write(tmp_path / "bad.txt", [good, good, row, good])
    with pytest.raises(ValueError, match=r"bad\.txt, line 3: .*%s" % what):
        objectives.window_cnv_objectives(IDX, [f], on_device=False)


def test_existing_name_is_refused_before_any_device_work(tmp_path, monkeypatch, files):
    from digdriver_amd import engine
    from digdriver_amd.data_tools import objectives
    from digdriver_amd.io import mapfile

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(engine, "window_cnv_means", no_device)
    for data in (str(tmp_path / "train.map"), str(tmp_path / "train.h5")):
        mapfile.write_array(data, "idx", IDX.astype(np.int32))
        mapfile.write_array(data, "mixed.cnv_x", np.zeros((len(IDX), 3)))
        with pytest.raises(ValueError, match="name already exists"):
            objectives.add_cnv_objectives(data, files[0], suffix="_x")
        with pytest.raises(ValueError, match="two segment files"):
            objectives.add_cnv_objectives(data, [files[0], str(tmp_path / "other" / "mixed.cnv.txt")])
    with pytest.raises(ValueError, match="no segment file"):
        objectives.window_cnv_objectives(IDX, [])
    with pytest.raises(ValueError, match="window width"):
        objectives.window_cnv_objectives(np.array([[1, 50, 50]]), files[:1])


def test_entry_points_are_exported_and_their_twins_check_before_touching_the_device():
    import ctypes
    from digdriver_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dig_hip.h")).read()
    for name in ("dig_cnv_segment_deltas", "dig_cnv_window_means"):
        assert hasattr(lib, name) and hasattr(lib, name + "_host") and hasattr(lib, name + "_size")
        assert name in _lib.EXPORTED_SYMBOLS and name + "_host" in _lib.EXPORTED_SYMBOLS and name + "_size" in _lib._SIZE_QUERIES
        assert _lib._SIGNATURES[name][-1] is ctypes.c_void_p and _lib._SIGNATURES[name + "_host"][-1] is ctypes.c_int
        assert name + "(" in header and name + "_host(" in header and name + "_size(" in header
    assert _lib._SIGNATURES["dig_cnv_segment_deltas_host"][:-1] == _lib._SIGNATURES["dig_cnv_segment_deltas"][:-1]
    assert _lib._SIGNATURES["dig_cnv_window_means_host"][:-1] == _lib._SIGNATURES["dig_cnv_window_means"][:-2]      # the twin stages the carries
    assert "#define DIG_CNV_SCAN_CHUNK %d\n" % _lib.DIG_CNV_SCAN_CHUNK in header and _lib.DIG_CNV_SCAN_CHUNK == 2048
    K = _lib.DIG_CNV_SCAN_CHUNK
    sizes = lambda C, N: (int(lib.dig_cnv_segment_deltas_size(C, N)), int(lib.dig_cnv_window_means_size(C, N)))
    assert sizes(1, 0) == (24, 0) and sizes(2, 5) == (2 * 3 * 6 * 8, 2 * 3 * 8) and sizes(5, K) == (15 * (K + 1) * 8, 15 * 8)
    assert sizes(5, K + 1) == (15 * (K + 2) * 8, 30 * 8) and sizes(37, 288_000) == (111 * 288_001 * 8, 111 * 141 * 8)
    assert sizes(0, 5) == (-1, -1) and sizes(1, -1) == (-1, -1) and sizes(1 << 20, 1 << 30) == (-1, -1)
    i64 = lambda *v: np.array(v, np.int64)
    p = _lib.host_ptr
    ok = dict(win_start=i64(0, 100, 50), chrom_id=i64(1, 2), chrom_off=i64(0, 2, 3), seg=(i64(1), i64(10), i64(20)), klass=np.array([0], np.uint8),
              weight=np.array([1], np.int32), cohort=np.array([0], np.int32), W=100, C=1)
    deltas = np.zeros(3 * 4, np.int64)

    def refused(fragment, **change):
        a = dict(ok, **change)
        with pytest.raises(_lib.DigHipError, match=fragment) as exc:
            _lib.call("dig_cnv_segment_deltas_host", p(a["win_start"]), p(a["chrom_id"]), p(a["chrom_off"]), len(a["chrom_id"]), 3, a["W"],
                      p(a["seg"][0]), p(a["seg"][1]), p(a["seg"][2]), p(a["klass"]), p(a["weight"]), p(a["cohort"]), 1, a["C"], p(deltas), 0)
        assert "dig_cnv_segment_deltas_host: requirement failed" in str(exc.value)

    refused("W within", W=0)
    refused("C within", C=0)
    refused("chrom_off: 0 first, N last", chrom_off=i64(0, 2, 2))
    refused("chrom_id ascending", chrom_id=i64(2, 1))
    refused("window starts distinct and ascending", win_start=i64(100, 100, 50))
    refused("0 <= start < end", seg=(i64(1), i64(20), i64(20)))
    refused("class within", klass=np.array([3], np.uint8))
    refused("class within", weight=np.array([0], np.int32))
    refused("cohort within", cohort=np.array([1], np.int32))
    with pytest.raises(_lib.DigHipError, match="dig_cnv_window_means_host: requirement failed: non-null pointers"):
        _lib.call("dig_cnv_window_means_host", None, 3, 1, 100, None, 0)
    with pytest.raises(_lib.DigHipError, match="dig_cnv_window_means_host: requirement failed: N within"):
        _lib.call("dig_cnv_window_means_host", p(deltas), -1, 1, 100, p(np.zeros(9)), 0)


def test_engine_refuses_bad_windows_and_sizes_as_value_errors():
    from digdriver_amd import engine
    z, b, i = np.zeros(0, np.int64), np.zeros(0, np.uint8), np.zeros(0, np.int32)
    with pytest.raises(ValueError, match="starts within"):
        engine.window_cnv_means([1], [-5], 100, z, z, z, b, i, i, 1)
    with pytest.raises(ValueError, match="C within"):
        engine.window_cnv_means([1], [5], 100, z, z, z, b, i, i, 0)
    with pytest.raises(ValueError, match="W within"):
        engine.window_cnv_means([1], [5], 0, z, z, z, b, i, i, 1)


def test_command_line_arguments():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import DataExtractor as cli
    finally:
        sys.path.pop(0)
    a = cli.parse_args(["addCnvObjectives", "d.h5", "a.bed.gz", "b.txt", "--suffix", "_cnv"])
    assert (a.h5_file, a.cnv_file, a.suffix, a.func) == ("d.h5", ["a.bed.gz", "b.txt"], "_cnv", cli.add_cnv_objectives)
    assert cli.parse_args(["addCnvObjectives", "d.h5", "a.txt"]).suffix == ""
    with pytest.raises(SystemExit, match="not built.*addCnvObjectives"):
        cli.add_objectives(cli.parse_args(["addObjectives", "d.h5", "m.txt", "--cnv"]))
    for other in ("addTracks", "mappability", "createChunk"):
        with pytest.raises(SystemExit):
            cli.parse_args([other, "d.h5"])


# ---- the `_host` twins: they stage through a device ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_host_twins_equal_the_golden_and_the_statement(files):
    from digdriver_amd.data_tools import objectives
    names, labels = objectives.window_cnv_objectives(IDX, files, on_device=False)
    assert names == ["mixed.cnv", "sparse.cnv", "none.cnv"]
    assert labels.dtype == np.float64 and same_bits(labels, WANT) and same_bits(labels, _statement())
    # one file is its column of the batch
    assert same_bits(objectives.window_cnv_objectives(IDX, files[1], on_device=False)[1][:, :, 0], WANT[:, :, 1])


@pytest.mark.gpu
def test_windows_unsorted_repeated_overlapping_and_of_other_widths(files, tmp_path):
    """Stride 40 at W = 100 (an --overlap container), shuffled, some rows twice, END - START of the later rows not W: every row is
    [START, START + W) with W from the first row, and the answer is the statement's, row by row."""
    from digdriver_amd.data_tools import objectives
    rng = np.random.default_rng(3)
    idx = np.array([(c, s, s + W) for c in (1, 2, 7) for s in range(0, 3_200, 40)] + [(5, 0, W), (5, 40, 40 + W)], np.int64)
    idx = np.concatenate([idx, idx[rng.integers(0, len(idx), 25)]])[rng.permutation(len(idx) + 25)]
    idx[1:, 2] += rng.integers(-30, 30, len(idx) - 1)                     # only the first row's width counts
    gz = _write(tmp_path / "mixed.txt.gz", GOLDEN["cohorts"]["mixed"], gzip.open)
    names, labels = objectives.window_cnv_objectives(idx, [gz, files[1], files[2]], on_device=False)
    want = _statement(idx)
    assert names == ["mixed", "sparse.cnv", "none.cnv"] and same_bits(labels, want)
    assert (want[idx[:, 0] == 5] == 0).all() and (want[:, :, 0].sum(axis=0) > 0).all()     # chromosome 5 has no row in any file
    rep = [np.flatnonzero((idx[:, :2] == row[:2]).all(axis=1)) for row in idx]
    assert max(len(r) for r in rep) >= 2 and all(same_bits(labels[r[0]], labels[j]) for r in rep for j in r)


@pytest.mark.gpu
def test_command_line_extends_an_hdf5_container_in_place(files, tmp_path):
    from digdriver_amd.io import mapfile
    h5 = str(tmp_path / "train.h5")
    rng = np.random.default_rng(5)
    x = rng.integers(0, 100, (len(IDX), 10, 3)).astype(np.float32)
    mapfile.write_array(h5, "x_data", x)
    mapfile.write_array(h5, "idx", IDX.astype(np.int32))
    size = os.path.getsize(h5)
    head = open(h5, "rb").read()
    assert x.tobytes() in head
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "DataExtractor.py"), "addCnvObjectives", h5, files[0], files[1], files[2],
           "--suffix", "_v1"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Saving dataset as mixed.cnv_v1" in r.stdout and "Adding CNV counts from %s to %s" % (files[2], h5) in r.stdout
    body = open(h5, "rb").read()
    assert len(body) > size and sum(a != b for a, b in zip(head[96:], body[96:size])) <= 16     # the root header's symbol-table message, nothing else
    assert x.tobytes() in body[:size] and same_bits(mapfile.read_array(h5, "x_data"), x)
    for c, name in enumerate(("mixed.cnv_v1", "sparse.cnv_v1", "none.cnv_v1")):
        got = mapfile.read_array(h5, name)
        assert got.shape == (len(IDX), 3) and same_bits(np.asarray(got), np.ascontiguousarray(WANT[:, :, c]))
    assert np.array_equal(mapfile.read_array(h5, "idx"), IDX)
    # a second run under the same names is refused, as create_dataset refuses it; so is a bad segment, with its line
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode != 0 and "name already exists" in r.stderr
    bad = _write(tmp_path / "bad.txt", [("1", 10, 20, "2.5", 1, 1, "D")])
    r = subprocess.run(cmd[:4] + [bad], capture_output=True, text=True)
    assert r.returncode != 0 and "bad.txt, line 1: cp_num" in r.stderr and not mapfile.has_key(h5, "bad")
    # a directory mirror takes the same call
    from digdriver_amd.data_tools import objectives
    d = str(tmp_path / "train.map")
    mapfile.write_array(d, "idx", IDX.astype(np.int32))
    assert objectives.add_cnv_objectives(d, files[0], on_device=False) == ["mixed.cnv"]
    assert same_bits(mapfile.read_array(d, "mixed.cnv"), np.ascontiguousarray(WANT[:, :, 0]))
