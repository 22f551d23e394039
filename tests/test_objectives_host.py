"""CPU-only checks of DataExtractor addObjectives for many cohorts: the plain statement (objectives_statement.py) against the golden
made with the reference's own sample filters (tests/golden/make_objectives_golden.py), the host-side pieces of the product (row
encoding, sample thresholds, name rule) against the statement and the golden, the exported symbols, and the refusals that come before
any device work.  The kernels themselves run in test_gpu_objectives.py."""
import json
import os
import sys

import numpy as np
import pytest

import objectives_statement as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "objectives_golden.json")))
IDX = np.array(GOLDEN["idx"], np.int64)


def _rows(name):
    return [tuple(r) for r in GOLDEN["cohorts"][name]]


def _write(path, rows):
    with open(path, "w") as f:
        for r in rows:
            f.write("\t".join(str(v) for v in r) + "\n")
    return str(path)


@pytest.mark.parametrize("case", range(len(GOLDEN["cases"])))
def test_statement_reproduces_the_reference_golden(case):
    c = GOLDEN["cases"][case]
    assert S.window_labels(IDX, _rows(c["cohort"]), **c["options"]) == c["labels"]


def test_golden_holds_the_cases_it_is_for():
    """The ineffective cap, the zeros that switch nothing on, the one-sample cohort, and a sample on and one above each cut-off."""
    cases = {(c["cohort"], json.dumps(c["options"], sort_keys=True)): c["labels"] for c in GOLDEN["cases"]}
    base = cases[("big", "{}")]
    m, k = GOLDEN["big_plain_limit"], GOLDEN["big_stdev_factor"]
    loads = sorted(GOLDEN["big_sample_loads"].values())
    assert m in loads and m + 1 in loads
    std = S.stdev(loads)
    below = max(n for n in loads if n <= std * k)
    assert below + 1 in loads and below < std * k < below + 1
    assert cases[("big", json.dumps({"max_muts_per_elt_per_sample": 1}))] == base                       # the cap changes nothing
    assert cases[("big", json.dumps({"max_muts_per_elt_per_sample": 0, "max_muts_per_sample": 0, "sample_filter_stdev": 0.0},
                                    sort_keys=True))] == base                                           # 0 is off
    assert cases[("big", json.dumps({"max_muts_per_sample": m}))] != base
    assert cases[("single", json.dumps({"sample_filter_stdev": 0.5}))] == cases[("single", "{}")]       # std of one sample: NaN
    assert max(base) >= 600                                                                             # the 700-row run, de-duplicated


def test_encoded_rows_and_thresholds_give_the_statements_samples(tmp_path):
    """encode_objective_rows keeps what the join can see, and keep_samples drops exactly the samples the statement drops."""
    from digdriver_amd.data_tools import objectives
    rows = _rows("big")
    chrom_ids = {str(c): int(c) for c in np.unique(IDX[:, 0])}
    enc = objectives.encode_objective_rows(_write(tmp_path / "big.annot.txt", rows), chrom_ids)
    seen = [r for r in rows if r[0] in chrom_ids]
    assert len(enc["chrom"]) == len(seen) < len(rows)                                # 3, X and 'chr1' are not in idx
    assert enc["sample"].dtype == np.int32 and enc["uid"].dtype == np.int32 and enc["indel"].dtype == np.uint8
    assert [enc["sample_names"][s] for s in enc["sample"]] == [r[5] for r in seen]
    ident = {}
    for r, u in zip(seen, enc["uid"].tolist()):
        assert ident.setdefault(r[:5], u) == u                                       # one id per (CHROM, START, END, REF, ALT)
    assert len(set(ident.values())) == len(ident) == enc["n_uid"]
    # rows that disagree on ANNOT take the class of the first row of their (mutation, sample)
    first = {}
    for r in seen:
        first.setdefault((r[:5], r[5]), r[7] == "INDEL")
    assert enc["indel"].tolist() == [int(first[(r[:5], r[5])]) for r in seen]
    assert sum(int(first[(r[:5], r[5])]) != int(r[7] == "INDEL") for r in seen) == 2
    _table, loads = S.sample_loads(IDX, rows)
    hits = np.array([loads.get(s, 0) for s in enc["sample_names"]], np.int32)
    offs = np.array([0, len(hits)])
    m, k = GOLDEN["big_plain_limit"], GOLDEN["big_stdev_factor"]
    limit = S.stdev(list(loads.values())) * k
    for kw in (dict(), dict(max_muts_per_sample=m), dict(sample_filter_stdev=k), dict(max_muts_per_sample=m, sample_filter_stdev=k),
               dict(max_muts_per_sample=0, sample_filter_stdev=0.0), dict(max_muts_per_sample=1)):
        want = np.ones(len(hits), bool)
        if kw.get("sample_filter_stdev"):
            want &= ~(hits > limit)
        if kw.get("max_muts_per_sample"):
            want &= ~(hits > kw["max_muts_per_sample"])
        assert objectives.keep_samples(hits, offs, **kw).astype(bool).tolist() == want.tolist(), kw
    assert objectives.keep_samples(hits, offs, max_muts_per_sample=m).sum() == len(hits) - 1            # 41 goes, 40 stays
    # a sample that hits nothing is no row of the reference's frame: it does not enter the standard deviation
    assert objectives.keep_samples(np.array([0, 0, 4, 8], np.int32), [0, 4], sample_filter_stdev=3.0).tolist() == [1, 1, 1, 1]
    assert objectives.keep_samples(np.array([0, 0, 4, 9], np.int32), [0, 4], sample_filter_stdev=2.5).tolist() == [1, 1, 1, 0]
    # one sample per cohort: NaN, nobody goes; the cohorts are filtered apart
    assert objectives.keep_samples(np.array([500, 3, 4, 30], np.int32), [0, 1, 4], sample_filter_stdev=1.0).tolist() == [1, 1, 1, 0]


def test_empty_file_and_missing_sample_labels(tmp_path):
    from digdriver_amd.data_tools import objectives
    (tmp_path / "empty.txt").write_text("")
    enc = objectives.encode_objective_rows(str(tmp_path / "empty.txt"), {"1": 1})
    assert len(enc["chrom"]) == 0 and enc["n_uid"] == 0 and enc["sample_names"] == []
    f = _write(tmp_path / "na.txt", [("1", 5, 6, "A", "C", "NA", ".", "Noncoding"), ("1", 5, 6, "A", "C", "S1", ".", "Noncoding")])
    enc = objectives.encode_objective_rows(f, {"1": 1})
    assert enc["sample_names"] == ["S1"] and len(enc["chrom"]) == 1


@pytest.mark.parametrize("path, suffix, want", [
    ("/data/muts/Liver-HCC_SNV_MNV_INDEL.ICGC.annot.txt", "", "Liver-HCC_SNV_MNV_INDEL.ICGC"),
    ("Breast.txt.gz", "_v2", "Breast_v2"),
    ("rel/dir/Skin.bed", "", "Skin"),
    ("Kidney.annot.bed.txt", "", "Kidney"),
    ("plain", ".x", "plain.x"),
    ("a.bedfile.annotated.txt", "", "a"),
])
def test_dataset_name_rule(path, suffix, want):
    from digdriver_amd.data_tools import objectives
    assert objectives.objective_name(path, suffix) == want


def test_entry_points_are_exported_and_refuse_a_key_that_does_not_fit():
    from digdriver_amd import _lib
    lib = _lib.load()
    for sym in ("dig_window_pair_keys", "dig_window_sample_hits", "dig_window_objectives"):
        assert hasattr(lib, sym) and hasattr(lib, sym + "_host") and sym in _lib.EXPORTED_SYMBOLS
    # 30 + 30 + 1 + 30 bits: refused on the host, before any device work
    big = 1 << 30
    with pytest.raises(_lib.DigHipError, match="does not fit 63 bits"):
        _lib.call("dig_window_sample_hits_host", None, 0, big, big, big, None, 0)
    with pytest.raises(_lib.DigHipError, match="does not fit 63 bits"):
        _lib.call("dig_window_pair_keys_host", None, None, 0, None, 0, None, None, None, 0, big, big, big, None, 0)
    keys = np.array([5, 3], np.int64)
    hits = np.zeros(4, np.int32)
    with pytest.raises(_lib.DigHipError, match="keys ascending"):
        _lib.call("dig_window_sample_hits_host", _lib.host_ptr(keys), 2, 4, 10, 10, _lib.host_ptr(hits), 0)
    off = np.array([0, 3], np.int64)
    with pytest.raises(_lib.DigHipError, match="sample_off"):
        _lib.call("dig_window_objectives_host", None, 0, _lib.host_ptr(np.ones(4, np.uint8)), _lib.host_ptr(off), 4, 10, 1, 10,
                  _lib.host_ptr(np.zeros(10)), 0)


def test_existing_name_is_refused_before_any_device_work(tmp_path, monkeypatch):
    from digdriver_amd import engine
    from digdriver_amd.data_tools import objectives
    from digdriver_amd.io import mapfile

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(engine, "window_objectives", no_device)
    f = _write(tmp_path / "Cohort.annot.txt", _rows("single"))
    for data in (str(tmp_path / "train.map"), str(tmp_path / "train.h5")):
        mapfile.write_array(data, "idx", IDX.astype(np.int32))
        mapfile.write_array(data, "Cohort_x", np.zeros(len(IDX)))
        with pytest.raises(ValueError, match="name already exists"):
            objectives.add_objectives(data, f, suffix="_x")
        with pytest.raises(ValueError, match="two mutation files"):
            objectives.add_objectives(data, [f, str(tmp_path / "other" / "Cohort.txt")])


def test_command_line_takes_the_references_arguments_and_refuses_cnv(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import DataExtractor as cli
    finally:
        sys.path.pop(0)
    a = cli.parse_args(["addObjectives", "d.h5", "m1.txt", "m2.txt", "--max-muts-per-sample", "7", "--sample-filter-stdev", "2.5",
                        "--max-muts-per-elt-per-sample", "3", "--suffix", "_s"])
    assert (a.h5_file, a.mut_file, a.max_muts_per_sample, a.sample_filter_stdev, a.max_muts_per_elt_per_sample, a.suffix, a.cnv) == \
        ("d.h5", ["m1.txt", "m2.txt"], 7, 2.5, 3, "_s", False)
    b = cli.parse_args(["addObjectives", "d.h5", "m.txt"])
    assert (b.mut_file, b.max_muts_per_sample, b.sample_filter_stdev, b.max_muts_per_elt_per_sample, b.suffix) == (["m.txt"], None, None, None, "")
    with pytest.raises(SystemExit, match="not built"):
        cli.add_objectives(cli.parse_args(["addObjectives", "d.h5", "m.txt", "--cnv"]))
    with pytest.raises(SystemExit):
        cli.parse_args(["addTracks", "d.h5"])


def test_too_many_pairs_is_refused_in_window_objectives_own_words(monkeypatch):
    """engine.window_objectives hands the join its limit (pair indices are 32-bit) and its refusal; no device work in front of it."""
    from digdriver_amd import engine
    seen = {}

    def join(be, *tables, max_pairs=None, too_many=None):
        seen.update(max_pairs=max_pairs, rows=len(tables[3]))
        raise ValueError(too_many % (max_pairs + 1))
    monkeypatch.setattr(engine, "overlap_join", join)
    z = np.zeros(3, np.int64)
    with pytest.raises(ValueError) as exc:
        engine.window_objectives([1, 1], [0, 100], [100, 200], z + 1, z, z + 1, z, z, z, [0, 1], 1)
    assert str(exc.value) == "2147483648 (mutation, window) pairs: the join's pair indices are 32-bit; fewer cohorts per call"
    assert seen == dict(max_pairs=2 ** 31 - 1, rows=3)
