"""The counts by sample of the per-base route, the parts that need no GPU: the plain-Python statement's hand-worked cases, the reader
of the sample column, `keep` from --max-muts-per-sample, the refusals of the `_host` twins before any device work, the bindings,
and the command line."""
import ctypes
import importlib.util
import os

import numpy as np
import pandas as pd
import pytest

from conftest import ROOT
import tile_samples_cases as K
import tile_samples_statement as S
from digdriver_amd import _lib
from digdriver_amd.sequence_model import nb_model


@pytest.mark.parametrize("name", sorted(S.HAND_CASES))
def test_statement_hand_cases(name):
    regions, rows, C, binsize, n_tiles, keep, cap, k_cap, k_samples = S.HAND_CASES[name]
    assert S.tile_sample_counts(regions, rows, C, binsize, n_tiles, keep, cap) == (k_cap, k_samples)
    # the thinned rows, counted without cap and filter, give k_cap: what ties the statement to the row-counting route
    stay = S.thinned_rows(regions, rows, C, binsize, n_tiles, keep, cap)
    assert S.tile_sample_counts(regions, [rows[i] for i in stay], C, binsize, n_tiles)[0] == k_cap


def test_statement_keep_drops_only_samples_above_the_limit():
    assert S.keep_from_max_muts([0, 0, 0, 1, 1, 3], 4, 2) == [0, 1, 1, 1]
    assert S.keep_from_max_muts([0, 0, 0, 1, 1, 3], 4, 3) == [1, 1, 1, 1]
    assert S.keep_from_max_muts([0, 0, 0], 2, None) == [1, 1]
    assert list(nb_model.sample_keep([3, 2, 0, 1], 2)) == [0, 1, 1, 1] and list(nb_model.sample_keep([3, 2], None)) == [1, 1]


ROWS = [("1", 10, 11, "a"), ("2", 20, 25, "b"), ("1", 30, 31, "a"), ("1", 31, 32, "NA"), ("2", 5, 6, "7")]


@pytest.mark.parametrize("extra", [0, 1, 2, 3])
@pytest.mark.parametrize("gz,chr_prefix", [(False, False), (True, True)])
def test_reader_takes_column_six_of_six_to_nine_column_files(tmp_path, extra, gz, chr_prefix):
    path = K.write_file(tmp_path / ("m.bed.gz" if gz else "m.bed"), ROWS, chr_prefix=chr_prefix, gz=gz, extra_columns=extra)
    got = nb_model._mutation_rows(path, samples=True)
    assert list(got.columns) == ["CHROM", "START", "END", "ID"]
    assert list(got.CHROM) == ["1", "2", "1", "1", "2"] and list(got.START) == [10, 20, 30, 31, 5] and list(got.END) == [11, 25, 31, 32, 6]
    assert list(got.ID) == ["a", "b", "a", "NA", "7"]                    # labels are strings; "NA" is a name, not a missing value
    plain = nb_model._mutation_rows(path)                                # without a sample option: the three columns of before
    assert list(plain.columns) == ["CHROM", "START", "END"] and plain.equals(got[["CHROM", "START", "END"]])


def test_reader_refuses_files_without_labels(tmp_path):
    short = tmp_path / "short.bed"
    short.write_text("1\t10\t11\tA\tC\n1\t20\t21\tA\tC\n")
    with pytest.raises(ValueError, match="column 6"):
        nb_model._mutation_rows(str(short), samples=True)
    assert len(nb_model._mutation_rows(str(short))) == 2                 # the route without samples reads it as before
    empty = tmp_path / "empty.bed"
    empty.write_text("1\t10\t11\tA\tC\ts\n1\t20\t21\tA\tC\t\n9\t5\t6\tA\tC\t\n")
    with pytest.raises(ValueError, match="1 rows without a sample label in column 6"):
        nb_model._cohort_rows([str(empty)], {"1"}, True)                 # (the row on the unknown chromosome 9 is not counted)
    ok = nb_model._cohort_rows([str(empty)], {"9"}, False)
    assert list(ok[0]["start"]) == [5] and "sample" not in ok[0]
    with pytest.raises(ValueError, match="column ID"):
        nb_model._cohort_rows([pd.DataFrame({"CHROM": ["1"], "START": [1], "END": [2]})], {"1"}, True)


def test_equal_labels_in_two_cohorts_are_different_samples_and_keep_is_per_cohort():
    a = pd.DataFrame({"CHROM": ["1"] * 5 + ["9"], "START": range(6), "END": range(1, 7), "ID": ["x", "y", "x", "x", "z", "y"]})
    b = pd.DataFrame({"CHROM": ["chr1"] * 3, "START": range(3), "END": range(1, 4), "ID": ["x", "x", "w"]})
    rows = nb_model._cohort_rows([a, b], {"1"}, True, max_muts_per_sample=2)
    args = nb_model._sample_arguments(rows, 3, True)
    assert rows[0]["sample_names"] == ["x", "y", "z"] and rows[1]["sample_names"] == ["w", "x"]
    assert list(args["sample_offsets"]) == [0, 3, 5] and args["cap"] == 3 and args["by_sample"] is True
    assert list(args["mut_sample"]) == [0, 1, 0, 0, 2, 4, 4, 3] and args["mut_sample"].dtype == np.int32
    # x of cohort 0 has 3 rows (> 2) and goes; x of cohort 1 has 2 and stays; the row on chromosome 9 was not counted for y
    assert list(args["keep"]) == [0, 1, 1, 1, 1] and args["keep"].dtype == np.uint8
    stacked = [int(s) for s in args["mut_sample"]]
    assert list(args["keep"]) == S.keep_from_max_muts(stacked, 5, 2)


def test_option_domains():
    assert nb_model._check_sample_options(None, None, False) is False
    assert nb_model._check_sample_options(0, None, False) and nb_model._check_sample_options(None, 1, False)
    assert nb_model._check_sample_options(None, None, True, "PVAL_SAMPLE")
    for bad in (dict(max_muts_per_tile_per_sample=0), dict(max_muts_per_tile_per_sample=1.5), dict(max_muts_per_sample=-1),
                dict(cut_on="QVAL"), dict(cut_on="PVAL_SAMPLE")):
        kw = dict(max_muts_per_sample=None, max_muts_per_tile_per_sample=None, by_sample=False, cut_on="PVAL")
        kw.update(bad)
        with pytest.raises(ValueError):
            nb_model._check_sample_options(**kw)
    # refused before a genome is packed or a device is touched
    with pytest.raises(ValueError, match="PVAL_SAMPLE requires by_sample"):
        nb_model.nb_model_hits([{}], np.zeros((0, 3)), [[]], [[]], ["no such file"], "no such fasta", n_up=1, n_down=1, pval_max=0.1,
                               cut_on="PVAL_SAMPLE")


def test_sharded_tiles_refuses_the_sample_keywords():
    from digdriver_amd import parallel
    for kw in (dict(mut_sample=np.zeros(1, np.int32)), dict(sample_offsets=[0, 1]), dict(keep=[1]), dict(cap=2), dict(by_sample=True)):
        with pytest.raises(NotImplementedError, match="one device"):
            parallel.ShardedTiles(None, [], [], [], None, None, None, [], [], [], [], 50, 0, 0, 1, **kw)


# ---- the library: bindings and refusals, no device -----------------------------------------------------------------------------
def test_bindings_mirror_the_header():
    header = open(os.path.join(ROOT, "include", "dig_hip.h")).read()
    for name in ("dig_tile_sample_keys", "dig_tile_sample_counts"):
        assert name + "(" in header and name + "_host(" in header
        assert _lib._SIGNATURES[name][-1] is ctypes.c_void_p and _lib._SIGNATURES[name + "_host"][-1] is ctypes.c_int
        assert _lib._SIGNATURES[name + "_host"][:-1] == _lib._SIGNATURES[name][:-1]
        assert name in _lib.EXPORTED_SYMBOLS and name + "_host" in _lib.EXPORTED_SYMBOLS
    assert len(_lib._SIGNATURES["dig_tile_sample_keys"]) == 17 and len(_lib._SIGNATURES["dig_tile_sample_counts"]) == 10


def _refused(name, args, fragment):
    rc = getattr(_lib.load(), name)(*[_lib.host_ptr(a) if isinstance(a, np.ndarray) else a for a in args])
    msg = _lib.last_error()
    assert rc == -1 and name in msg and "requirement failed" in msg and fragment in msg, (name, rc, msg)


def test_host_twins_refuse_before_any_device_work():
    """DIG_EINVAL in the entry point's name, with no device present: a key whose fields do not fit 63 bits, sizes that reach 2^31,
    pairs and samples outside the tables, keys that are not ascending."""
    buf, i32 = np.zeros(64, np.int64), lambda *v: np.array(v, np.int32)
    keys = lambda over: [buf, buf, 1, buf, 1, buf, buf, None, buf, buf, 50] + over + [buf, 0]        # ..., n_tiles, R, C, n_samples, keys, device
    fit = "does not fit 63 bits"
    _refused("dig_tile_sample_keys_host", keys([1 << 20, 1 << 20, 1 << 20, 1 << 10]), fit)          # 60 + 11 bits
    _refused("dig_tile_sample_keys_host", keys([1 << 20, 1 << 20, 1 << 13, 1 << 11]), fit)          # 53 + 12 (2^11 samples and the all-ones field)
    _refused("dig_tile_sample_keys_host", keys([1 << 31, 1, 1, 1]), "below 2^31")
    _refused("dig_tile_sample_keys_host", keys([8, 1, -1, 1]), "C, R, n_tiles, n_samples >= 0")
    counts = lambda over: [buf, 1] + over + [0, buf, buf, 0]                                         # keys, n, C, R, n_tiles, n_samples, cap, ...
    _refused("dig_tile_sample_counts_host", counts([1 << 20, 1 << 20, 1 << 20, 1 << 10]), fit)
    _refused("dig_tile_sample_counts_host", counts([1, 1, 1, 1 << 31]), "below 2^31")
    _refused("dig_tile_sample_counts_host", [buf, -1, 1, 1, 1, 1, 0, buf, buf, 0], "0 <= n < 2^31")
    _refused("dig_tile_sample_counts_host", [np.array([5, 3], np.int64), 2, 1, 1, 1, 1, 0, buf, buf, 0], "keys ascending")
    # host data outside the tables: pair_mut = 3 of 2 rows; a sample 4 of 4 in a cohort within [0, C); binsize 0
    rows = [np.array([0, 10], np.int64), 2, i32(0, 0), i32(0, 4), None, buf, i32(1), 50, 8, 1, 1, 4, buf, 0]
    _refused("dig_tile_sample_keys_host", [i32(3), i32(0), 1] + rows, "pairs inside the mutation / region tables")
    _refused("dig_tile_sample_keys_host", [i32(1), i32(0), 1] + rows, "global sample within [0, n_samples)")
    rows[7] = 0
    _refused("dig_tile_sample_keys_host", [i32(1), i32(0), 1] + rows, "binsize >= 1")


def test_key_layout_at_its_boundary():
    """2^20 2^20 2^12 tiles take 52 bits.  2^11 - 1 samples take 11 (the field holds the values 0 .. n_samples, so that the all-ones
    key is no real one): 63 bits, accepted; 2^11 samples take 12: refused.  With n_pairs = 0 the twin returns after the layout check
    and before any device call, so the accepting side is seen without a device too."""
    buf = np.zeros(8, np.int64)
    p = _lib.host_ptr(buf)
    lib = _lib.load()
    assert lib.dig_tile_sample_keys_host(p, p, 0, p, 1, p, p, None, p, p, 50, 1 << 12, 1 << 20, 1 << 20, (1 << 11) - 1, p, 0) == 0
    assert lib.dig_tile_sample_keys_host(p, p, 0, p, 1, p, p, None, p, p, 50, 1 << 12, 1 << 20, 1 << 20, 1 << 11, p, 0) == -1
    assert "dig_tile_sample_keys_host" in _lib.last_error() and "63 bits" in _lib.last_error()


# ---- the command line ----------------------------------------------------------------------------------------------------------
def _cli():
    spec = importlib.util.spec_from_file_location("dig_driver_cli_tile_samples", os.path.join(ROOT, "scripts", "DigDriver.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BASE = "tileDriver g.fa --mutation-files a.bed b.bed --maps ma mb --outdir out --outpfx A B --fdr 0.1 "


def test_command_line_parses_the_four_options():
    cli = _cli()
    a = cli.parse_args(BASE)
    assert a.max_muts_per_sample is None and a.max_muts_per_tile_per_sample is None and a.by_sample is False and a.cut_on == "PVAL"
    a = cli.parse_args(BASE + "--max-muts-per-sample 500 --max-muts-per-tile-per-sample 2 --by-sample --cut-on PVAL_SAMPLE")
    assert (a.max_muts_per_sample, a.max_muts_per_tile_per_sample, a.by_sample, a.cut_on) == (500, 2, True, "PVAL_SAMPLE")
    assert a.func is cli.cmd_tile
    with pytest.raises(SystemExit):
        cli.parse_args(BASE + "--cut-on QVAL")
    with pytest.raises(SystemExit):
        cli.parse_args(BASE + "--max-muts-per-tile-per-sample 1.5")


def test_command_line_refusals_come_before_any_file_is_read():
    cli = _cli()
    with pytest.raises(SystemExit, match="--cut-on PVAL_SAMPLE requires --by-sample"):
        cli.main(BASE + "--cut-on PVAL_SAMPLE")
    with pytest.raises(SystemExit, match="--max-muts-per-tile-per-sample takes an integer >= 1"):
        cli.main(BASE + "--max-muts-per-tile-per-sample 0")
    with pytest.raises(SystemExit, match="--max-muts-per-sample takes an integer >= 0"):
        cli.main(BASE + "--max-muts-per-sample -3")
    assert not os.path.exists("out")
