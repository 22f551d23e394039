"""The target route for many cohorts, the parts that need no card: the encoder, the plain-Python statement of the panel counts
against the serial routes' pandas expressions, the binding and the refusals in front of any launch, and the command lines.
(The host twins stage through a card: their comparison with the statement is in test_gpu_target_cohorts.py.)"""
import importlib.util
import os
import types

import numpy as np
import pandas as pd
import pytest

import gene_cohort_cases as K
import panel_counts_statement as S
import target_cohort_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script(name):
    spec = importlib.util.spec_from_file_location("_cli_" + name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_encode_panel_rows_gives_the_rows_of_read_mutation_file(tmp_path):
    from digdriver_amd.data_tools import mutation_tools, tabulate_gpu
    f = T.hand_file(tmp_path)
    labels = ["PA", "PB", "BOTH", "PC"]
    enc = tabulate_gpu.encode_panel_rows(f, labels, cohort_id=4)
    rows = mutation_tools.read_mutation_file(f, drop_duplicates=True)
    assert len(rows) == 10                                      # 13 lines: the repeated row, the second sample's indel and X are gone
    assert [(labels + ["-"])[i] for i in enc["label"]] == [g if g in labels else "-" for g in rows.GENE]
    assert [enc["sample_names"][i] for i in enc["sample"]] == rows.SAMPLE.tolist()
    assert enc["sample_names"] == ["S1", "S3", "S4", "S5"]      # S2's only row was the repeated indel
    names = {v: k for k, v in T.CLASSES.items()}
    assert [names.get(int(a), "other") for a in enc["annot"]] == [a if a in T.CLASSES else "other" for a in rows.ANNOT]
    assert 6 in enc["annot"] and 5 in enc["annot"]              # Noncoding apart from any other label
    assert enc["label"].dtype == np.int32 and enc["sample"].dtype == np.int32 and enc["annot"].dtype == np.uint8
    assert (enc["cohort"] == 4).all() and enc["cohort"].dtype == np.int32


def test_a_file_without_gene_columns_is_refused(tmp_path):
    from digdriver_amd.data_tools import tabulate_gpu
    f = K.write_rows(tmp_path / "bare.tsv", [("1", 10, 11, "A", "C", "S1"), ("2", 20, 21, "A", "C", "S2")])
    with pytest.raises(ValueError, match="bare.tsv"):
        tabulate_gpu.encode_panel_rows(f, ["PA"])


def test_statement_counts_the_hand_file_as_written_down(tmp_path):
    got = S.cohort_panel_counts(T.file_tuples(T.hand_file(tmp_path)), T.HAND_PANELS)
    assert got == T.HAND_COUNTS
    # S3 blacklisted: its Stop_loss row and its Synonymous row leave
    got = S.cohort_panel_counts(T.file_tuples(T.hand_file(tmp_path)), T.HAND_PANELS, ["S3"])
    assert got["n_cds"] == 6 and got["panels"]["MSK_341"] == dict(n_mut=3, n_pairs=3, n_sample=2)


def _files(tmp_path):
    return [T.hand_file(tmp_path)] + K.small_case(tmp_path)["files"]


def test_statement_gives_the_counts_of_panel_scale(tmp_path, monkeypatch):
    from digdriver_amd.driver_model import transfer_tools as tt
    panels = dict(T.ROUTE_PANELS, **T.HAND_PANELS)
    monkeypatch.setattr(tt, "_PANEL_DIRS", [T.write_panel_dir(tmp_path, panels)])
    maps = T.write_target_maps(tmp_path, 1)
    for f in _files(tmp_path):
        tuples = T.file_tuples(f)
        samples = sorted(set(s for _, s, _ in tuples))
        for black in ((), samples[:1], samples[1:3]):
            st = S.cohort_panel_counts(tuples, panels, black)
            for panel in ("MSK_341", "MSK_230"):
                run = tt.CohortRun(f, maps[0])
                assert run.panel_scale(panel, tt.gene_panel(panel), list(black), False) == st["panels"][panel]["n_mut"] / run.attrs["N_MUT_" + panel]
                assert run.panel_scale(panel, tt.gene_panel(panel), list(black), True) == st["panels"][panel]["n_sample"] / run.attrs["N_SAMPLE_" + panel]


def test_statement_gives_the_attributes_of_count_training_mutations(tmp_path, monkeypatch):
    from digdriver_amd.driver_model import transfer_tools as tt
    from digdriver_amd.io import mapfile
    pre = _script("DigPretrain")
    panels = {k: v for k, v in dict(T.ROUTE_PANELS, **T.HAND_PANELS).items() if k.startswith("MSK")}
    monkeypatch.setattr(tt, "_PANEL_DIRS", [T.write_panel_dir(tmp_path, panels)])
    files = _files(tmp_path)
    maps = T.write_target_maps(tmp_path, len(files), attrs=False, regions=True)
    for f, m in zip(files, maps):
        pre.count_training_mutations(types.SimpleNamespace(outputFile=m, fmut=f))
        attrs = mapfile.read_attrs(m)
        st = S.cohort_panel_counts(T.file_tuples(f), panels)
        assert attrs["N_SAMPLES"] == st["n_samples"] and attrs["N_MUT_CDS"] == st["n_cds"] == attrs["N_MUT_SAMPLE_CDS"]
        for name in panels:
            assert attrs["N_MUT_" + name] == st["panels"][name]["n_mut"]
            assert attrs["N_MUT_SAMPLE_" + name] == st["panels"][name]["n_pairs"]
        assert attrs["N_SAMPLE_MSK_230"] == st["panels"]["MSK_230"]["n_sample"]
        assert "N_MUT_MSK_410" not in attrs                     # (no such panel file here)


def test_entry_points_are_bound_and_check_the_key_width():
    from digdriver_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dig_hip.h")).read()
    for sym in ("dig_panel_row_keys", "dig_panel_row_keys_host", "dig_panel_counts", "dig_panel_counts_host"):
        assert sym in _lib.EXPORTED_SYMBOLS and getattr(lib, sym) is not None
        assert "int %s(" % sym in header
    assert lib.dig_abi_version() == 12 and "#define DIG_ABI_VERSION 12" in header
    h = _lib.host_ptr
    off = np.array([0, 1 << 40], np.int64)
    buf, mask = np.zeros(8, np.int64), np.zeros(8, np.uint32)
    # 30 bits of label + 40 bits of sample
    rc = lib.dig_panel_row_keys_host(h(buf), h(buf), h(buf), h(buf), h(off), None, h(mask), 0, 1 << 30, 1, 1, 1 << 40, h(buf), h(buf), 0)
    assert rc < 0 and "63 bits" in _lib.last_error() and "dig_panel_row_keys_host" in _lib.last_error()
    rc = lib.dig_panel_counts_host(h(buf), 0, h(mask), h(off), 1 << 30, 1, 1, 1 << 40, h(buf), h(buf), h(buf), 0)
    assert rc < 0 and "63 bits" in _lib.last_error() and "dig_panel_counts_host" in _lib.last_error()
    rc = lib.dig_panel_row_keys(h(buf), h(buf), h(buf), h(buf), h(off), None, h(mask), 0, 1 << 30, 1, 1, 1 << 40, h(buf), h(buf), None)
    assert rc < 0 and "63 bits" in _lib.last_error() and "dig_panel_row_keys" in _lib.last_error()
    rc = lib.dig_panel_row_keys_host(h(buf), h(buf), h(buf), h(buf), h(off), None, h(mask), 0, 4, 33, 1, 4, h(buf), h(buf), 0)
    assert rc < 0 and "P within [1, 32]" in _lib.last_error()


@pytest.mark.parametrize("bad", ["label", "annot", "sample", "cohort"])
def test_a_row_outside_the_tables_is_refused_by_the_host_twin(bad):
    from digdriver_amd import _lib
    lib = _lib.load()
    h = _lib.host_ptr
    row = dict(label=np.array([1, 2], np.int32), sample=np.array([0, 2], np.int32), annot=np.array([1, 6], np.uint8),
               cohort=np.array([0, 0], np.int32))
    row[bad] = row[bad].copy()
    row[bad][1] = dict(label=3, annot=7, sample=3, cohort=1)[bad]       # L = 2, three samples, one cohort
    off, mask = np.array([0, 3], np.int64), np.array([1, 1], np.uint32)
    keys, n_cds = np.zeros(2, np.int64), np.zeros(1, np.int64)
    rc = lib.dig_panel_row_keys_host(h(row["label"]), h(row["sample"]), h(row["annot"]), h(row["cohort"]), h(off), None, h(mask), 2, 2, 1, 1,
                                     3, h(keys), h(n_cds), 0)
    assert rc < 0 and "dig_panel_row_keys_host" in _lib.last_error() and "within" in _lib.last_error()


def _no_launch(monkeypatch):
    from digdriver_amd import _lib

    def refuse(name, *args):
        raise AssertionError("a library call (%s) in front of the refusal" % name)
    monkeypatch.setattr(_lib, "call", refuse)


def test_a_map_without_the_attribute_is_named_before_any_device_work(tmp_path, monkeypatch):
    from digdriver_amd.driver_model import cohort_batch, transfer_tools as tt
    from digdriver_amd.io import mapfile
    monkeypatch.setattr(tt, "_PANEL_DIRS", [T.write_panel_dir(tmp_path)])
    maps = T.write_target_maps(tmp_path, 2)
    bare = K.write_maps(tmp_path / "panels", 1)[0]                      # a map without attributes
    _no_launch(monkeypatch)
    with pytest.raises(KeyError, match="genes0.map.*N_MUT_MSK_341"):
        cohort_batch.run_target_cohorts(["a.tsv", "b.tsv"], [maps[0], bare])
    with pytest.raises(KeyError, match="N_SAMPLE_MSK_230"):
        cohort_batch.run_target_cohorts(["a.tsv", "b.tsv"], [bare, maps[1]], panel="MSK_230", scale_by_sample=True)
    with pytest.raises(ValueError, match="one map per cohort"):
        cohort_batch.run_target_cohorts(["a.tsv", "b.tsv"], [maps[0]])


def test_maps_with_different_gene_indices_are_refused_before_any_launch(tmp_path, monkeypatch):
    from digdriver_amd.driver_model import cohort_batch, transfer_tools as tt
    from digdriver_amd.io import mapfile
    monkeypatch.setattr(tt, "_PANEL_DIRS", [T.write_panel_dir(tmp_path)])
    maps = T.write_target_maps(tmp_path, 3)
    other = K.model_frame(2)
    other.loc[3, "GENE"] = "G99"
    mapfile.write_frame(maps[2], "genic_model", other)
    _no_launch(monkeypatch)
    with pytest.raises(ValueError, match="genes2.map"):
        cohort_batch.run_target_cohorts(["a.tsv", "b.tsv", "c.tsv"], maps)


def test_command_lines_take_the_new_sub_commands():
    drv, pre = _script("DigDriver"), _script("DigPretrain")
    a = drv.parse_args("targetCohorts --mutation-files a.tsv b.tsv --maps a.map b.map --outdir out --outpfx a b --panel MSK_341 "
                       "--scale-factor-manual 0.5 0.25 --max-muts-per-sample 100 --cgc-genes CGC_ALL --scale-by-samples --panel-dir p")
    assert a.func is drv.cmd_target_cohorts and a.mutation_files == ["a.tsv", "b.tsv"] and a.maps == ["a.map", "b.map"]
    assert a.outpfx == ["a", "b"] and a.scale_factor_manual == [0.5, 0.25] and a.panel == "MSK_341" and a.scale_by_samples
    assert a.max_muts_per_sample == 100 and a.cgc_genes == "CGC_ALL" and a.panel_dir == "p"
    g = drv.parse_args("geneCohorts --mutation-files a.tsv --maps a.map --outdir out --outpfx a --selection --no-pval-sel "
                       "--max-muts-per-gene-per-sample 3")
    assert g.func is drv.cmd_gene_cohorts and g.selection and not g.pval_sel and g.pval_burden and g.scale_by_expectation
    assert g.max_muts_per_gene_per_sample == 3 and g.scale_factor_manual is None
    c = pre.parse_args("countMutationsCohorts --mutation-files a.tsv b.tsv --maps a.map b.map")
    assert c.func is pre.count_training_mutations_cohorts and c.fmuts == ["a.tsv", "b.tsv"] and c.maps == ["a.map", "b.map"]


@pytest.mark.parametrize("text", [
    "targetCohorts --mutation-files a.tsv b.tsv --maps a.map --outdir out --outpfx a b --panel MSK_341",
    "targetCohorts --mutation-files a.tsv b.tsv --maps a.map b.map --outdir out --outpfx a --panel MSK_341",
    "targetCohorts --mutation-files a.tsv b.tsv --maps a.map b.map --outdir out --outpfx a b --panel MSK_341 --scale-factor-manual 0.5",
    "geneCohorts --mutation-files a.tsv b.tsv --maps a.map --outdir out --outpfx a b",
    "geneCohorts --mutation-files a.tsv --maps a.map --outdir out --outpfx a --scale-by-samples",
    "geneCohorts --mutation-files a.tsv --maps a.map --outdir out --outpfx a --scale-by-mutations",
])
def test_driver_command_lines_refuse_what_does_not_fit(text, monkeypatch):
    drv = _script("DigDriver")
    _no_launch(monkeypatch)
    with pytest.raises(SystemExit) as exc:
        drv.main(text)
    assert "ERROR" in str(exc.value)


def test_count_command_line_refuses_unequal_lists(monkeypatch):
    pre = _script("DigPretrain")
    _no_launch(monkeypatch)
    with pytest.raises(SystemExit) as exc:
        pre.count_training_mutations_cohorts(pre.parse_args("countMutationsCohorts --mutation-files a.tsv b.tsv --maps a.map"))
    assert "one map per mutation file" in str(exc.value)
