"""targetDriver and countMutations for many cohorts: the panel-count kernels against the plain-Python statement
(tests/panel_counts_statement.py) at the shapes where they can go wrong, through the host twins and on device tensors; the frames of
cohort_batch.run_target_cohorts against transfer_tools.run_target_model, compared exactly; count_cohort_mutations against
DigPretrain.py's count_training_mutations; and the command lines end to end."""
import importlib.util
import os
import types

import numpy as np
import pandas as pd
import pytest

import gene_cohort_cases as K
import target_cohort_cases as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script(name):
    spec = importlib.util.spec_from_file_location("_cli_" + name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    return torch.device("cuda:0")


# ---- the kernels against the statement ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("hand")
    out = T.kernel_cases()
    out["hand_file"] = T.encode([T.file_tuples(T.hand_file(tmp))], T.HAND_PANELS)
    return out


CASE_NAMES = ["hand_file", "lanes600", "lanes577", "long_run", "seventy_labels", "one_panel", "panel_31", "one_label", "empty_cohorts",
              "blacklist_between"]


def _run(args, on_device, dev):
    from digdriver_amd import engine
    from digdriver_amd.data_tools import cohort_rows
    rows = cohort_rows.place([args[k] for k in ("label", "sample", "annot", "cohort")], on_device, dev)
    got = engine.panel_counts(*rows, args["sample_offsets"], args["label_mask"], args["P"], skip=args["skip"])
    return {k: (v.cpu().numpy() if on_device else v) for k, v in got.items()}


@pytest.mark.parametrize("name", CASE_NAMES)
def test_panel_counts_equal_the_statement_on_host_arrays_and_on_the_device(name, cases, dev):
    args, want = cases[name]
    host, device = _run(args, False, dev), _run(args, True, dev)
    for k in ("n_mut", "n_pairs", "n_sample", "n_cds"):
        assert host[k].dtype == np.int64 and host[k].shape == want[k].shape
        assert np.array_equal(host[k], want[k]), (k, host[k], want[k])
        assert np.array_equal(device[k], host[k]), k


def test_the_cases_hold_what_they_are_there_for(cases):
    assert cases["hand_file"][1]["n_sample"].tolist() == [[3, 2]]
    a, w = cases["lanes600"]
    assert len(a["label"]) == 600 and len(cases["lanes577"][0]["label"]) == 577 and a["skip"].sum() == 1
    assert sorted(set(a["cohort"][:10].tolist())) == [0] and a["cohort"][10] == 1 and (w["n_sample"] > 1).all()
    a, w = cases["long_run"]
    assert w["n_mut"][0, 0] >= 700 and w["n_pairs"][0, 0] < 10
    a, w = cases["seventy_labels"]
    assert w["n_pairs"].sum() == 70 + 1 + 2 and w["n_sample"].tolist() == [[2, 2]]       # (L00 is in both panels)
    a, w = cases["panel_31"]
    assert a["P"] == 32 and int(a["label_mask"].max()) >> 31 == 1 and (a["label_mask"] == 1 << 31).sum() == 1
    assert w["n_mut"][0, 31] == 5 and w["n_mut"][0, 30] == 1 and w["n_sample"][0, 31] == 3 and w["n_mut"][1, 31] == 1 and w["n_mut"][1, 0] == 0
    assert len(cases["one_label"][0]["label_mask"]) == 1
    a, w = cases["empty_cohorts"]
    assert w["n_mut"][1].sum() == 0 and w["n_cds"].tolist() == [1, 2, 0, 2] and np.diff(a["sample_offsets"]).tolist() == [1, 2, 0, 1]
    a, w = cases["blacklist_between"]
    assert a["skip"].tolist() == [0, 1, 0] and w["n_sample"].tolist() == [[2, 2]]


def test_no_rows_leave_zeros(dev):
    from digdriver_amd import engine
    import torch
    none_i, none_b = np.zeros(0, np.int32), np.zeros(0, np.uint8)
    for got in (engine.panel_counts(none_i, none_i, none_b, none_i, [0, 2, 5], [1, 3], 2),
                engine.panel_counts(*(torch.as_tensor(x, device=dev) for x in (none_i, none_i, none_b, none_i)), [0, 2, 5], [1, 3], 2)):
        assert all(int(torch.as_tensor(v).sum()) == 0 for v in got.values())
        assert tuple(got["n_mut"].shape) == (2, 2) and tuple(got["n_cds"].shape) == (2,)


def test_device_rows_outside_the_tables_are_refused(dev, cases):
    import torch
    from digdriver_amd import engine
    args, _ = cases["one_panel"]
    for k, v in (("label", 3), ("annot", 7), ("sample", 2), ("cohort", 1)):
        rows = {n: torch.as_tensor(args[n].copy(), device=dev) for n in ("label", "sample", "annot", "cohort")}
        rows[k][1] = v
        with pytest.raises(ValueError, match="outside the tables"):
            engine.panel_counts(rows["label"], rows["sample"], rows["annot"], rows["cohort"], args["sample_offsets"], args["label_mask"], 1)


# ---- the route against the serial route ----------------------------------------------------------------------------------------
MODES = {
    "default": dict(),
    "keep_synonymous_capped": dict(drop_synonymous=False, max_muts_per_gene_per_sample=2),
    "cgc_genes": dict(cgc_genes="CGC_ALL"),
    "by_sample_msk_230": dict(panel="MSK_230", scale_by_sample=True),
    "manual": dict(),                                           # (with factors: one of them 0, which both routes take as "not given")
}
FACTORS = [0.37, 0.0, 1.5]


@pytest.fixture(scope="module")
def route(tmp_path_factory):
    from digdriver_amd.driver_model import transfer_tools as tt
    tmp = tmp_path_factory.mktemp("target")
    case = K.small_case(tmp)
    maps = T.write_target_maps(tmp, 3)
    before = list(tt._PANEL_DIRS)
    tt._PANEL_DIRS[:] = [T.write_panel_dir(tmp)]
    yield dict(files=case["files"], maps=maps, tmp=tmp, panel_dir=tt._PANEL_DIRS[0])
    tt._PANEL_DIRS[:] = before


def _serial(route, mode):
    from digdriver_amd.driver_model import transfer_tools as tt
    return [tt.run_target_model(f, m, max_muts_per_sample=T.HYPER_LIMIT, **MODES[mode],
                                **(dict(scale_factor=FACTORS[c]) if mode == "manual" else {}))
            for c, (f, m) in enumerate(zip(route["files"], route["maps"]))]


def test_the_cohorts_hold_what_they_are_there_for(route):
    from digdriver_amd.data_tools import mutation_tools
    from digdriver_amd.driver_model import transfer_tools as tt
    tested = T.ROUTE_PANELS["MSK_341"]
    lists = []
    for f in route["files"]:
        rows = tt.read_mutations_cds(f)
        rows = rows.loc[rows.GENE.isin(tested) & (rows.ANNOT != 'Synonymous')]
        lists.append(mutation_tools.filter_hypermut_samples(rows, T.HYPER_LIMIT, return_blacklist=True)[1])
        if f.endswith("cohort2.tsv"):
            assert not (rows.ANNOT == 'INDEL').any()
    assert lists == [[], ["S1_8"], []]


@pytest.mark.parametrize("mode", list(MODES))
def test_frames_equal_the_serial_route(mode, route, dev):
    from digdriver_amd.driver_model import cohort_batch
    want = _serial(route, mode)
    got = cohort_batch.run_target_cohorts(route["files"], route["maps"], max_muts_per_sample=T.HYPER_LIMIT, **MODES[mode],
                                          **(dict(scale_factors=FACTORS) if mode == "manual" else {}))
    assert len(got) == 3
    for g, w in zip(got, want):
        pd.testing.assert_frame_equal(g, w, check_exact=True)
        assert list(g.columns) == list(w.columns) and (g.dtypes == w.dtypes).all()


def test_written_files_are_those_of_the_serial_frames(route, dev):
    from digdriver_amd.driver_model import cohort_batch
    from digdriver_amd.io import mapfile
    out = route["tmp"] / "written"
    frames, paths = cohort_batch.run_and_write_target_cohorts(route["files"], route["maps"], str(out), ["a", "b", "c"],
                                                              max_muts_per_sample=T.HYPER_LIMIT)
    assert [os.path.basename(p) for p in paths] == ["a.results.txt", "b.results.txt", "c.results.txt"]
    for path, frame in zip(paths, _serial(route, "default")):
        ref = str(out / "serial.txt")
        mapfile.write_results_tsv(frame, ref)
        assert open(path, "rb").read() == open(ref, "rb").read()


def test_command_lines_run_end_to_end(route, dev):
    from digdriver_amd.driver_model import cohort_batch
    from digdriver_amd.io import mapfile
    drv = _script("DigDriver")
    out = route["tmp"] / "cli"
    lists = "--mutation-files {} --maps {} --outdir {} --outpfx a b c --panel-dir {} --max-muts-per-sample {}".format(
        " ".join(route["files"]), " ".join(route["maps"]), out, route["panel_dir"], T.HYPER_LIMIT)
    drv.main("targetCohorts " + lists + " --panel MSK_341")
    want = cohort_batch.run_target_cohorts(route["files"], route["maps"], max_muts_per_sample=T.HYPER_LIMIT, drop_synonymous=False)
    for pfx, frame in zip("abc", want):
        mapfile.write_results_tsv(frame, str(out / "want.txt"))
        assert open(out / (pfx + ".results.txt"), "rb").read() == open(out / "want.txt", "rb").read()
        os.remove(out / (pfx + ".results.txt"))
    drv.main("geneCohorts " + lists)
    want = cohort_batch.run_gene_cohorts(route["files"], route["maps"], max_muts_per_sample=T.HYPER_LIMIT)
    for pfx, frame in zip("abc", want):
        mapfile.write_results_tsv(frame, str(out / "want.txt"))
        assert open(out / (pfx + ".results.txt"), "rb").read() == open(out / "want.txt", "rb").read()


# ---- countMutations ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [0, None], ids=["device", "host_twins"])
def test_count_cohort_mutations_writes_the_attributes_of_the_serial_function(device, route, tmp_path, dev):
    from digdriver_amd.driver_model import cohort_batch
    from digdriver_amd.io import mapfile
    pre = _script("DigPretrain")
    files = [T.hand_file(tmp_path)] + route["files"]
    (tmp_path / "serial").mkdir()
    (tmp_path / "batch").mkdir()
    serial = T.write_target_maps(tmp_path / "serial", 4, attrs=False, regions=True)
    batch = T.write_target_maps(tmp_path / "batch", 4, attrs=False, regions=True)
    for f, m in zip(files, serial):
        pre.count_training_mutations(types.SimpleNamespace(outputFile=m, fmut=f))
    got = cohort_batch.count_cohort_mutations(files, batch, write=True, device=device)
    for c in range(4):
        want = mapfile.read_attrs(serial[c])
        assert got[c] == want and mapfile.read_attrs(batch[c]) == want
        assert all(type(v) is int for v in got[c].values())
        assert want["N_MUT_SAMPLE_CDS"] == want["N_MUT_CDS"] > 0 and "N_SAMPLE_MSK_230" in want and "N_MUT_MSK_341" in want
        assert "N_MUT_MSK_410" not in want and "N_MUT_ucla_1202" not in want             # panels without their files are skipped


def test_count_cohort_mutations_without_any_panel_file(tmp_path, monkeypatch, dev):
    from digdriver_amd.driver_model import cohort_batch, transfer_tools as tt
    from digdriver_amd.io import mapfile
    pre = _script("DigPretrain")
    (tmp_path / "none").mkdir()
    monkeypatch.setattr(tt, "_PANEL_DIRS", [str(tmp_path / "none")])
    maps = T.write_target_maps(tmp_path, 2, attrs=False, regions=True)
    f = T.hand_file(tmp_path)
    pre.count_training_mutations(types.SimpleNamespace(outputFile=maps[0], fmut=f))
    got = cohort_batch.count_cohort_mutations([f], [maps[1]], write=False)
    want = mapfile.read_attrs(maps[0])
    assert {k: v for k, v in got[0].items() if not k.startswith("N_MUT_T")} == {k: v for k, v in want.items() if not k.startswith("N_MUT_T")}
    assert got[0]["N_MUT_CDS"] == 8 and mapfile.read_attrs(maps[1]) == {}
