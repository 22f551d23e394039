"""The plumbing the many-cohort routes share, without a device and without the library: engine._scan and
engine._requirements_as_value_errors, data_tools/cohort_rows.py, and cohort_batch._read_models behind the two model readers; and, with
the library's host writer, cohort_batch._check_cut, _write_frames (against the bytes of before: tests/golden/write_frames_golden.json)
and _usable_cores."""
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from digdriver_amd import _lib, _marshal, engine
from digdriver_amd.data_tools import cohort_rows


# ---- the scan of a two-call entry point -------------------------------------------------------------------------------------
@pytest.fixture
def be():
    return _marshal.HostBackend(0)


def test_scan_gives_exclusive_offsets_and_the_total(be):
    offsets, total = engine._scan(be, np.array([0, 3, 0, 2], np.int32))
    assert offsets.dtype == np.int64 and offsets.tolist() == [0, 0, 3, 3]
    assert type(total) is int and total == 5
    offsets, total = engine._scan(be, np.array([7], np.int32))
    assert offsets.dtype == np.int64 and offsets.tolist() == [0] and total == 7


def test_scan_of_no_rows_is_typed_and_empty(be):
    offsets, total = engine._scan(be, np.zeros(0, np.int32))
    assert offsets.dtype == np.int64 and offsets.shape == (0,)
    assert type(total) is int and total == 0


def test_scan_does_not_wrap_above_32_bits(be):
    offsets, total = engine._scan(be, np.array([2 ** 30 + 1, 2 ** 30 + 1], np.int32))
    assert type(total) is int and total == 2 ** 31 + 2 and total > 2 ** 31 - 1
    assert offsets.dtype == np.int64 and offsets.tolist() == [0, 2 ** 30 + 1]


def test_scan_in_groups_gives_where_each_group_starts(be):
    offsets, total, ptr = engine._scan(be, np.array([0, 3, 0, 2, 1, 1], np.int32), groups=3)         # tile_select: C = 3, R = 2
    assert offsets.tolist() == [0, 0, 3, 3, 5, 6] and total == 7 and type(total) is int
    assert ptr.dtype == np.int64 and ptr.tolist() == [0, 3, 5, 7] and ptr.tolist()[:-1] == offsets[::2].tolist()
    for groups in (3, 0):                                                                             # R = 0, C = 0
        offsets, total, ptr = engine._scan(be, np.zeros(0, np.int32), groups=groups)
        assert offsets.dtype == np.int64 and offsets.shape == (0,) and total == 0 and type(total) is int
        assert ptr.dtype == np.int64 and ptr.tolist() == [0] * (groups + 1)


# ---- the error translation --------------------------------------------------------------------------------------------------
def test_a_refused_requirement_leaves_as_value_error():
    refused = _lib.DigHipError("dig_site_counts_host failed (-1): requirement failed: x")
    with pytest.raises(ValueError) as info:
        with engine._requirements_as_value_errors():
            raise refused
    assert type(info.value) is ValueError and str(info.value) == str(refused) and info.value.__cause__ is refused


def test_other_errors_leave_unchanged():
    other = _lib.DigHipError("dig_site_counts failed (-2): hipMalloc failed: out of memory")
    with pytest.raises(_lib.DigHipError) as info:
        with engine._requirements_as_value_errors():
            raise other
    assert info.value is other
    key = KeyError("requirement failed: not the library's")
    with pytest.raises(KeyError) as info:
        with engine._requirements_as_value_errors():
            raise key
    assert info.value is key


# ---- the cohort stack -------------------------------------------------------------------------------------------------------
def _records():
    """Three cohorts with 2, 0 and 3 samples and 4, 0 and 1 rows."""
    return [dict(sample=np.array([0, 1, 1, 0], np.int32), uid=np.array([3, 0, 1, 3], np.int64), pos=np.array([5, 6, 7, 8], np.int64),
                 flag=np.array([1, 0, 0, 1], bool), sample_names=["a", "b"]),
            dict(sample=np.zeros(0, np.int32), uid=np.zeros(0, np.int64), pos=np.zeros(0, np.int64), flag=np.zeros(0, bool),
                 sample_names=[]),
            dict(sample=np.array([2], np.int32), uid=np.array([1], np.int64), pos=np.array([9], np.int64), flag=np.array([0], bool),
                 sample_names=["x", "y", "z"])]


def test_sample_offsets():
    off = cohort_rows.sample_offsets(_records())
    assert off.dtype == np.int64 and off.tolist() == [0, 2, 2, 5]
    none = cohort_rows.sample_offsets([])
    assert none.dtype == np.int64 and none.tolist() == [0]


def test_shifted_sample_column_equals_the_hand_written_stack():
    rows = _records()
    off = cohort_rows.sample_offsets(rows)
    by_hand = np.concatenate([r["sample"] + np.int32(off[c]) for c, r in enumerate(rows)])          # (run_sites_cohorts before)
    got = cohort_rows.column(rows, "sample", shift=off)
    assert got.dtype == by_hand.dtype == np.int32 and np.array_equal(got, by_hand) and got.tolist() == [0, 1, 1, 0, 4]
    by_hand = np.concatenate([np.asarray(r["sample"], np.int32) + np.int32(o) for r, o in zip(rows, off[:-1])])   # (objectives before)
    got = cohort_rows.column(rows, "sample", "i32", off)
    assert got.dtype == np.int32 and np.array_equal(got, by_hand)


@pytest.mark.parametrize("name, dtype", [("i64", np.int64), ("i32", np.int32), ("u8", np.uint8)])
def test_every_concatenation_keeps_the_requested_dtype(name, dtype):
    rows = _records()
    for records, subset, want in ((rows, None, [1, 0, 0, 1, 0]), (rows, [2, 0], [0, 1, 0, 0, 1]), (rows, [1], []), (rows, [], []),
                                  ([], None, []), ([rows[1], rows[1]], None, [])):
        got = cohort_rows.column(records, "flag", name, subset=subset)
        assert got.dtype == dtype and got.ndim == 1 and got.tolist() == want
    assert cohort_rows.column(rows, "pos").dtype == np.int64 and cohort_rows.column(rows, "flag").dtype == bool      # their own


def test_subset_takes_its_cohorts_shift_and_order():
    rows = _records()
    off = cohort_rows.sample_offsets(rows)
    assert cohort_rows.column(rows, "sample", "i32", off, subset=[2]).tolist() == [4]
    assert cohort_rows.column(rows, "sample", "i32", off, subset=[2, 0]).tolist() == [4, 0, 1, 1, 0]
    assert cohort_rows.cohort_column(rows, "sample", [2, 0]).tolist() == [2, 0, 0, 0, 0]


def test_cohort_column():
    got = cohort_rows.cohort_column(_records(), "pos")
    assert got.dtype == np.int32 and got.tolist() == [0, 0, 0, 0, 2]
    none = cohort_rows.cohort_column([], "pos")
    assert none.dtype == np.int32 and none.shape == (0,)


def test_dense_id_offsets_of_an_empty_cohort_add_nothing():
    rows = _records()
    off = cohort_rows.id_offsets(rows, "uid")
    assert off.dtype == np.int64 and off.tolist() == [0, 4, 4, 6]                      # max + 1 = 4, nothing, max + 1 = 2
    assert cohort_rows.column(rows, "uid", shift=off).tolist() == [3, 0, 1, 3, 5]
    assert cohort_rows.id_offsets([rows[1], rows[1]], "uid").tolist() == [0, 0, 0] and cohort_rows.id_offsets([], "uid").tolist() == [0]


def test_place_keeps_host_arrays_on_the_host(monkeypatch):
    a = np.arange(6, dtype=np.int32).reshape(2, 3).T
    monkeypatch.setattr(_lib, "TORCH_FREE", True)                                      # (None: the device unless torch-free)
    for on_device in (False, None):
        got = cohort_rows.place([a, [1, 2]], on_device)
        assert all(isinstance(x, np.ndarray) and x.flags["C_CONTIGUOUS"] for x in got) and np.array_equal(got[0], a)


def test_cohort_rows_does_not_import_torch():
    code = ("import sys, numpy as np\n"
            "from digdriver_amd.data_tools import cohort_rows\n"
            "rows = [dict(sample=np.zeros(2, np.int32), sample_names=['a'])]\n"
            "cohort_rows.column(rows, 'sample', 'i32', cohort_rows.sample_offsets(rows)); cohort_rows.cohort_column(rows, 'sample')\n"
            "cohort_rows.id_offsets(rows, 'sample'); cohort_rows.place([np.zeros(2)], False)\n"
            "assert 'torch' not in sys.modules, 'cohort_rows imported torch'\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=_lib._HERE + "/..")


def test_engine_imports_nothing_from_data_tools():
    code = ("import sys\n"
            "from digdriver_amd import engine\n"
            "assert 'digdriver_amd.data_tools.tabulate_gpu' not in sys.modules, 'engine imported tabulate_gpu'\n"
            "assert not [m for m in sys.modules if m.startswith('digdriver_amd.data_tools')], 'engine imported data_tools'\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=_lib._HERE + "/..")
    src = open(engine.__file__).read()
    assert "data_tools import" not in src and "import data_tools" not in src              # (nor inside a function)


# ---- the model reader -------------------------------------------------------------------------------------------------------
def _gene_frame(mu, genes=("G1", "TP53", "G3")):
    n = len(genes)
    one = np.ones(n)
    return pd.DataFrame(dict(CHROM=["1"] * n, GENE=list(genes), GENE_LENGTH=[900] * n, R_SIZE=[10] * n, R_OBS=[4] * n, R_INDEL=[1] * n,
                             MU=np.asarray(mu, float), SIGMA=np.asarray(mu, float) / 2, MU_INDEL=[8.0] * n, SIGMA_INDEL=[4.0] * n,
                             FLAG=[0] * n, P_MIS=0.5 * one, P_NONS=0.0625 * one, P_SILENT=0.25 * one, P_SPLICE=0.0625 * one,
                             P_TRUNC=0.125 * one, P_INDEL=0.03125 * one))


def _site_frame(mu, elts=("E1", "E2")):
    return pd.DataFrame(dict(ELT=list(elts), R_OBS=[3, 4], MU=np.asarray(mu, float), SIGMA=[1.0, 2.0], P_SUM=[0.5, 0.25],
                             EXTRA=["dropped", "dropped"]))


@pytest.fixture
def in_memory(monkeypatch):
    """maps[path][key] -> frame in place of mapfile.read_frame; mu^2 / sigma^2, sigma^2 / mu in place of the device's Gamma parameters,
    counted."""
    from digdriver_amd.io import mapfile
    from digdriver_amd.sequence_model import nb_model
    maps, calls = {}, []

    def gamma(mu, sigma, device=0):
        calls.append(np.shape(mu))
        return mu ** 2 / sigma ** 2, sigma ** 2 / mu
    monkeypatch.setattr(mapfile, "read_frame", lambda f, key: maps[f][key].copy())
    monkeypatch.setattr(nb_model, "normal_params_to_gamma", gamma)
    monkeypatch.setattr(_lib, "call", lambda name, *a: pytest.fail("a library call: " + name))
    return maps, calls


def test_gene_models_are_stacked_with_one_gamma_call_per_pair(in_memory):
    from digdriver_amd.driver_model import cohort_batch, transfer_tools as tt
    maps, calls = in_memory
    maps.update(a={"genic_model": _gene_frame([4.0, 6.0, 8.0])}, b={"genic_model": _gene_frame([2.0, 10.0, 12.0])})
    frames, planes = cohort_batch._read_gene_models(["a", "b"])
    assert calls == [(3, 2), (3, 2)]                                                   # (MU, SIGMA) and (MU_INDEL, SIGMA_INDEL), over [G, C]
    assert sorted(planes) == sorted(['MU', 'SIGMA', 'MU_INDEL', 'SIGMA_INDEL', 'Pi_INDEL', 'ALPHA', 'THETA', 'ALPHA_INDEL', 'THETA_INDEL']
                                    + ['Pi_' + c for c in tt.GENE_CLASSES])
    assert all(v.dtype == np.float64 and v.shape == (3, 2) and v.flags["C_CONTIGUOUS"] for v in planes.values())
    assert planes['MU'].tolist() == [[4.0, 2.0], [6.0, 10.0], [8.0, 12.0]] and planes['SIGMA'].tolist() == [[2.0, 1.0], [3.0, 5.0], [4.0, 6.0]]
    assert planes['ALPHA'].tolist() == [[4.0, 4.0]] * 3 and planes['THETA'].tolist() == [[1.0, 0.5], [1.5, 2.5], [2.0, 3.0]]
    assert planes['ALPHA_INDEL'].tolist() == [[4.0, 4.0]] * 3 and planes['THETA_INDEL'].tolist() == [[2.0, 2.0]] * 3
    assert planes['Pi_SYN'].tolist() == [[0.25, 0.25]] * 3 and planes['Pi_NONSYN'].tolist() == [[0.625, 0.625]] * 3   # Pi_MIS + Pi_TRUNC
    assert planes['Pi_INDEL'].tolist() == [[0.03125, 0.03125]] * 3
    for c, m in enumerate(frames):
        assert list(m.columns) == list(tt._GENE_COLS_LEFT) and list(m.index) == ["G1", "TP53", "G3"] and m.index.name == "GENE"
        assert m.THETA.tolist() == planes['THETA'][:, c].tolist() and m.ALPHA_INDEL.tolist() == [4.0] * 3
        assert m.Pi_NONSYN.tolist() == [0.625] * 3 and m.Pi_SPL.tolist() == [0.0625] * 3 and m.MU.tolist() == planes['MU'][:, c].tolist()
    # the scale factor both routes take from such a frame: synonymous rows over the expected count outside TP53
    assert cohort_batch._expected_syn_scale(frames[0], 6) == 6 / (4.0 * 0.25 + 8.0 * 0.25)


def test_site_models_are_stacked_with_one_gamma_call(in_memory):
    from digdriver_amd.driver_model import cohort_batch
    maps, calls = in_memory
    maps.update(a={"mysites": _site_frame([2.0, 4.0])}, b={"mysites": _site_frame([3.0, 8.0])})
    frames, planes = cohort_batch._read_site_models(["a", "b"], "mysites")
    assert calls == [(2, 2)] and sorted(planes) == ['ALPHA', 'MU', 'Pi_SUM', 'SIGMA', 'THETA']
    assert all(v.dtype == np.float64 and v.shape == (2, 2) for v in planes.values())
    assert planes['MU'].tolist() == [[2.0, 3.0], [4.0, 8.0]] and planes['Pi_SUM'].tolist() == [[0.5, 0.5], [0.25, 0.25]]
    assert planes['ALPHA'].tolist() == [[4.0, 9.0], [4.0, 16.0]] and planes['THETA'].tolist() == [[0.5, 1 / 3.0], [1.0, 0.5]]
    for c, m in enumerate(frames):
        assert list(m.columns) == cohort_batch._SITE_MODEL_COLS and list(m.index) == ["E1", "E2"] and m.index.name == "ELT"
        assert m.ALPHA.tolist() == planes['ALPHA'][:, c].tolist() and m.THETA.tolist() == planes['THETA'][:, c].tolist()
        assert m.R_OBS.tolist() == [3, 4] and m.Pi_SUM.tolist() == [0.5, 0.25]


def test_a_differing_index_gets_the_routes_own_message(in_memory):
    from digdriver_amd.driver_model import cohort_batch
    maps, calls = in_memory
    maps.update(a={"genic_model": _gene_frame([4.0, 6.0, 8.0]), "mysites": _site_frame([2.0, 4.0])},
                b={"genic_model": _gene_frame([4.0, 6.0, 8.0]), "mysites": _site_frame([2.0, 4.0])},
                c={"genic_model": _gene_frame([4.0, 6.0, 8.0], ("G1", "TP53", "G9")), "mysites": _site_frame([2.0, 4.0], ("E1", "E9"))})
    with pytest.raises(ValueError) as info:
        cohort_batch._read_gene_models(["a", "b", "c"])
    assert str(info.value) == ("c: its gene model's gene index differs from that of a (run_gene_cohorts needs one gene index for all "
                               "maps)")
    with pytest.raises(ValueError) as info:
        cohort_batch._read_site_models(["a", "b", "c"], "mysites")
    assert str(info.value) == ("c: the element index of its 'mysites' model differs from that of a (run_sites_cohorts needs one element "
                               "index for all maps)")
    assert calls == []                                                                 # refused in front of the element-wise call


# ---- the cut's arguments, the writer of finished frames, the cores ------------------------------------------------------------
def test_the_cut_is_checked_and_its_column_numbered():
    from digdriver_amd.driver_model import cohort_batch
    columns = ["PVAL_SNV_BURDEN", "PVAL_SAMPLE_BURDEN", "PVAL_INDEL_BURDEN", "PVAL_MUT_BURDEN"]
    assert [cohort_batch._check_cut(0.5, None, k) for k in columns] == [0, 1, 2, 3]
    assert [cohort_batch._check_cut(None, 0.1, k) for k in columns] == [0, 1, 2, 3]
    for pval_max, fdr in ((None, None), (0.5, 0.1)):
        with pytest.raises(ValueError) as info:
            cohort_batch._check_cut(pval_max, fdr, "PVAL_SNV_BURDEN")
        assert str(info.value) == "exactly one of pval_max and fdr must be given"
    with pytest.raises(ValueError) as info:
        cohort_batch._check_cut(0.5, None, "QVAL_SNV_BURDEN")
    assert str(info.value) == "cut_on: one of " + ", ".join(columns)
    # the column run_element_meta ranks the members by goes with no cut, and is named in its own words
    assert cohort_batch._check_cut(None, None, "PVAL_MUT_BURDEN", "best_on") == 3
    with pytest.raises(ValueError) as info:
        cohort_batch._check_cut(None, None, "MU", "best_on")
    assert str(info.value) == "best_on: one of " + ", ".join(columns)


def _hand_frames():
    """Three small result frames: bools, NaN, the extremes of float printing, an int32 column, OBS_* columns (written as integers),
    another index in the second (the label cache must not serve it), and a quoted element name in the third (pandas writes it)."""
    a = pd.DataFrame({"FLAG": np.array([True, False, False]), "MU": np.array([0.1, np.nan, 1e-300]), "R_OBS": np.array([3, 0, 12], np.int32),
                      "OBS_SAMPLES": np.array([2.0, 0.0, 5.0]), "OBS_SNV": np.array([2.0, 0.0, 7.0]),
                      "PVAL_SNV_BURDEN": np.array([0.25, np.nan, 1.5e-17])}, index=pd.Index(["e1", "e2", "e3"], name="ELT"))
    b = pd.DataFrame({"MU": np.array([1.0 / 3.0, 2.5]), "OBS_INDEL": np.array([1.0, 0.0]), "N_COHORTS": np.array([3, 3], np.int64)},
                     index=pd.Index(["e2", "e9"], name="ELT"))
    c = pd.DataFrame({"MU": np.array([0.5, 1e22]), "OBS_SNV": np.array([4.0, 1.0])}, index=pd.Index(['e"quoted"', "e4"], name="ELT"))
    return [a, b, c]


def test_finished_frames_are_written_with_the_bytes_of_before_at_any_thread_count(tmp_path):
    import json
    import os
    from digdriver_amd.driver_model import cohort_batch
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "write_frames_golden.json")
    want = {k: v.encode("ascii") for k, v in json.load(open(golden)).items()}          # what write_results wrote before _write_frames
    assert sorted(want) == ["a.results.txt", "b.results.txt", "c.results.txt"] and b'"e""quoted"""' in want["c.results.txt"]
    names = ["a", "b", "c"]
    for threads in (1, 4):
        out = tmp_path / ("threads%d" % threads) / "nested"
        paths = cohort_batch._write_frames(_hand_frames(), [str(out / (n + ".results.txt")) for n in names], threads)
        assert [os.path.basename(p) for p in paths] == sorted(want)
        for p in paths:
            assert open(p, "rb").read() == want[os.path.basename(p)], (threads, p)
    for workers in (None, 1, 2):
        paths = cohort_batch.write_results(_hand_frames(), str(tmp_path / ("workers%s" % workers)), names, workers=workers)
        assert [open(p, "rb").read() for p in paths] == [want[n + ".results.txt"] for n in names]
    assert cohort_batch._write_frames([], []) == [] and cohort_batch.write_results([], str(tmp_path / "none"), []) == []


def test_usable_cores_follow_the_affinity_mask():
    import os
    from digdriver_amd.driver_model import cohort_batch
    from digdriver_amd.sequence_model import genic_driver_tools
    n = cohort_batch._usable_cores()
    assert type(n) is int and 1 <= n <= os.cpu_count()
    if hasattr(os, "sched_getaffinity"):
        assert n == len(os.sched_getaffinity(0))
    assert genic_driver_tools._usable_cores is cohort_batch._usable_cores           # (the maps' reader sizes its pool by the same)
    files, per_file = cohort_batch._writer_threads(3)
    assert files == min(3, n) and per_file == max(1, min(8, n // 3)) and cohort_batch._writer_threads(3, 2) == (files, 2)
    assert cohort_batch._writer_threads(0) == (1, min(8, n)) and cohort_batch._writer_threads(10 ** 6) == (n, 1)
