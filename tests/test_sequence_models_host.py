"""DigPretrain sequenceModels without a GPU: sequence_tools.train_sequence_models and the command line against the golden made with
the reference's own train_sequence_model per cohort (tests/golden/make_sequence_models_golden.py), for K = 192 and K = 3 072, against
train_sequence_model called per cohort, and the refusals that come before any device work.

The route runs on numpy arrays (on_device=False).  Its counting step, engine.sequence_counts, goes through the library's `_host`
twins and so needs a card: where none is visible the plain statement (sequence_counts_statement.py) stands in for that one call --
file parsing, row encoding, the serial route, S_genome, the frames and the command line are the product's either way; the kernel
itself runs in test_gpu_sequence_models.py."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import sequence_counts_statement as S
from conftest import GOLDEN, ROOT
from digdriver_amd import _lib, engine
from digdriver_amd.data_tools import mutation_tools
from digdriver_amd.io import mapfile
from digdriver_amd.sequence_model import sequence_tools as st

FX = json.load(open(os.path.join(GOLDEN, "sequence_models_golden.json")))
IDX = np.array(FX["idx"], np.int64)
MAPP = np.array(FX["mappability"])
TRI = ["none", "long", "big"]


def has_card():
    try:
        return _lib.device_count() > 0
    except _lib.DigHipError:
        return False                                                    # (the library has not been built)


def statement_counts(wc, ws, we, rc, rs, re, rt, rk, K, C, device=0):
    return S.sequence_counts(wc, ws, we, rc, rs, re, rt, rk, K, C)


@pytest.fixture
def counting(monkeypatch):
    if not has_card():
        monkeypatch.setattr(engine, "sequence_counts", statement_counts)


def cohort_text(name):
    if name == "penta":
        with gzip.open(os.path.join(GOLDEN, "penta_context_golden.json.gz"), "rt") as f:
            return json.load(f)["annotated"]
    return FX["cohorts"][name]


def write_cohorts(tmp_path, names):
    files = []
    for name in names:
        (tmp_path / (name + ".annot.txt")).write_text(cohort_text(name))
        files.append(str(tmp_path / (name + ".annot.txt")))
    return files


def genome_counts(n_up):
    return S.genome_frame(len(IDX), list(st.mk_context_sequences(n_up, n_up).keys()))


def golden_model(name):
    return [m for m in FX["models"] if m["cohort"] == name][0]


def test_golden_holds_the_cases_it_is_for():
    keep = MAPP > FX["map_thresh"]
    assert 150 <= len(IDX) <= 250 and sorted(set(IDX[:, 0])) == [1, 2, 3]
    assert (MAPP == FX["map_thresh"]).sum() >= 3 and 10 < (~keep).sum() < keep.sum()
    rows = [tuple(w) for w in IDX[keep]]
    assert rows.count((3, 4000, 4100)) == 2 and (3, 4200, 4320) in rows and (3, 4280, 4400) in rows
    for c, gap in ((1, True), (2, False)):
        w = IDX[IDX[:, 0] == c]
        assert ((w[1:, 1] > w[:-1, 2]).all() if gap else (w[1:, 1] == w[:-1, 2]).all())
    big = [r.split("\t") for r in FX["cohorts"]["big"].splitlines()]
    assert 1800 <= len(big) <= 2300
    assert {"X", "Y", "9"} <= {r[0] for r in big}
    assert {r[0] for r in FX["cohorts"]["none"].splitlines() for r in [r.split("\t")]} == {"X", "Y", "9"}
    seen, first_indel, later_differs = {}, 0, 0
    for r in big:
        key = tuple(r[:6])
        if key in seen:
            first_indel += seen[key][7] == "INDEL" and r[7] != "INDEL"
            later_differs += seen[key][7] != "INDEL" and (r[7:] != seen[key][7:])
        seen.setdefault(key, r)
    assert first_indel >= 10 and later_differs >= 50
    table = set(zip(*[st.mk_mutation_context(1, 1, return_df=True)[c] for c in ("MUT_TYPE", "CONTEXT")]))
    assert sum((r[8], r[9]) not in table and r[7] != "INDEL" for r in big) >= 40
    inside = lambda r, w: r[0] == str(w[0]) and w[1] <= int(r[1]) < w[2]
    assert sum(inside(r, (3, 4000, 4100)) for r in big) >= 60 and sum(inside(r, (3, 4280, 4320)) for r in big) >= 60
    long = [r.split("\t") for r in FX["cohorts"]["long"].splitlines()]
    assert sum(int(r[2]) - int(r[1]) != 1 and r[7] != "INDEL" for r in long) >= 5
    assert golden_model("none")["rows_read"] > 0 and sum(golden_model("none")["COUNT"]) == 0
    # the doubled and the overlapping windows add nothing: fewer rows counted than read
    assert 0 < sum(golden_model("big")["COUNT"]) < golden_model("big")["rows_read"]


@pytest.mark.parametrize("n_up, names", [(1, TRI), (2, ["penta"]), (2, ["penta", "penta"])])
def test_route_gives_the_references_tables(tmp_path, counting, n_up, names):
    files = write_cohorts(tmp_path, sorted(set(names)))
    files = [files[sorted(set(names)).index(n)] for n in names]
    frame = genome_counts(n_up)
    models, counts, serial = st.train_sequence_models(files, IDX, MAPP, frame, map_thresh=FX["map_thresh"], n_up=n_up, n_down=n_up,
                                                      on_device=False)
    K = 3 * 4 ** (2 * n_up + 1)
    assert counts.shape == (len(names), K) and counts.dtype == np.int64
    assert serial == ([1] if n_up == 1 else [])
    S_genome = frame[MAPP > FX["map_thresh"]].sum(axis=0)
    assert [int(v) for v in S_genome.values] == FX["S_genome"][str(n_up)]
    for c, name in enumerate(names):
        want = golden_model(name)
        f_mut, f_ctx = models[c]
        assert len(f_mut) == K and len(f_ctx) == K // 3
        assert counts[c].tolist() == want["COUNT"]
        assert np.array_equal(f_mut.COUNT.to_numpy(float), np.array(want["COUNT"], float))
        assert list(f_mut.columns) == want["columns"]
        if want["MUT_TYPE"]:
            assert list(f_mut.MUT_TYPE) == want["MUT_TYPE"] and list(f_mut.CONTEXT) == want["CONTEXT"]
        # the tolerances test_penta_context_host.py applies to the same two tables
        np.testing.assert_allclose(f_mut.FREQ.to_numpy(float), np.array(want["FREQ"]), rtol=1e-15, atol=0)
        assert [str(i) for i in f_ctx.index] == want["context_index"]
        np.testing.assert_allclose(f_ctx.FREQ.to_numpy(float), np.array(want["context_FREQ"]), rtol=1e-12, atol=0)
        # ... and the serial command's own steps (scripts/DigPretrain.py pretrain_sequence_model) give the same frames
        df_mut = mutation_tools.read_mutation_file(files[c], drop_duplicates=True)
        df_mut = df_mut[df_mut.ANNOT != 'INDEL']
        one_mut, one_ctx = st.train_sequence_model(IDX[MAPP > FX["map_thresh"]], df_mut, S_genome, n_up=n_up, n_down=n_up)
        pd.testing.assert_frame_equal(f_mut, one_mut)
        pd.testing.assert_frame_equal(f_ctx, one_ctx)


def test_encoded_rows(tmp_path):
    f = write_cohorts(tmp_path, ["big"])[0]
    chrom_ids = {"1": 1, "2": 2, "3": 3}
    enc = st.encode_sequence_rows(f, chrom_ids)
    assert enc["one_base"] and enc["frame"] is None                     # (the indels of `big` are longer; they are dropped first)
    assert enc["chrom"].dtype == enc["start"].dtype == enc["end"].dtype == np.int64 and enc["type"].dtype == np.int32
    df = mutation_tools.read_mutation_file(f, drop_duplicates=True)
    df = df[(df.ANNOT != 'INDEL') & df.CHROM.isin([1, 2, 3])]
    assert len(df) == len(enc["chrom"]) == golden_model("big")["rows_read"] - 30        # the rows on chromosome 9
    assert enc["chrom"].tolist() == df.CHROM.tolist() and enc["start"].tolist() == df.START.tolist()
    table = st.mk_mutation_context(1, 1, return_df=True)
    pos = {(m, c): i for i, (m, c) in enumerate(zip(table.MUT_TYPE, table.CONTEXT))}
    assert enc["type"].tolist() == [pos.get((m, c), 192) for m, c in zip(df.MUT_TYPE, df.CONTEXT)]
    assert (enc["type"] == 192).sum() >= 40
    long = st.encode_sequence_rows(write_cohorts(tmp_path, ["long"])[0], chrom_ids)
    assert not long["one_base"] and len(long["frame"]) == golden_model("long")["rows_read"]
    # a chromosome the windows do not hold is left out, whatever its id
    assert len(st.encode_sequence_rows(f, {"2": 7})["chrom"]) == int((df.CHROM == 2).sum())
    assert set(st.encode_sequence_rows(f, {"2": 7})["chrom"].tolist()) == {7}


_DRIVER = """
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
sys.path.insert(0, {scripts!r})
import DigPretrain
if {stub}:
    import sequence_counts_statement as S
    from digdriver_amd import engine
    engine.sequence_counts = lambda wc, ws, we, rc, rs, re, rt, rk, K, C, device=0: S.sequence_counts(wc, ws, we, rc, rs, re, rt, rk, K, C)
DigPretrain.main({text!r})
assert "torch" not in sys.modules
print("no torch")
"""


@pytest.mark.parametrize("n_up", [1, 2])
def test_command_line_writes_the_routes_frames_without_torch(tmp_path, counting, n_up):
    names = TRI if n_up == 1 else ["penta"]
    files = write_cohorts(tmp_path, names)
    frame = genome_counts(n_up)
    gc = str(tmp_path / "genome_counts.map")
    mapfile.write_array(gc, "idx", IDX.astype(np.int32))
    mapfile.write_array(gc, "mappability", MAPP.astype(np.float64))
    mapfile.write_frame(gc, "all_window_genome_counts", frame)
    maps = [str(tmp_path / (n + ".map")) for n in names]
    text = "sequenceModels {} --mutation-files {} --maps {} --map-thresh {}".format(gc, " ".join(files), " ".join(maps), FX["map_thresh"])
    if n_up == 2:
        text += " --up 2 --down 2"
    script = _DRIVER.format(root=ROOT, tests=os.path.join(ROOT, "tests"), scripts=os.path.join(ROOT, "scripts"), stub=not has_card(),
                            text=text)
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, DIG_CLI_ASSERT_NO_TORCH="1"))
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().endswith("no torch")
    if n_up == 1:
        assert files[1] + ": rows longer or shorter than one base" in r.stdout
    models, _, _ = st.train_sequence_models(files, IDX, MAPP, frame, map_thresh=FX["map_thresh"], n_up=n_up, n_down=n_up, on_device=False)
    K = 3 * 4 ** (2 * n_up + 1)
    for (f_mut, f_ctx), f_map in zip(models, maps):
        pd.testing.assert_frame_equal(mapfile.read_frame(f_map, "sequence_model_%d" % K), f_mut)
        pd.testing.assert_frame_equal(mapfile.read_frame(f_map, "sequence_model_%d" % (K // 3)), f_ctx)


def _cli():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import DigPretrain
    finally:
        sys.path.pop(0)
    return DigPretrain


def test_command_line_arguments_and_unequal_lists(tmp_path):
    cli = _cli()
    a = cli.parse_args("sequenceModels gc.h5 --mutation-files a.txt b.txt --maps a.h5 b.h5")
    assert (a.genome_counts, a.fmuts, a.maps, a.map_thresh, a.up, a.down) == ("gc.h5", ["a.txt", "b.txt"], ["a.h5", "b.h5"], 0.5, 1, 1)
    b = cli.parse_args("sequenceModel m.txt gc.h5 out.h5")                  # the one-cohort command as it was
    assert (b.fmut, b.genome_counts, b.output_h5, b.map_thresh) == ("m.txt", "gc.h5", "out.h5", 0.5) and b.func is cli.pretrain_sequence_model
    # nothing of this exists: a refusal after the first read would be a FileNotFoundError
    missing = str(tmp_path / "nowhere")
    with pytest.raises(SystemExit, match="one map per mutation file"):
        cli.main("sequenceModels {0}/gc.h5 --mutation-files {0}/a.txt {0}/b.txt --maps {0}/a.h5".format(missing))
    assert not os.path.exists(missing)


def test_entry_point_is_exported_and_refuses_before_any_device_work():
    lib = _lib.load()
    for sym in ("dig_sequence_counts", "dig_sequence_counts_host"):
        assert hasattr(lib, sym) and sym in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 12
    pair = np.zeros(2, np.int32)
    typ, coh = np.array([0, 5], np.int32), np.array([0, 1], np.int32)
    out = np.zeros((2, 4), np.int64)
    p = _lib.host_ptr

    def twin(pair, typ, coh, K, C):
        _lib.call("dig_sequence_counts_host", p(pair), len(pair), p(typ), p(coh), len(typ), K, C, p(out), 0)
    with pytest.raises(_lib.DigHipError, match=r"K within \[1, 3072\]"):
        twin(pair, typ, coh, 0, 2)
    with pytest.raises(_lib.DigHipError, match=r"K within \[1, 3072\]"):
        twin(pair, typ, coh, 3073, 2)
    with pytest.raises(_lib.DigHipError, match=r"C within"):
        twin(pair, typ, coh, 4, 0)
    with pytest.raises(_lib.DigHipError, match=r"cohort within \[0, C\)"):
        twin(pair, typ, coh, 5, 1)
    with pytest.raises(_lib.DigHipError, match=r"type within \[0, K\]"):
        twin(pair, typ, coh, 4, 2)
    with pytest.raises(_lib.DigHipError, match="a pair within the rows"):
        twin(np.array([0, 2], np.int32), typ, coh, 5, 2)
    # the device entry point checks its scalars in front of the first HIP call
    with pytest.raises(_lib.DigHipError, match=r"K within \[1, 3072\]"):
        _lib.call("dig_sequence_counts", None, 0, None, None, 0, 0, 1, None, None)
    with pytest.raises(_lib.DigHipError, match=r"C within"):
        _lib.call("dig_sequence_counts", None, 0, None, None, 0, 4, 0, None, None)
    # the engine turns the library's refusal into a ValueError (no rows: the join has nothing to launch)
    z = np.zeros(0, np.int64)
    with pytest.raises(ValueError, match=r"K within \[1, 3072\]"):
        engine.sequence_counts([1], [0], [10], z, z, z, z, z, 0, 1)


def test_too_many_pairs_is_refused_in_sequence_counts_own_words(monkeypatch):
    seen = {}

    def join(be, *tables, max_pairs=None, too_many=None):
        seen.update(max_pairs=max_pairs, rows=len(tables[3]))
        raise ValueError(too_many % (max_pairs + 1))
    monkeypatch.setattr(engine, "overlap_join", join)
    z = np.zeros(3, np.int64)
    with pytest.raises(ValueError) as exc:
        engine.sequence_counts([1, 1], [0, 100], [100, 200], z + 1, z, z + 1, z, z, 192, 1)
    assert str(exc.value) == "2147483648 (row, window) pairs: the join's pair indices are 32-bit; fewer cohorts per call"
    assert seen == dict(max_pairs=2 ** 31 - 1, rows=3)
    with pytest.raises(ValueError, match="windows: chromosome ids"):
        engine.sequence_counts([1 << 22], [0], [100], z + 1, z, z + 1, z, z, 192, 1)
