"""elementDriver --f-sites for many cohorts without a GPU: the encoders of data_tools/sites.py and the plain statement against the golden
made with the reference's own code per cohort (tests/golden/make_sites_cohorts_golden.py), cohort_batch.run_sites_cohorts against the
golden frames and, frame for frame, against transfer_tools.run_sites_region_model per cohort, and the refusals that come before any
device work.

run_sites_cohorts runs on host arrays here (device=None: the library's `_host` twins).  Where no card is visible the plain statement
(sites_statement.py) stands in for its one counting call and scipy (oracle/dig_oracle.py) for the Gamma parameters and the mid-p
values, in the serial and the batched route alike -- file parsing, encoding, the scale factors, the frames and their dtypes are the
product's either way; the kernels themselves run in test_gpu_sites_cohorts.py."""
import numpy as np
import pandas as pd
import pytest

import sites_cohort_cases as K
import sites_statement as S
from conftest import rel_close
from digdriver_amd import _lib
from digdriver_amd.data_tools import mutation_tools, sites
from digdriver_amd.driver_model import cohort_batch
from digdriver_amd.driver_model import transfer_tools as tt
from digdriver_amd.io import mapfile

FX = K.FX


@pytest.fixture
def stand_ins(monkeypatch):
    K.stand_in_without_a_card(monkeypatch)


def test_golden_holds_the_cases_it_is_for():
    rows = [r.split("\t") for r in FX["sites"].splitlines()]
    sp = FX["special"]
    assert 35 <= len(rows) <= 45 and sorted({r[5] for r in rows}) == ["", "A", "B", "C", "D", "E", "X"]
    differs = lambda i, j: [q for q in range(10) if rows[i][q] != rows[j][q]]
    assert differs(sp["shared"], sp["shared"] + 1) == [5] and differs(sp["twice"], sp["twice"] + 1) == []
    assert differs(sp["alt"], sp["alt"] + 1) == [4] and differs(sp["end"], sp["end"] + 1) == [2]
    assert differs(sp["gene"], sp["gene"] + 1) == [6]
    assert rows[sp["nan"]][9] == "nan" and rows[sp["unnamed"]][5] == "" and rows[sp["sex"]][0] == "X"
    assert FX["models"]["full"]["index"] == list("ABCDEZ") and FX["models"]["hit"]["index"] == list("ABCDE")
    hits = [r.split("\t") for r in FX["cohorts"]["hits"].splitlines()]
    assert any(r[7] == "INDEL" for r in hits) and any(r[0] == "X" for r in hits) and any(r[9] == "" for r in hits)
    assert len(hits) != len({tuple(r) for r in hits})                                  # duplicate rows
    assert K.golden_table("none") == {} and set(K.golden_table("all")) == set("ABCDE") and "X" in K.golden_table("hits")
    kinds = {(f["cohort"], f["model"]): f["dtypes"]["OBS_SNV"] for f in FX["frames"]}
    assert kinds[("all", "hit")] == "int64" and kinds[("hits", "hit")] == "int64" and kinds[("all", "full")] == "float64"


def test_encoders_and_statement_give_the_references_count_tables(tmp_path):
    f_sites, f_muts = K.write_files(tmp_path)
    args, names, rows = K.encoded(f_sites, f_muts)
    assert names == list("ABCDEX")                                                     # (the unnamed row is dropped, X's site rows stay)
    site_pos = args[0]
    assert (np.diff(site_pos) >= 0).all() and len(site_pos) == len(FX["sites"].splitlines()) - 2      # less the unnamed row and the one on X
    counts = S.site_counts(*args)
    for c, name in enumerate(K.COHORTS):
        assert K.count_table(counts, names, c) == K.golden_table(name), name
        serial = mutation_tools.tabulate_sites_in_element(f_sites, f_muts[c])
        assert {n: (int(a), int(b)) for n, a, b in zip(serial.index, serial.OBS_SAMPLES, serial.OBS_SNV)} == K.golden_table(name)


def test_encode_site_rows_keeps_the_serial_routes_rows(tmp_path):
    f_sites, f_muts = K.write_files(tmp_path)
    table = sites.encode_sites_file(f_sites)
    for c, f in enumerate(f_muts):
        enc = sites.encode_site_rows(f, table["dicts"], c)
        frame = mutation_tools.read_mutation_file(f, drop_duplicates=False)
        assert enc["n_syn"] == len(frame[(frame.GENE != 'TP53') & (frame.ANNOT == 'Synonymous')])
        kept = frame[frame.ANNOT != 'INDEL']
        assert len(enc["pos"]) == len(kept) and (enc["cohort"] == c).all() and enc["attr"].dtype == np.int64
        assert enc["pos"].tolist() == ((kept.CHROM.values.astype(np.int64) << 40) | kept.START.values).tolist()
        assert [enc["sample_names"][s] for s in enc["sample"]] == kept.SAMPLE.tolist()
        # a row has a code exactly when each of its six labels is a label of the sites file (missing = missing)
        sites_frame = mutation_tools.read_mutation_file(f_sites)
        sites_frame = sites_frame[sites_frame.SAMPLE.notna()]
        known = np.ones(len(kept), bool)
        for col in sites.LABEL_COLS:
            held = set(sites_frame[col].dropna())
            known &= np.array([(v in held) if isinstance(v, str) else sites_frame[col].isna().any() for v in kept[col]])
        assert ((enc["attr"] >= 0) == known).all()
    hits = sites.encode_site_rows(f_muts[0], table["dicts"], 0)
    assert (hits["attr"] < 0).any() and (hits["attr"] >= 0).any()
    assert len(set(table["site_attr"].tolist())) < len(table["site_attr"])             # the doubled and the shared rows share a code


def test_a_row_that_could_match_without_a_sample_is_refused(tmp_path):
    f_sites, _ = K.write_files(tmp_path, [])
    table = sites.encode_sites_file(f_sites)
    site = FX["sites"].splitlines()[0].split("\t")
    other = ["1", "5", "6", "A", "C", "", "GQ", "Noncoding", "A>C", "AAC"]               # cannot match: left out
    f_ok, f_bad = tmp_path / "ok.txt", tmp_path / "bad.txt"
    f_ok.write_text("\t".join(site[:5] + ["S0"] + site[6:]) + "\n" + "\t".join(other) + "\n")
    assert len(sites.encode_site_rows(str(f_ok), table["dicts"])["pos"]) == 1
    f_bad.write_text("\t".join(site[:5] + ["S0"] + site[6:]) + "\n" + "\t".join(site[:5] + [""] + site[6:]) + "\n")
    with pytest.raises(ValueError, match="SAMPLE"):
        sites.encode_site_rows(str(f_bad), table["dicts"])
    maps = K.write_maps(tmp_path, "full", 1)
    with pytest.raises(ValueError, match="SAMPLE"):
        cohort_batch.run_sites_cohorts([str(f_bad)], f_sites, maps, K.KEY, scale_factors=[1.0], scale_by_expectation=False, device=None)


@pytest.mark.parametrize("which", ["full", "hit"])
def test_route_gives_the_references_frames(tmp_path, stand_ins, which):
    f_sites, f_muts = K.write_files(tmp_path)
    maps = K.write_maps(tmp_path, which, len(f_muts), same_rates=True)
    frames = cohort_batch.run_sites_cohorts(f_muts, f_sites, maps, K.KEY, scale_factors=[FX["scale"][n] for n in K.COHORTS],
                                            scale_by_expectation=False, device=None)
    for name, frame in zip(K.COHORTS, frames):
        want = K.golden_frame(name, which)
        assert list(frame.index) == want["index"] and frame.index.name == "ELT"
        assert list(frame.columns)[:len(want["order"])] == want["order"]
        for col in ("R_OBS", "OBS_SNV", "OBS_SAMPLES"):                                # counts: exact
            assert [float(v) for v in frame[col]] == want["columns"][col], (name, col)
        if name != "none":                                                             # (the reference's empty table: object columns)
            assert {c: str(frame[c].dtype) for c in frame.columns} == want["dtypes"], name
        for col in want["order"]:
            if col not in ("R_OBS", "OBS_SNV", "OBS_SAMPLES"):                         # the project's 1e-6 relative contract
                rel_close(frame[col].values, want["columns"][col], rtol=1e-6)
    assert K.golden_frame("none", which)["pvalues_failed"] and "PVAL_SAMPLE_BURDEN" in frames[1].columns


@pytest.mark.parametrize("mode", ["expectation", "factors"])
@pytest.mark.parametrize("which", ["full", "hit"])
def test_route_equals_the_serial_route_frame_for_frame(tmp_path, stand_ins, which, mode):
    f_sites, f_muts = K.write_files(tmp_path)
    f_muts = f_muts + [f_muts[0]]                                                      # a cohort twice, against another map
    maps = K.write_maps(tmp_path, which, len(f_muts))
    factors = [0.7, 1.3, 0.05, 2.0]
    kw = dict(scale_by_expectation=True) if mode == "expectation" else dict(scale_factors=factors, scale_by_expectation=False)
    seen = []
    frames = cohort_batch.run_sites_cohorts(f_muts, f_sites, maps, K.KEY, device=None, on_frame=lambda c, f: seen.append(c), **kw)
    assert seen == list(range(len(f_muts)))
    for c, frame in enumerate(frames):
        serial = tt.run_sites_region_model(f_muts[c], f_sites, maps[c], K.KEY, scale_factor=None if mode == "expectation" else factors[c],
                                           scale_by_expectation=mode == "expectation")
        pd.testing.assert_frame_equal(frame, serial, check_exact=True)


def _no_launch(monkeypatch):
    def refuse(name, *args):
        raise AssertionError("library call %s before the refusal" % name)
    monkeypatch.setattr(_lib, "call", refuse)


@pytest.mark.parametrize("kw", [dict(scale_type="MSK_230"), dict(scale_type="genome"), dict(), dict(scale_factors=[1.0, 0.0, 1.0])])
def test_unbatched_scale_rules_are_refused_before_any_device_work(tmp_path, monkeypatch, kw):
    f_sites, f_muts = K.write_files(tmp_path)
    maps = K.write_maps(tmp_path, "full", len(f_muts))
    _no_launch(monkeypatch)
    with pytest.raises(NotImplementedError, match="run_sites_region_model"):
        cohort_batch.run_sites_cohorts(f_muts, f_sites, maps, K.KEY, scale_by_expectation=False, **kw)


def test_maps_with_different_element_indices_are_refused_before_any_launch(tmp_path, monkeypatch):
    f_sites, f_muts = K.write_files(tmp_path)
    maps = K.write_maps(tmp_path, "full", len(f_muts))
    mapfile.write_frame(maps[2], K.KEY, K.element_frame("hit", 2))
    _no_launch(monkeypatch)
    with pytest.raises(ValueError, match="full2.map"):
        cohort_batch.run_sites_cohorts(f_muts, f_sites, maps, K.KEY)


def test_entry_points_are_bound_and_check_the_key_width():
    lib = _lib.load()
    for sym in ("dig_site_match_count", "dig_site_match_count_host", "dig_site_match_keys", "dig_site_match_keys_host",
                "dig_site_counts", "dig_site_counts_host"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert lib.dig_abi_version() == 12
    E, n_samples = (1 << 31) - 1, (1 << 31) - 1                                        # 31 bits of sample; C E: 32 bits for C = 2, 33 for C = 3
    rc = lib.dig_site_counts_host(None, 0, E, 3, n_samples, None, None, 0)
    assert rc < 0 and "63 bits" in _lib.last_error() and "dig_site_counts_host" in _lib.last_error()
    rc = lib.dig_site_match_keys(None, None, None, None, 0, E, None, None, None, None, None, None, 0, 3, n_samples, None, 0, None, None)
    assert rc < 0 and "63 bits" in _lib.last_error() and "dig_site_match_keys" in _lib.last_error()
    assert lib.dig_site_match_keys(None, None, None, None, 0, E, None, None, None, None, None, None, 0, 2, n_samples, None, 0, None,
                                   None) == 0                                            # 63 bits: fits; nothing to launch
    assert lib.dig_site_match_count(None, None, None, None, 0, E, None, None, None, None, None, None, 0, 0, n_samples, None, None) < 0
    assert "C >= 1" in _lib.last_error()
    assert lib.dig_site_match_count(None, None, None, None, -1, 4, None, None, None, None, None, None, 0, 1, 4, None, None) < 0
