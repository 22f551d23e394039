"""CPU-only checks of geneDriver for many cohorts: the row encoding against the serial route's reader, the plain-Python statement of
the counts (gene_obs_statement.py) against the repo's own pandas functions -- which the existing tests pin to the reference's
goldens -- on the inputs of test_gpu_gene_cohorts.py, the exported symbols, and the refusals that come before any device work."""
import ctypes

import numpy as np
import pandas as pd
import pytest

import gene_cohort_cases as K
import gene_obs_statement as S

# one indel in three samples under one gene label (one row kept); the same indel under two gene labels in one sample (both kept);
# duplicate SNV rows (kept); X and a chr-prefixed label (dropped with the sex chromosomes); a gene outside the model; TP53;
# Stop_loss and labelled Noncoding rows (class 5); rows without a gene label (not coding)
HAND_ROWS = [
    ("1", 100, 101, "A", "C", "S1", "G00", "Missense"),
    ("1", 100, 101, "A", "C", "S1", "G00", "Missense"),
    ("1", 100, 101, "A", "C", "S1", "G00", "Missense"),
    ("2", 500, 503, "ACG", "A", "S1", "G01", "INDEL"),
    ("2", 500, 503, "ACG", "A", "S2", "G01", "INDEL"),
    ("2", 500, 503, "ACG", "A", "S3", "G01", "INDEL"),
    ("4", 700, 703, "TTA", "T", "S2", "G02", "INDEL"),
    ("4", 700, 703, "TTA", "T", "S2", "G03", "INDEL"),
    ("X", 900, 901, "G", "T", "S1", "G00", "Nonsense"),
    ("chr3", 900, 901, "G", "T", "S1", "G00", "Nonsense"),
    ("5", 40, 41, "G", "T", "S3", "OUTSIDE", "Synonymous"),
    ("17", 75, 76, "C", "T", "S2", "TP53", "Synonymous"),
    ("17", 76, 77, "C", "T", "S4", "TP53", "Missense"),
    ("6", 10, 11, "T", "A", "S4", "G02", "Stop_loss"),
    ("6", 12, 13, "T", "A", "S4", "G02", "Noncoding"),
    ("6", 14, 15, "T", "A", "S5", ".", "Noncoding"),
    ("8", 20, 21, "T", "A", "S3", "G03", "Essential_Splice"),
    ("8", 22, 23, "T", "A", "S3", "G03", "Synonymous"),
]


@pytest.mark.parametrize("genes", [["G00", "G01", "G02", "G03", "TP53"], ["G00", "G01", "G02", "G03"]], ids=["tp53_in_model", "tp53_not_in_model"])
def test_encode_gene_rows_gives_the_rows_of_read_mutations_cds(tmp_path, genes):
    from digdriver_amd.data_tools import tabulate_gpu
    from digdriver_amd.driver_model import transfer_tools as tt
    f = K.write_rows(tmp_path / "hand.tsv", HAND_ROWS)
    want = tt.read_mutations_cds(f)
    assert len(want) == 13                                           # 18 rows - X - chr3 - '.' - two of the three-sample indel
    assert (want.ANNOT == "INDEL").sum() == 3 and (want.GENE.isin(["G02", "G03"]) & (want.ANNOT == "INDEL")).sum() == 2
    G = len(genes)
    gene_id = lambda g: genes.index(g) if g in genes else (G + 1 if g == "TP53" else G)
    cls = lambda a: tabulate_gpu.GENE_ROW_CLASSES.get(a, 5)
    enc = tabulate_gpu.encode_gene_rows(f, pd.Index(genes), cohort_id=4)
    assert enc["gene"].dtype == np.int32 and enc["sample"].dtype == np.int32 and enc["annot"].dtype == np.uint8
    assert (enc["cohort"] == 4).all() and enc["cohort"].dtype == np.int32
    got = sorted(zip(enc["gene"].tolist(), [enc["sample_names"][s] for s in enc["sample"]], enc["annot"].tolist()))
    assert got == sorted((gene_id(g), s, cls(a)) for g, s, a in zip(want.GENE, want.SAMPLE, want.ANNOT))
    assert sorted(enc["sample_names"]) == sorted(want.SAMPLE.unique()) and len(set(enc["sample_names"])) == len(enc["sample_names"])
    assert (G + 1 in enc["gene"]) == ("TP53" not in genes) and G in enc["gene"] and 5 in enc["annot"]
    # the encoder's older first_indel flag sits behind drop_duplicate_mutations and would lose one of the two-label rows
    old = tabulate_gpu.encode_mutation_file(f, native=False)
    assert int(old["first_indel"].sum()) == 2
    kept = tabulate_gpu.encode_gene_rows(f, pd.Index(genes), keep={"G00", "TP53"})
    assert len(kept["gene"]) == int(want.GENE.isin(["G00", "TP53"]).sum())


def test_a_file_without_a_coding_row_is_refused(tmp_path):
    from digdriver_amd.data_tools import tabulate_gpu
    f = K.write_rows(tmp_path / "noncoding.tsv", [("1", 5, 6, "A", "C", "S1", ".", "Noncoding"), ("X", 5, 6, "A", "C", "S1", "G00", "Missense")])
    with pytest.raises(ValueError, match="noncoding.tsv"):
        tabulate_gpu.encode_gene_rows(f, pd.Index(["G00"]))


def _serial_counts(f_mut, c, max_muts_per_sample, cap):
    """The serial route's integer bookkeeping of one cohort: (frame of transfer_gene_model, blacklist, n_syn, genes of the count table)."""
    from digdriver_amd.data_tools import mutation_tools
    from digdriver_amd.driver_model import transfer_tools as tt
    rows = tt.read_mutations_cds(f_mut)
    kept, black = mutation_tools.filter_hypermut_samples(rows, max_muts_per_sample, return_blacklist=True)
    counts = mutation_tools.mutations_per_gene(kept, max_muts_per_gene_per_sample=cap)
    m = K.model_frame(c)
    m = m.set_index(m.GENE).rename(columns=tt._GENE_RENAME)
    m["Pi_NONSYN"] = m.Pi_MIS + m.Pi_TRUNC
    for tail in ("", "_INDEL"):                                      # (any numbers: this is the integer bookkeeping)
        m["ALPHA" + tail], m["THETA" + tail] = m["MU" + tail] ** 2 / m["SIGMA" + tail] ** 2, m["SIGMA" + tail] ** 2 / m["MU" + tail]
    out = tt.transfer_gene_model(kept, counts, m, 1.0)
    n_syn = int(((kept.ANNOT == "Synonymous") & (kept.GENE != "TP53")).sum())
    return out, black, n_syn, counts, rows


@pytest.mark.parametrize("which", ["small", "long_run"])
def test_statement_gives_the_counts_of_the_serial_route(tmp_path, which):
    case = K.small_case(tmp_path) if which == "small" else K.long_run_case(tmp_path)
    st = K.statement_planes(case)
    n_black = []
    for c, f in enumerate(case["files"]):
        out, black, n_syn, counts, rows = _serial_counts(f, c, case["max_muts_per_sample"], case["max_muts_per_gene_per_sample"])
        assert list(out.index) == K.GENES
        for a, name in enumerate(K._OBS):
            assert (out[name].values.astype(np.int64) == st["obs"][:, a, c]).all(), (c, name)
        for q, cls in enumerate(("SYN", "MIS", "NONS", "SPL", "TRUNC", "NONSYN")):
            assert (out["N_SAMP_" + cls].values == st["n_samp"][:, q, c]).all(), (c, cls)
        assert (out.N_SAMP_INDEL.values == st["n_samp_indel"][:, c]).all()
        assert sorted(black) == st["blacklist"][c] and n_syn == st["n_syn"][c]
        assert ((st["n_pairs"][:, c] > 0) == np.isin(K.GENES, counts.index)).all()
        n_black.append(len(black))
        # the inputs have what the GPU test relies on
        sizes = rows.groupby(["GENE", "SAMPLE", "ANNOT"]).size()
        if which == "small":
            assert 350 <= len(rows) <= 650 and rows.SAMPLE.nunique() == 9
            assert (sizes[sizes.index.get_level_values("GENE").isin(K.GENES)] > 2).any()            # the cap of 2 binds
            assert ((rows.ANNOT == "INDEL").sum() == 0) == (c == 2)
            assert (st["n_pairs"][:, c] == 0).any() == (c == 2) == (out.OBS_SYN.dtype.kind == "f")     # the join's NaN -> float columns
            assert rows.ANNOT.isin(["Stop_loss", "Noncoding"]).any() and rows.GENE.isin(["OUT1", "OUT2"]).any()
        elif c == 0:
            assert sizes.max() == 700 and st["obs"][K.GENES.index("G03"), 1, 0] >= 500
    assert n_black == ([0, 1, 0] if which == "small" else [0, 0])
    if which == "long_run":
        assert 2800 <= sum(len(K.coding_tuples(f)[0]) for f in case["files"]) <= 3300


def test_statement_clips_as_a_number_then_casts():
    rows = [("G00", "a", "Missense")] * 3 + [("G00", "b", "Missense")] * 4 + [("G00", "c", "Missense")]
    assert S.cohort_counts(rows, ["G00"], 3e9, 2.5)["obs"] == {("G00", "Missense"): 6}              # int(2.5 + 2.5 + 1)
    frame = pd.DataFrame(rows, columns=["GENE", "SAMPLE", "ANNOT"])
    from digdriver_amd.data_tools import mutation_tools
    assert int(mutation_tools.mutations_per_gene(frame, 2.5).OBS_MIS["G00"]) == 6


def test_entry_points_are_bound_and_check_the_key_width():
    from digdriver_amd import _lib
    lib = _lib.load()
    for sym in ("dig_gene_row_keys", "dig_gene_row_keys_host", "dig_gene_counts", "dig_gene_counts_host"):
        assert sym in _lib.EXPORTED_SYMBOLS and getattr(lib, sym) is not None
    assert lib.dig_abi_version() == 12
    off = np.array([0, 1 << 30], np.int64)
    buf = np.zeros(8, np.int64)
    h = _lib.host_ptr
    rc = lib.dig_gene_row_keys_host(h(buf), h(buf), h(buf), h(buf), h(off), 0, 1 << 30, 1 << 30, 1 << 30, h(buf), h(buf), 0)
    assert rc < 0 and "63 bits" in _lib.last_error() and "dig_gene_row_keys_host" in _lib.last_error()
    rc = lib.dig_gene_counts_host(None, 0, None, 0, ctypes.c_double(1.0), ctypes.c_double(1.0), 0, 1, 1, None, None, None, None, None, 0)
    assert rc < 0 and "non-null" in _lib.last_error()


def _no_launch(monkeypatch):
    from digdriver_amd import _lib

    def refuse(name, *args):
        raise AssertionError("a library call (%s) in front of the refusal" % name)
    monkeypatch.setattr(_lib, "call", refuse)


def test_ratio_scale_factors_are_refused_before_any_device_work(tmp_path, monkeypatch):
    from digdriver_amd.driver_model import cohort_batch
    _no_launch(monkeypatch)
    for kw in (dict(scale_by_sample=True), dict(scale_by_expectation=False)):
        with pytest.raises(NotImplementedError):
            cohort_batch.run_gene_cohorts(["a.tsv"], ["a.map"], **kw)


def test_maps_with_different_gene_indices_are_refused_before_any_launch(tmp_path, monkeypatch):
    from digdriver_amd.driver_model import cohort_batch
    from digdriver_amd.io import mapfile
    maps = K.write_maps(tmp_path, 3)
    other = K.model_frame(2)
    other.loc[3, "GENE"] = "G99"
    mapfile.write_frame(maps[2], "genic_model", other)
    _no_launch(monkeypatch)
    with pytest.raises(ValueError, match="genes2.map"):
        cohort_batch.run_gene_cohorts(["a.tsv", "b.tsv", "c.tsv"], maps)
