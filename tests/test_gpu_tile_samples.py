"""The counts by sample of the per-base route on the GPU (dig_tile_sample_keys, the key sort, dig_tile_sample_counts behind
engine.tile_sample_counts; the sample options of nb_model, nb_model_hits and `DigDriver.py tileDriver`) on the problem of
tile_samples_cases.py.  Everything is compared exactly: counts are integers, and p-values come from the same kernel on equal inputs.
  1  k_cap, k_samples of the device entry points and of the `_host` twins equal the plain-Python statement
  2  no cap, no filter: k_cap is engine.tile_mut_counts bit for bit; cap 1: k_cap is k_samples
  3  nb_model / nb_model_hits with the options on the full rows equal the EXISTING route on rows thinned on the host by the statement
  4  tileDriver in fresh child processes: the new columns in their order; without the options the bytes of before
The kernels launch one thread per key on an uncapped grid (row_blocks), so there is no grid-stride pass to test."""
import functools
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from conftest import ROOT
import tile_samples_cases as K
import tile_samples_statement as S

pytestmark = pytest.mark.gpu

PVAL_MAX, FDR = 1e-3, 0.1


@functools.lru_cache(maxsize=None)
def _problem():
    from digdriver_amd.data_tools.genome import PackedGenome
    rows = K.cohort_rows()
    mu, sigma = K.mu_sigma()
    return dict(genome=PackedGenome.from_sequences(K.genome_sequences()), rows=rows, frames=K.frames(rows), st=K.stacked(rows),
                d_prs=[K.s_prob(c) for c in range(K.C)], mu=mu, sigma=sigma, chroms=[str(c) for c in K.IDX[:, 0]])


@functools.lru_cache(maxsize=None)
def _tiles(binsize):
    """(first_pos, n_valid) host arrays, n_tiles, and the same as device tensors: what base_tile_probs says about the regions."""
    from digdriver_amd import engine
    from digdriver_amd.sequence_model import nb_model
    P = _problem()
    s_prob = np.stack([nb_model._s_prob_table(d, 1) for d in P["d_prs"]])
    _, first, nval = engine.base_tile_probs(P["genome"], P["chroms"], K.IDX[:, 1], K.IDX[:, 2], s_prob, binsize)
    first_h, nval_h = first.cpu().numpy(), nval.cpu().numpy()
    T = -(-400 // binsize)
    # the regions are what the module's docstring says: whole, one tile short, all N (tiles exist), cut off, whole, without a position
    assert list(nval_h[:5]) == [T, -(-350 // binsize), T, -(-149 // binsize), T] and nval_h[5] <= 0
    assert list(first_h[:5]) == [100, 500, 1000, 1850, 200]
    return first_h, nval_h, T, first, nval


@functools.lru_cache(maxsize=None)
def _keep():
    st = _problem()["st"]
    keep = np.array(S.keep_from_max_muts([int(s) for s in st["sample"]], int(st["sample_offsets"][-1]), K.MAX_MUTS_PER_SAMPLE), np.uint8)
    names = st["names"][0]
    assert keep.sum() == len(keep) - 1 and keep[names.index("HYPER")] == 0 and keep[names.index("HOT")] == 1
    return keep


def _with_foreign_cohorts(st):
    """The stack with two more rows in the busiest tile whose cohort ids lie outside [0, C)."""
    extra = dict(chrom=["1", "1"], start=[305, 305], end=[306, 306], cohort=[-1, K.C], sample=[0, 0])
    return {k: np.concatenate([st[k], np.array(extra[k], st[k].dtype)]) for k in extra}


def _counts(binsize, rows, keep, cap, device):
    """engine.tile_sample_counts on device tensors or, device=False, on host arrays (the `_host` twins), as host arrays."""
    import torch
    from digdriver_amd import engine
    P = _problem()
    first_h, nval_h, T, first_d, nval_d = _tiles(binsize)
    up = (lambda x: None if x is None else torch.as_tensor(x, device="cuda:0")) if device else (lambda x: x)
    first, nval = (first_d, nval_d) if device else (first_h, nval_h)
    got = engine.tile_sample_counts(P["genome"], P["chroms"], K.IDX[:, 1], K.IDX[:, 2], first, nval, rows["chrom"], up(rows["start"]),
                                    up(rows["end"]), up(rows["cohort"]), up(rows["sample"]), P["st"]["sample_offsets"], up(keep), cap, K.C,
                                    binsize, T)
    return tuple(g.cpu().numpy() if device else g for g in got)


@functools.lru_cache(maxsize=None)
def _statement(binsize, filtered, cap):
    P = _problem()
    first_h, nval_h, T, _, _ = _tiles(binsize)
    rows = K.statement_rows(_with_foreign_cohorts(P["st"]))
    k_cap, k_samples = S.tile_sample_counts(K.statement_regions(first_h, nval_h), rows, K.C, binsize, T,
                                            keep=list(_keep()) if filtered else None, cap=cap)
    return np.array(k_cap, np.int32), np.array(k_samples, np.int32)


@pytest.mark.parametrize("binsize", K.BINSIZES)
@pytest.mark.parametrize("filtered,cap", [(True, K.CAP), (False, None), (True, 1), (False, 299)])
def test_counts_of_device_and_host_twins_equal_the_statement(binsize, filtered, cap):
    rows = _with_foreign_cohorts(_problem()["st"])
    want_cap, want_samples = _statement(binsize, filtered, cap)
    for device in (True, False):
        k_cap, k_samples = _counts(binsize, rows, _keep() if filtered else None, cap, device)
        assert k_cap.dtype == k_samples.dtype == np.int32 and k_cap.shape == want_cap.shape
        assert np.array_equal(k_cap, want_cap), (device, np.argwhere(k_cap != want_cap)[:5])
        assert np.array_equal(k_samples, want_samples), (device, np.argwhere(k_samples != want_samples)[:5])
    # what the problem was built to hold (bin size 50: region 0, HOT in tile 1, the 70 samples in tile 4, S1 in tiles 4 and 5)
    hot, busy = ((0, 0, 1), (0, 0, 4)) if binsize == 50 else ((0, 0, 60), (0, 0, 205))
    assert want_samples[busy] >= 70 and want_cap[hot] >= (300 if cap is None else min(300, cap))
    assert (want_cap[:, 5] == 0).all() and want_cap[:, 2].sum() > 0 and want_cap[0, 3].sum() > 0


@pytest.mark.parametrize("binsize", K.BINSIZES)
def test_without_cap_and_filter_the_counts_are_tile_mut_counts_and_cap_one_counts_samples(binsize):
    import torch
    from digdriver_amd import engine
    P = _problem()
    rows = _with_foreign_cohorts(P["st"])
    first_h, nval_h, T, first_d, nval_d = _tiles(binsize)
    up = lambda x: torch.as_tensor(x, device="cuda:0")
    plain = engine.tile_mut_counts(P["genome"], P["chroms"], K.IDX[:, 1], K.IDX[:, 2], first_d, nval_d, rows["chrom"], up(rows["start"]),
                                   up(rows["end"]), up(rows["cohort"]), K.C, binsize, T).cpu().numpy()
    k_cap, k_samples = _counts(binsize, rows, None, None, True)
    assert k_cap.tobytes() == plain.tobytes() and plain.sum() > 1500
    one, samples = _counts(binsize, rows, None, 1, True)
    assert np.array_equal(one, samples) and np.array_equal(samples, k_samples) and (k_cap > k_samples).any()


def test_no_pairs_no_rows_and_a_sample_outside_its_cohort():
    """Rows that overlap no region, and no rows at all: both planes zero, on both backends.  A row that names a sample of another
    cohort is refused by name."""
    P = _problem()
    st = P["st"]
    nowhere = dict(chrom=np.array(["2"] * 5), start=np.arange(5, dtype=np.int64), end=np.arange(5, dtype=np.int64) + 1,
                   cohort=np.zeros(5, np.int32), sample=np.zeros(5, np.int32))
    none = {k: v[:0] for k, v in nowhere.items()}
    for rows in (nowhere, none):
        for device in (True, False):
            k_cap, k_samples = _counts(50, rows, None, K.CAP, device)
            assert k_cap.shape == (K.C, 6, 8) and not k_cap.any() and not k_samples.any()
    bad = dict(nowhere, sample=np.full(5, st["sample_offsets"][1], np.int32))
    for device in (True, False):
        with pytest.raises(ValueError, match="global sample within its cohort"):
            _counts(50, bad, None, None, device)


# ---- against the route that is pinned to the reference: the existing code on rows thinned on the host ----------------------------
@functools.lru_cache(maxsize=None)
def _thinned_frames(binsize, cap):
    """Per cohort the frame of the rows the statement leaves: dropped samples removed, min(n, cap) rows per (tile, sample)."""
    P = _problem()
    first_h, nval_h, T, _, _ = _tiles(binsize)
    st = P["st"]
    stay = S.thinned_rows(K.statement_regions(first_h, nval_h), K.statement_rows(st), K.C, binsize, T, keep=list(_keep()), cap=cap)
    stay = np.array(stay)
    bounds = np.concatenate([[0], np.cumsum([len(r) for r in P["rows"]])])
    out = []
    for c, frame in enumerate(P["frames"]):
        mine = stay[(stay >= bounds[c]) & (stay < bounds[c + 1])] - bounds[c]
        out.append(frame.iloc[mine].reset_index(drop=True))
    assert len(out[0]) < len(P["frames"][0]) - 400          # (HYPER's rows and all but `cap` of HOT's are gone)
    return out


@functools.lru_cache(maxsize=None)
def _existing_route(binsize, cap):
    """nb_model as it was before the sample options (no option: no sample column read), per cohort, on the thinned rows; with the
    q-values of the stated rule."""
    from digdriver_amd.sequence_model import nb_model
    P = _problem()
    out = []
    for c, frame in enumerate(_thinned_frames(binsize, cap)):
        df = nb_model.nb_model(P["d_prs"][c], K.IDX, P["mu"][c], P["sigma"][c], frame.drop(columns="ID"), P["genome"], n_up=1, n_down=1,
                               binsize=binsize)
        q = pd.Series(np.nan, index=df.index)
        ok = df.PVAL.notna()
        q[ok] = nb_model.get_q_vals(df.PVAL[ok].values)
        out.append((df, q))
    return out


def _same_bits(got, want, what):
    assert len(got) == len(want), what
    assert np.asarray(got, float).tobytes() == np.asarray(want, float).tobytes(), what


@pytest.mark.parametrize("binsize", K.BINSIZES)
def test_nb_model_with_the_options_equals_the_existing_route_on_thinned_rows(binsize):
    from digdriver_amd.sequence_model import nb_model
    P = _problem()
    capped, single = _existing_route(binsize, K.CAP), _existing_route(binsize, 1)
    for c in range(K.C):
        got = nb_model.nb_model(P["d_prs"][c], K.IDX, P["mu"][c], P["sigma"][c], P["frames"][c], P["genome"], n_up=1, n_down=1,
                                binsize=binsize, max_muts_per_sample=K.MAX_MUTS_PER_SAMPLE, max_muts_per_tile_per_sample=K.CAP, by_sample=True)
        want, one = capped[c][0], single[c][0]
        assert list(got.columns) == list(want.columns) + ["OBS_SAMPLES", "PVAL_SAMPLE"] and len(got) == len(want) > 0
        pd.testing.assert_frame_equal(got[want.columns], want, check_exact=True)
        for col in want.columns:
            if col != "REGION":
                _same_bits(got[col], want[col], (c, col))
        _same_bits(got.OBS_SAMPLES, one.OBS, (c, "OBS_SAMPLES"))
        _same_bits(got.PVAL_SAMPLE, one.PVAL, (c, "PVAL_SAMPLE"))
        # without by_sample: the columns of before
        plain = nb_model.nb_model(P["d_prs"][c], K.IDX, P["mu"][c], P["sigma"][c], P["frames"][c], P["genome"], n_up=1, n_down=1,
                                  binsize=binsize, max_muts_per_sample=K.MAX_MUTS_PER_SAMPLE, max_muts_per_tile_per_sample=K.CAP)
        pd.testing.assert_frame_equal(plain, want, check_exact=True)
    assert (capped[0][0].OBS != single[0][0].OBS).any()


@pytest.mark.parametrize("binsize", K.BINSIZES)
@pytest.mark.parametrize("mode", ["pval", "fdr"])
@pytest.mark.parametrize("cut_on", ["PVAL", "PVAL_SAMPLE"])
def test_nb_model_hits_with_the_options_equals_the_existing_route_on_thinned_rows(binsize, mode, cut_on):
    """The hits are the rows of the full frame -- the existing route on the thinned rows, its OBS / PVAL on the one-row-per-(tile,
    sample) rows as OBS_SAMPLES / PVAL_SAMPLE -- that pass the cut on the chosen score, with that score's q-values."""
    from digdriver_amd.sequence_model import nb_model
    P = _problem()
    kw = dict(pval_max=PVAL_MAX) if mode == "pval" else dict(fdr=FDR)
    frames = nb_model.nb_model_hits(P["d_prs"], K.IDX, P["mu"], P["sigma"], P["frames"], P["genome"], n_up=1, n_down=1, binsize=binsize,
                                    max_muts_per_sample=K.MAX_MUTS_PER_SAMPLE, max_muts_per_tile_per_sample=K.CAP, by_sample=True,
                                    cut_on=cut_on, **kw)
    capped, single = _existing_route(binsize, K.CAP), _existing_route(binsize, 1)
    n_hits = n_rows = 0
    for c, got in enumerate(frames):
        (full, q_cap), (one, q_one) = capped[c], single[c]
        score, q = (full.PVAL, q_cap) if cut_on == "PVAL" else (one.PVAL, q_one)
        sel = (score <= PVAL_MAX) if mode == "pval" else (q <= FDR)
        want = full[sel].assign(OBS_SAMPLES=one.OBS[sel], PVAL_SAMPLE=one.PVAL[sel])
        if mode == "fdr":
            want = want.assign(QVAL=q[sel])
        assert list(got.columns) == list(want.columns) and got.index.dtype == np.int64
        assert list(got.columns)[9:] == ["OBS_SAMPLES", "PVAL_SAMPLE"] + (["QVAL"] if mode == "fdr" else [])
        pd.testing.assert_frame_equal(got, want, check_exact=True)
        for col in got.columns:
            if col != "REGION":
                _same_bits(got[col], want[col], (c, col))
        assert got.attrs["n_testable"] == int(score.notna().sum()) and got.attrs["n_tiles"] == len(full)
        n_hits, n_rows = n_hits + len(got), n_rows + len(full)
    assert 0 < n_hits < n_rows


def test_the_hits_of_the_existing_route_on_thinned_rows_are_the_hits_with_a_cap_and_a_filter():
    """nb_model_hits itself, without a sample column, on the thinned rows against nb_model_hits with the cap and the filter on the
    full rows: frame for frame, QVAL included."""
    from digdriver_amd.sequence_model import nb_model
    P = _problem()
    common = dict(n_up=1, n_down=1, binsize=50, fdr=FDR)
    got = nb_model.nb_model_hits(P["d_prs"], K.IDX, P["mu"], P["sigma"], P["frames"], P["genome"], max_muts_per_sample=K.MAX_MUTS_PER_SAMPLE,
                                 max_muts_per_tile_per_sample=K.CAP, **common)
    want = nb_model.nb_model_hits(P["d_prs"], K.IDX, P["mu"], P["sigma"], [f.drop(columns="ID") for f in _thinned_frames(50, K.CAP)],
                                  P["genome"], **common)
    for g, w in zip(got, want):
        pd.testing.assert_frame_equal(g, w, check_exact=True)
        assert g.attrs == w.attrs


# ---- the command line ----------------------------------------------------------------------------------------------------------
def test_tile_driver_in_fresh_child_processes(tmp_path):
    """`DigDriver.py tileDriver` twice, each in a child process of its own: with the four options the .hits.txt files are
    nb_model_hits' frames with the new columns in the stated order; without them the bytes are those of nb_model_hits without a sample
    column (the files then need no labels: column 6 is cut off the copies that run reads)."""
    from digdriver_amd.io import mapfile
    from digdriver_amd.sequence_model import nb_model
    P = _problem()
    fasta = tmp_path / "genome.fa"
    fasta.write_text("".join(">%s\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))) for n, s in K.genome_sequences().items()))
    maps, files, bare = [], [], []
    for c in range(K.C):
        m = str(tmp_path / ("map%d" % c))
        mapfile.write_frame(m, "region_params", pd.DataFrame({"CHROM": K.IDX[:, 0], "START": K.IDX[:, 1], "END": K.IDX[:, 2],
                                                              "Y_PRED": P["mu"][c], "STD": P["sigma"][c]}))
        mapfile.write_frame(m, "sequence_model_64", pd.DataFrame({"FREQ": list(P["d_prs"][c].values())},
                                                                 index=pd.Index(list(P["d_prs"][c].keys()), name="CONTEXT")))
        maps.append(m)
        files.append(K.write_file(tmp_path / ("muts%d.bed" % c), P["rows"][c], chr_prefix=c == 1, gz=False, extra_columns=c))
        b = tmp_path / ("bare%d.bed" % c)
        b.write_text("".join("%s\t%d\t%d\n" % r[:3] for r in P["rows"][c]))
        bare.append(str(b))
    script = os.path.join(ROOT, "scripts", "DigDriver.py")
    head = [sys.executable, script, "tileDriver", str(fasta), "--maps"] + maps + ["--binsize", "50", "--outpfx", "A", "B", "C", "--fdr", str(FDR)]
    runs = [subprocess.Popen(head + ["--mutation-files"] + files + ["--outdir", str(tmp_path / "new"), "--max-muts-per-sample",
                                                                    str(K.MAX_MUTS_PER_SAMPLE), "--max-muts-per-tile-per-sample", str(K.CAP),
                                                                    "--by-sample", "--cut-on", "PVAL_SAMPLE"],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True),
            subprocess.Popen(head + ["--mutation-files"] + bare + ["--outdir", str(tmp_path / "old")], stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True)]
    for run in runs:
        said, _ = run.communicate(timeout=300)
        assert run.returncode == 0, said
    common = dict(n_up=1, n_down=1, binsize=50, fdr=FDR)
    new = nb_model.nb_model_hits(P["d_prs"], K.IDX, P["mu"], P["sigma"], P["frames"], P["genome"], max_muts_per_sample=K.MAX_MUTS_PER_SAMPLE,
                                 max_muts_per_tile_per_sample=K.CAP, by_sample=True, cut_on="PVAL_SAMPLE", **common)
    old = nb_model.nb_model_hits(P["d_prs"], K.IDX, P["mu"], P["sigma"], [f.drop(columns="ID") for f in P["frames"]], P["genome"], **common)
    for pfx, n, o in zip("ABC", new, old):
        for sub, frame in (("new", n), ("old", o)):
            want = tmp_path / ("want_%s_%s.txt" % (sub, pfx))
            mapfile.write_results_tsv(frame, str(want))
            assert (tmp_path / sub / (pfx + ".hits.txt")).read_bytes() == want.read_bytes(), (sub, pfx)
        header = (tmp_path / "new" / (pfx + ".hits.txt")).read_text().split("\n")[0].split("\t")
        assert header[1:] == ["CHROM", "POS", "OBS", "EXP", "PVAL", "Pi", "MU", "SIGMA", "REGION", "OBS_SAMPLES", "PVAL_SAMPLE", "QVAL"]
        assert (tmp_path / "old" / (pfx + ".hits.txt")).read_text().split("\n")[0].split("\t")[1:] == header[1:10] + ["QVAL"]
    assert sum(len(f) for f in new) > 0
