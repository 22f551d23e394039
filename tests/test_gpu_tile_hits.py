"""The hits of the per-base route on the GPU: dig_tile_select_count / fill (engine.tile_select, device form and `_host` twins)
against a numpy statement of the hit rule; nb_model_hits against the serial route (nb_model per cohort, filtered) bit for bit and
against the REFERENCE's own frames (tests/golden/tiled_golden.json.gz, tiled_penta_golden.json.gz); `DigDriver.py tileDriver` end
to end on maps and files written from tiled_golden."""
import functools
import gzip
import importlib.util
import itertools
import json
import os

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN, ROOT, rel_close

pytestmark = pytest.mark.gpu

SHAPES = [(3, 70, 130), (1, 5, 1), (2, 9, 64), (2, 9, 65), (1, 3, 4100)]        # rows shorter than a wave, one wave, one over, many steps
CUT_KINDS = [0.3, np.inf, -1.0, np.nan]


def _plane(shape, seed):
    """Random scores, a tenth NaN, some +-inf; n_valid from [-1, T] with 0, T and -1 present; the last row whole, every tile of
    it below any cut that takes something (a row whose every tile hits; a hit in the last tile of the last row)."""
    C, R, T = shape
    rng = np.random.default_rng(seed)
    score = rng.uniform(size=shape)
    score[rng.uniform(size=shape) < 0.1] = np.nan
    score[rng.uniform(size=shape) < 0.02] = np.inf
    score[rng.uniform(size=shape) < 0.02] = -np.inf
    nv = rng.integers(-1, T + 1, R).astype(np.int32)
    nv[:3] = [T, 0, -1][:min(R, 3)]
    nv[R - 1] = T
    score[:, R - 1, :] = -0.5                                   # (above the cut -1, which only the -inf scores pass)
    planes = dict(pt=rng.uniform(size=shape), exp=rng.uniform(size=shape) * 9, k=rng.integers(0, 7, shape).astype(np.int32))
    return score, nv, planes


def _expected(score, nv, cut, planes):
    C, R, T = score.shape
    with np.errstate(invalid="ignore"):
        hit = (np.arange(T)[None, None, :] < nv[None, :, None]) & (score <= np.asarray(cut, float).reshape(C, 1, 1))
    c, r, t = np.nonzero(hit)                                   # C order: cohort-major, then region, then tile
    want = dict(region=r.astype(np.int32), tile=t.astype(np.int32), score=score[hit], cohort_ptr=np.searchsorted(c, np.arange(C + 1)))
    want.update({name: p[hit] for name, p in planes.items()})
    return want, hit.reshape(C * R, T).sum(axis=1).astype(np.int32)


def _cut_sets(C):
    """Mixed cuts (a finite value, +inf, -1 and NaN over the cohorts, in every rotation that a single cohort needs), then no cohort
    with a hit, then every cohort with hits."""
    mixed = [[CUT_KINDS[(c + s) % 4] for c in range(C)] for s in (range(4) if C == 1 else range(2))]
    return mixed + [[-1.0] * C, [np.nan] * C, [np.inf] * C, [0.3] * C]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tile_select_device_and_host_twins_against_numpy(shape):
    import torch
    from digdriver_amd import engine
    C, R, T = shape
    score, nv, planes = _plane(shape, seed=sum(shape))
    dev = torch.device("cuda:0")
    d_score, d_nv = torch.as_tensor(score, device=dev), torch.as_tensor(nv, device=dev)
    d_planes = {k: torch.as_tensor(v, device=dev) for k, v in planes.items()}
    totals = []
    for cut in _cut_sets(C):
        want, want_counts = _expected(score, nv, cut, planes)
        totals.append(len(want["tile"]))
        got_d = engine.tile_select(d_score, d_nv, cut, **d_planes)
        got_h = engine.tile_select(score, nv, cut, **planes)
        for got, host in ((got_d, lambda x: x.cpu().numpy()), (got_h, lambda x: x)):
            assert np.array_equal(got["cohort_ptr"], want["cohort_ptr"]) and got["cohort_ptr"].dtype == np.int64
            for name in ("region", "tile", "score", "pt", "exp", "k"):
                g = host(got[name])
                assert g.dtype == want[name].dtype and g.tobytes() == want[name].tobytes(), (cut, name)
        assert np.array_equal(engine.tile_select_counts(d_score, d_nv, cut).cpu().numpy().reshape(-1), want_counts)
        assert np.array_equal(engine.tile_select_counts(score, nv, cut).reshape(-1), want_counts)
        # outputs and planes that are NULL are skipped: scores alone, and one plane without the others
        for be_score, be_nv, be_k, host in ((d_score, d_nv, d_planes["k"], lambda x: x.cpu().numpy()), (score, nv, planes["k"], lambda x: x)):
            lists = engine.tile_select(be_score, be_nv, cut, index=False)
            assert sorted(lists) == ["cohort_ptr", "score"] and host(lists["score"]).tobytes() == want["score"].tobytes()
            some = engine.tile_select(be_score, be_nv, cut, k=be_k)
            assert sorted(some) == ["cohort_ptr", "k", "region", "score", "tile"] and np.array_equal(host(some["k"]), want["k"])
    assert totals[-3] == 0 and totals[-4] <= totals[-1] <= totals[-2] and totals[-2] >= C * T      # NaN cuts: no cohort with a hit; +inf: every cohort with hits
    want, _ = _expected(score, nv, [np.inf] * C, planes)
    assert (np.diff(want["cohort_ptr"]) >= T).all() and want["region"][-1] == R - 1 and want["tile"][-1] == T - 1


def test_scalar_cut_and_refusals():
    """A single cut stands for every cohort.  C R >= 2^31 and T >= 2^31 are refused on the sizes alone (one-element buffers: the
    entry point must refuse before it reads), in both entry points."""
    import torch
    from digdriver_amd import _lib, engine
    score, nv, _ = _plane((3, 4, 5), seed=1)
    a, b = engine.tile_select(torch.as_tensor(score, device="cuda:0"), torch.as_tensor(nv, device="cuda:0"), 0.5), \
        engine.tile_select(score, nv, [0.5] * 3)
    assert np.array_equal(a["tile"].cpu().numpy(), b["tile"]) and np.array_equal(a["cohort_ptr"], b["cohort_ptr"]) and len(b["tile"]) > 5
    one = torch.zeros(1, dtype=torch.float64, device="cuda:0")
    i1 = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    o1 = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    p, s = _lib.dev_ptr, _lib.stream_ptr()
    for C, R, T, fragment in ((1 << 16, 1 << 15, 1, "C R below 2\\^31"), (1 << 31, 1, 1, "C R below 2\\^31"), (1, 1, 1 << 31, "fewer than 2\\^31 tiles")):
        with pytest.raises(_lib.DigHipError, match=fragment):
            _lib.call("dig_tile_select_count", p(one), p(i1), p(one), C, R, T, p(i1), s)
        with pytest.raises(_lib.DigHipError, match=fragment):
            _lib.call("dig_tile_select_fill", p(one), p(i1), p(one), C, R, T, p(o1), 1, None, None, None, p(i1), p(i1), p(one), None, None, None, s)
    torch.cuda.synchronize()
    assert float(one[0]) == 0.0 and int(i1[0]) == 0 and int(o1[0]) == 0


# ---- nb_model_hits against the serial route and the reference's own frames ------------------------------------------------------
PVAL_MAX, FDR = 1e-3, 0.1
# hits per (cohort 0 binsize 1, cohort 0 binsize 50, cohort 1 binsize 1, cohort 1 binsize 50), counted on the reference's frames
# on the CPU: no golden PVAL lies within 5e-3 relative of 1e-3 and no q within 8e-3 relative of 0.1, so the reference alone
# decides membership
GOLDEN_HITS = {("tiled_golden", "pval"): (22, 0, 28, 1), ("tiled_golden", "fdr"): (21, 0, 25, 8),
               ("tiled_penta_golden", "pval"): (21, 1, 24, 3), ("tiled_penta_golden", "fdr"): (14, 4, 21, 4)}


@functools.lru_cache(maxsize=None)
def _problem(name):
    from digdriver_amd.data_tools.genome import PackedGenome
    g = json.loads(gzip.open(os.path.join(GOLDEN, name + ".json.gz")).read())
    n_up = 1 if name == "tiled_golden" else 2
    ctx = ["".join(t) for t in itertools.product("ACGT", repeat=2 * n_up + 1)]
    d_prs = [coh["d_pr"] if isinstance(coh["d_pr"], dict) else dict(zip(ctx, coh["d_pr"])) for coh in g["cohorts"]]
    muts = []
    for coh in g["cohorts"]:
        m = pd.DataFrame(coh["rows"], columns=["CHROM", "START", "END", "REF", "ALT", "ID"])
        m["CHROM"] = m.CHROM.astype(str)
        muts.append(m)
    return dict(g=g, genome=PackedGenome.from_sequences(g["genome"]), n_up=n_up, d_prs=d_prs, muts=muts, idx=np.array(g["idx"]),
                mu=np.array([coh["mu"] for coh in g["cohorts"]]), sigma=np.array([coh["sigma"] for coh in g["cohorts"]]))


@functools.lru_cache(maxsize=None)
def _serial(name, binsize):
    """nb_model per cohort (computed once, left unchanged), with the q-values of the stated rule: get_q_vals of PVAL.dropna()."""
    from digdriver_amd.sequence_model import nb_model
    P = _problem(name)
    out = []
    for c in range(len(P["d_prs"])):
        df = nb_model.nb_model(P["d_prs"][c], P["idx"], P["mu"][c], P["sigma"][c], P["muts"][c], P["genome"], n_up=P["n_up"], n_down=P["n_up"],
                               binsize=binsize)
        q = pd.Series(np.nan, index=df.index)
        ok = df.PVAL.notna()
        q[ok] = nb_model.get_q_vals(df.PVAL[ok].values)
        out.append((df, q))
    return out


@functools.lru_cache(maxsize=None)
def _hits(name, binsize, mode):
    from digdriver_amd.sequence_model import nb_model
    P = _problem(name)
    kw = dict(pval_max=PVAL_MAX) if mode == "pval" else dict(fdr=FDR)
    return nb_model.nb_model_hits(P["d_prs"], P["idx"], P["mu"], P["sigma"], P["muts"], P["genome"], n_up=P["n_up"], n_down=P["n_up"],
                                  binsize=binsize, **kw)


CASES = [(n, b, m) for n in ("tiled_golden", "tiled_penta_golden") for b in (1, 50) for m in ("pval", "fdr")]


@pytest.mark.parametrize("name,binsize,mode", CASES)
def test_nb_model_hits_equals_the_filtered_serial_frames_bit_for_bit(name, binsize, mode):
    frames = _hits(name, binsize, mode)
    serial = _serial(name, binsize)
    assert len(frames) == len(serial) == 2
    for c, (got, (df, q)) in enumerate(zip(frames, serial)):
        if mode == "pval":
            want = df[df.PVAL <= PVAL_MAX]
        else:
            want = df[q <= FDR].assign(QVAL=q[q <= FDR])
        assert got.index.dtype == np.int64 and list(got.columns) == list(want.columns)
        pd.testing.assert_frame_equal(got, want, check_exact=True)
        for col in got.columns:
            if col != "REGION":
                assert got[col].values.tobytes() == want[col].values.astype(float).tobytes(), (c, col)
        assert got.attrs["n_testable"] == int(df.PVAL.notna().sum()) and got.attrs["n_tiles"] == len(df)
        if binsize == 1:
            assert got.attrs["n_testable"] < got.attrs["n_tiles"]             # NaN tiles: q-values exist only under the testable-tile rule


@pytest.mark.parametrize("name,binsize,mode", CASES)
def test_nb_model_hits_equals_the_references_own_rows(name, binsize, mode):
    """Membership by the reference's frame alone: its rows with PVAL <= 1e-3, or with q <= 0.1 over its non-NaN PVAL."""
    from digdriver_amd.sequence_model import nb_model
    frames = _hits(name, binsize, mode)
    for c, coh in enumerate(_problem(name)["g"]["cohorts"]):
        run = coh["runs"][str(binsize)]
        p = np.array(run["PVAL"], float)
        ok = ~np.isnan(p)
        if mode == "pval":
            with np.errstate(invalid="ignore"):
                keep = p <= PVAL_MAX
        else:
            keep = np.zeros(p.size, bool)
            keep[ok] = nb_model.get_q_vals(p[ok]) <= FDR
        got = frames[c]
        assert len(got) == keep.sum() == GOLDEN_HITS[(name, mode)][2 * c + (binsize == 50)]
        assert np.array_equal(got.index.values, np.flatnonzero(keep))
        assert np.array_equal(got.CHROM.values, np.array(run["CHROM"], float)[keep]) and np.array_equal(got.POS.values, np.array(run["POS"], float)[keep])
        assert np.array_equal(got.OBS.values, np.array(run["OBS"], float)[keep])
        rel_close(got.PVAL.values, p[keep], rtol=1e-6)
        np.testing.assert_allclose(got.EXP.values, np.array(run["EXP"], float)[keep], rtol=1e-12, atol=0)
        if mode == "fdr" and len(got):
            rel_close(got.QVAL.values, nb_model.get_q_vals(p[ok])[keep[ok]], rtol=1e-6)
            assert (got.QVAL.values <= FDR).all()


# ---- the command line -----------------------------------------------------------------------------------------------------------
def _cli():
    spec = importlib.util.spec_from_file_location("dig_driver_cli_tiles_gpu", os.path.join(ROOT, "scripts", "DigDriver.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tile_driver_end_to_end(tmp_path, capsys):
    """tileDriver on a FASTA, two maps (region_params from idx and each cohort's mu / sigma, sequence_model_64 from d_pr) and two
    mutation files written from tiled_golden: the .hits.txt files are nb_model_hits' frames as write_results_tsv writes them;
    --chroms 2 gives chromosome 2's rows; maps on different grids and a map without the sequence model are refused by name."""
    from digdriver_amd.io import mapfile
    P = _problem("tiled_golden")
    g, idx = P["g"], P["idx"]
    fasta = tmp_path / "genome.fa"
    fasta.write_text("".join(">%s\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))) for n, s in g["genome"].items()))
    maps, files = [], []
    for c, coh in enumerate(g["cohorts"]):
        m = str(tmp_path / ("map%d" % c))
        mapfile.write_frame(m, "region_params", pd.DataFrame({"CHROM": idx[:, 0], "START": idx[:, 1], "END": idx[:, 2],
                                                              "Y_PRED": P["mu"][c], "STD": P["sigma"][c]}))
        mapfile.write_frame(m, "sequence_model_64", pd.DataFrame({"FREQ": list(coh["d_pr"].values())},
                                                                 index=pd.Index(list(coh["d_pr"].keys()), name="CONTEXT")))
        f = tmp_path / ("muts%d.bed" % c)
        f.write_text("".join("\t".join(str(x) for x in r) + "\n" for r in coh["rows"]))
        maps.append(m)
        files.append(str(f))
    cli = _cli()
    common = "tileDriver %s --mutation-files %s --maps %s --binsize 1 " % (fasta, " ".join(files), " ".join(maps))
    cli.main(common + "--outdir %s --outpfx A B --fdr %g" % (tmp_path / "out", FDR))
    said = capsys.readouterr().out
    frames = _hits("tiled_golden", 1, "fdr")
    for pfx, frame in zip("AB", frames):
        want = tmp_path / ("want%s.txt" % pfx)
        mapfile.write_results_tsv(frame, str(want))
        assert (tmp_path / "out" / (pfx + ".hits.txt")).read_bytes() == want.read_bytes() and len(frame) > 20
        assert "%s: %d hits of %d testable tiles" % (pfx, len(frame), frame.attrs["n_testable"]) in said
    cli.main(common + "--outdir %s --outpfx A B --pval-max %g --chroms 2" % (tmp_path / "chr2", PVAL_MAX))
    full = _hits("tiled_golden", 1, "pval")
    for pfx, frame in zip("AB", full):
        got = pd.read_csv(tmp_path / "chr2" / (pfx + ".hits.txt"), sep="\t", index_col=0, float_precision="round_trip")
        want = frame[frame.CHROM == 2.0]
        assert len(want) > 0 and (frame.CHROM == 1.0).any()
        assert np.array_equal(got.POS.values, want.POS.values) and np.array_equal(got.PVAL.values, want.PVAL.values)
        assert list(got.REGION) == list(want.REGION) and (got.CHROM == 2.0).all()
    # refusals that need files: a map on another grid, a map without the sequence model of the contexts asked for
    other = str(tmp_path / "other")
    mapfile.write_frame(other, "region_params", pd.DataFrame({"CHROM": idx[:, 0], "START": idx[:, 1] + 1, "END": idx[:, 2],
                                                              "Y_PRED": P["mu"][0], "STD": P["sigma"][0]}))
    tail = " --outdir %s --outpfx A B --fdr 0.1" % (tmp_path / "no")
    with pytest.raises(ValueError, match="other"):
        cli.main("tileDriver %s --mutation-files %s --maps %s %s" % (fasta, " ".join(files), maps[0], other) + tail)
    with pytest.raises(SystemExit, match="map0.*sequence_model_1024"):
        cli.main(common + "--up 2 --down 2" + tail)
    assert not (tmp_path / "no").exists()
