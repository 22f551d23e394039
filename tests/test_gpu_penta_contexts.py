"""Penta-nucleotide context counting (dig_count_contexts5) on the MI355X: device form and `_host` twin against the reference's
golden frames, a fuzz against the numpy statement of test_penta_context_host.py, the sequence_tools frames, countGenomeContext
--up 2 --down 2, and the chain FASTA -> genome counts + annotated mutations -> train_sequence_model -> nb_model."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from conftest import ROOT
from digdriver_amd import _lib, engine
from digdriver_amd.data_tools import mutation_tools
from digdriver_amd.data_tools.genome import PackedGenome
from digdriver_amd.io import mapfile
from digdriver_amd.sequence_model import nb_model
from digdriver_amd.sequence_model import sequence_tools as st
from test_penta_context_host import CTX5, fasta_seqs, is_minus, load_fixture, rule5, rule5_regions, codes_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def _gpu():
    _lib.require_device()


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    fx = load_fixture()
    d = tmp_path_factory.mktemp("penta")
    fx["f_fasta"] = str(d / "genome.fa")
    with open(fx["f_fasta"], "w") as f:
        f.write(fx["fasta"])
    fx["genome"] = PackedGenome.from_sequences(fasta_seqs(fx["fasta"]))
    return fx


def _counts(genome, chroms, starts, ends, minus=None, on_device=True):
    out = engine.count_contexts(genome, chroms, starts, ends, minus, on_device=on_device, n_up=2, n_down=2)
    return out.cpu().numpy() if on_device else out


@pytest.mark.parametrize("on_device", [True, False])
def test_engine_matches_golden(_gpu, fx, on_device):
    r = fx["regions"]
    got = _counts(fx["genome"], r["chrom"], r["start"], r["end"], on_device=on_device)
    assert got.shape == (len(r["chrom"]), 1024) and got.dtype == np.int32
    assert np.array_equal(got, np.array(fx["by_regions"]["values"]))
    reg = fx["nonc_regions"]
    got = _counts(fx["genome"], ["chr" + x[0] for x in reg], [x[1] for x in reg], [x[2] for x in reg],
                  [is_minus(x[3]) for x in reg], on_device=on_device)
    cols = [CTX5.index(k.split(">")[0]) for k in fx["nonc"]["columns"]]
    assert np.array_equal(got[:, cols].astype(np.float64), np.array(fx["nonc"]["values"]))


def _fuzz_genome(rng, n_frac):
    """Three chromosomes: letters in either case, a fraction n_frac of other letters (N and IUPAC codes) scattered and in runs
    that start and end at every offset inside a word, chr2 longer than 131 072 bases."""
    seqs = {}
    for name, n in (("chr1", 40000), ("chr2", 150000), ("chr3", 7001)):
        s = rng.choice(np.array(list("ACGTacgt")), n)
        if n_frac:
            m = rng.random(n) < n_frac / 2
            s[m] = rng.choice(np.array(list("NnRYKMSWBDHV")), int(m.sum()))
            pos, cov = 0, 0
            while cov < n_frac * n / 2 and pos < n - 200:          # runs at every start offset mod 32, lengths 1 .. 40
                a = pos + int(rng.integers(0, 64))
                ln = int(rng.integers(1, 41))
                s[a:a + ln] = rng.choice(np.array(list("NNNNR")))
                cov += ln
                pos = a + ln + int(rng.integers(1, max(2, int(60 / max(n_frac, 0.02)))))
        seqs[name] = "".join(s)
    return seqs


def _fuzz_regions(rng, seqs):
    chroms, starts, ends, minus = [], [], [], []
    names = list(seqs)
    for _ in range(1500):
        c = names[int(rng.integers(0, len(names)))]
        L = len(seqs[c])
        a = 0 if rng.random() < 0.05 else int(rng.integers(2, L + 40))
        chroms.append(c)
        starts.append(a)
        ends.append(a + int(rng.integers(0, 3001)))
        minus.append(bool(rng.random() < 0.5))
    for off in range(32):                                          # every word / word-pair alignment of both ends
        for ln in (0, 1, 5, 17, 33, 2048 + off):
            a = 1000 + off
            chroms.append("chr1"), starts.append(a), ends.append(a + ln), minus.append(bool(off & 1))
    for c in names:                                                # whole chromosomes, both strands
        for m in (False, True):
            chroms.append(c), starts.append(0), ends.append(len(seqs[c])), minus.append(m)
    chroms.append("chr2"), starts.append(5), ends.append(5 + 140000), minus.append(False)     # > 131 072 bases
    return chroms, starts, ends, minus


@pytest.mark.parametrize("n_frac", [0.0, 0.01, 0.2, 0.9])
def test_fuzz_against_statement(_gpu, n_frac):
    rng = np.random.default_rng(int(n_frac * 1000) + 7)
    seqs = _fuzz_genome(rng, n_frac)
    g = PackedGenome.from_sequences(seqs)
    chroms, starts, ends, minus = _fuzz_regions(rng, seqs)
    want = rule5_regions(seqs, chroms, starts, ends, minus)
    got = _counts(g, chroms, starts, ends, minus)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, [(chroms[i], starts[i], ends[i], minus[i]) for i in bad[:5]]
    host = _counts(g, chroms[-40:], starts[-40:], ends[-40:], minus[-40:], on_device=False)
    assert np.array_equal(host, want[-40:])


def test_many_more_regions_than_waves(_gpu):
    rng = np.random.default_rng(11)
    seqs = _fuzz_genome(rng, 0.01)
    g = PackedGenome.from_sequences(seqs)
    R = 60000                                                      # the grid holds at most 8 192 waves (256 CUs x 32)
    starts = rng.integers(2, 39000, R)
    ends = starts + rng.integers(0, 300, R)
    minus = rng.random(R) < 0.5
    got = _counts(g, ["chr1"] * R, starts, ends, minus)
    codes = codes_of(seqs["chr1"])
    pick = np.concatenate([np.arange(50), rng.integers(0, R, 400), np.arange(R - 50, R)])
    for i in pick:
        assert np.array_equal(got[i], rule5(codes, int(starts[i]), int(ends[i]), bool(minus[i]))), i
    # row sums: every centre whose window holds ACGT only, counted once
    ok = (np.lib.stride_tricks.sliding_window_view(codes, 5) >= 0).all(axis=1)
    pre = np.concatenate([[0], np.cumsum(ok)])
    e = np.minimum(ends, len(codes) - 2)
    want = np.where(e > starts, pre[np.maximum(e, starts) - 2] - pre[starts - 2], 0)
    assert np.array_equal(got.sum(axis=1), want)


def test_start_one_raises(_gpu, fx):
    with pytest.raises(ValueError):
        engine.count_contexts(fx["genome"], ["chr1"], [1], [100], n_up=2, n_down=2)
    with pytest.raises(ValueError):
        st.count_contexts_by_regions(fx["genome"], ["chr1"], [1], [100], n_up=2, n_down=2)


def _check_frame(df, want):
    assert list(df.columns) == want["columns"]
    assert [str(i) for i in df.index] == want["index"]
    assert np.array_equal(df.values, np.array(want["values"]))


def test_sequence_tools_frames(_gpu, fx):
    r = fx["regions"]
    _check_frame(st.count_contexts_by_regions(fx["f_fasta"], r["chrom"], r["start"], r["end"], n_up=2, n_down=2), fx["by_regions"])
    _check_frame(st.count_contexts_by_regions(fx["f_fasta"], r["chrom"], r["start"], r["end"]), fx["by_regions"])     # the defaults
    _check_frame(st.count_contexts_by_regions(fx["f_fasta"], r["chrom"], r["start"], r["end"], n_up=2, n_down=2, collapse=True),
                 fx["by_regions_collapse"])
    nonc = st.nonc_elt_context_count([tuple(x) for x in fx["nonc_regions"]], st.mk_trans_idx(2, 2), fx["f_fasta"], n_up=2, n_down=2)
    _check_frame(nonc, fx["nonc"])
    df_bed = pd.DataFrame({0: [c[3:] for c in r["chrom"]], 1: r["start"], 2: r["end"]})
    _check_frame(st.count_contexts_in_bed(fx["f_fasta"], df_bed, n_up=2, n_down=2), fx["by_regions"])
    # the reference's precount ignores n_up / n_down (trinucleotide counts): the (2, 2) call equals the (1, 1) call
    bed = os.path.join(os.path.dirname(fx["f_fasta"]), "elts.bed")
    pd.DataFrame([["chr" + x[0], x[1], x[2], "e%d" % i, 0, x[3] if x[3] in ("+", "-") else "+"]
                  for i, x in enumerate(fx["nonc_regions"])]).to_csv(bed, sep="\t", header=False, index=False)
    a = st.precount_region_contexts_parallel(bed, fx["f_fasta"], 1, 10000, sub_elts=False, n_up=2, n_down=2)
    b = st.precount_region_contexts_parallel(bed, fx["f_fasta"], 1, 10000, sub_elts=False)
    assert a.shape[1] == 192 and a.equals(b)


def _run(*args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "DigPreprocess.py")] + [str(a) for a in args],
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def _seeded_fasta(path, rng):
    seqs = {}
    for name, n in (("chr1", 60000), ("chr2", 45000), ("chr3", 30001)):
        s = rng.choice(np.array(list("ACGT")), n)
        for _ in range(8):
            a = int(rng.integers(0, n - 400))
            s[a:a + int(rng.integers(1, 300))] = "N"
        s = "".join(s)
        for _ in range(6):
            a = int(rng.integers(0, n - 500))
            s = s[:a] + s[a:a + 400].lower() + s[a + 400:]
        seqs[name] = s
    with open(path, "w") as f:
        for n, s in seqs.items():
            f.write(">%s\n%s\n" % (n, "\n".join(s[i:i + 70] for i in range(0, len(s), 70))))
    return seqs


def _windows(seqs, w):
    return [(int(n[3:]), a, a + w) for n in seqs for a in range(0, len(seqs[n]), w)]


def test_count_genome_context_round_trip(_gpu, tmp_path):
    rng = np.random.default_rng(31)
    fa = str(tmp_path / "g.fa")
    seqs = _seeded_fasta(fa, rng)
    win = _windows(seqs, 5000)
    bed = tmp_path / "w.bed"
    bed.write_text("".join("%d\t%d\t%d\n" % w for w in win))
    for ext in (".map", ".h5"):
        gc = str(tmp_path / ("gc" + ext))
        _run("countGenomeContext", fa, gc, "--bed", bed, "--up", "2", "--down", "2")
        want = rule5_regions(seqs, ["chr%d" % w[0] for w in win], [w[1] for w in win], [w[2] for w in win])
        allw = mapfile.read_frame(gc, "all_window_genome_counts")
        assert list(allw.columns) == CTX5 and np.array_equal(allw.values, want)
        assert list(allw.index) == ["chr%d:%d-%d" % w for w in win]
        tot = mapfile.read_frame(gc, "genome_counts")
        assert list(tot.columns) == ["COUNT"] and list(tot.index) == CTX5
        assert np.array_equal(tot.COUNT.values, want.sum(axis=0))
        assert np.array_equal(mapfile.read_array(gc, "idx"), np.array(win, np.int32))
        attrs = mapfile.read_attrs(gc)
        assert (int(attrs["n_up"]), int(attrs["n_down"]), int(attrs["collapse"])) == (2, 2, 0)


def test_chain_genome_counts_mutations_model(_gpu, tmp_path):
    """countGenomeContext and addMutationContext (--up 2 --down 2) on one seeded FASTA feed train_sequence_model(n_up=2):
    the model equals the one built from the statement's counts, and nb_model(n_up=2) runs on it."""
    rng = np.random.default_rng(47)
    fa = str(tmp_path / "g.fa")
    seqs = _seeded_fasta(fa, rng)
    win = _windows(seqs, 10000)
    bed = tmp_path / "w.bed"
    bed.write_text("".join("%d\t%d\t%d\n" % w for w in win))
    gc = str(tmp_path / "gc.map")
    _run("countGenomeContext", fa, gc, "--bed", bed, "--up", "2", "--down", "2")
    rows = []
    up = {k: v.upper() for k, v in seqs.items()}
    for _ in range(20000):
        c = int(rng.integers(1, 4))
        p = int(rng.integers(2, len(up["chr%d" % c]) - 3))
        ref = up["chr%d" % c][p]
        alt = "A" if ref != "A" else "G"
        rows.append("%d\t%d\t%d\t%s\t%s\tS%d\tG%d\tNoncoding\n" % (c, p, p + 1, ref, alt, rng.integers(0, 20), rng.integers(0, 9)))
    fmut = tmp_path / "m.tsv"
    fmut.write_text("".join(rows))
    fann = str(tmp_path / "annotated.tsv")
    _run("addMutationContext", fmut, fa, fann, "--up", "2", "--down", "2")
    df_mut = mutation_tools.read_mutation_file(fann, drop_duplicates=False)
    assert len(df_mut) > 15000 and (df_mut.CONTEXT.str.len() == 5).all()
    regions = np.array(win)
    S_cli = mapfile.read_frame(gc, "genome_counts").COUNT
    want = rule5_regions(seqs, ["chr%d" % w[0] for w in win], [w[1] for w in win], [w[2] for w in win]).sum(axis=0)
    assert (want > 0).all()
    S_rule = pd.Series(want, index=CTX5)
    f_cli, c_cli = st.train_sequence_model(regions, df_mut, S_cli, n_up=2, n_down=2)
    f_rule, c_rule = st.train_sequence_model(regions, df_mut, S_rule, n_up=2, n_down=2)
    assert len(f_cli) == 3072 and len(c_cli) == 1024 and list(c_cli.index) == CTX5
    assert f_cli.COUNT.sum() == len(df_mut.drop_duplicates())
    pd.testing.assert_frame_equal(f_cli, f_rule)
    pd.testing.assert_frame_equal(c_cli, c_rule)
    idx = np.array(win[:6])
    df = nb_model.nb_model(c_cli.FREQ, idx, [5.0] * len(idx), [2.0] * len(idx), df_mut, fa, n_up=2, n_down=2)
    assert len(df) > 0 and (df.Pi.values >= 0).all()
    np.testing.assert_allclose(df.groupby("REGION").Pi.sum().values, 1.0, rtol=1e-9)      # per-region tile probabilities
    live = df.Pi.values > 0                                        # (a tile inside an N run has no context: Pi 0, no test)
    assert live.mean() > 0.9 and np.isfinite(df.PVAL.values[live]).all() and np.isfinite(df.EXP.values).all()
