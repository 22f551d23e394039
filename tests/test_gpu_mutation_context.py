"""addMutationContext on the MI355X: the frames and files of the reference (golden), device form against the `_host` twin, a
fuzz against a plain-Python statement of the per-row rule, and an annotated file fed on to elementDriver."""
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
from digdriver_amd.sequence_model import sequence_tools as st
from test_mutation_context_host import fasta_seqs, load_fixture, rule3, write_file

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def _gpu():
    _lib.require_device()


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    fx = load_fixture()
    d = tmp_path_factory.mktemp("mutctx")
    fx["f_fasta"] = write_file(d, "genome.fa", fx["fasta"])
    fx["paths"] = {n: write_file(d, n + ".tsv", t) for n, t in fx["inputs"].items()}
    return fx


@pytest.mark.parametrize("on_device", [True, False])
def test_frames_match_golden(_gpu, fixture, on_device):
    for case in fixture["cases"]:
        df = mutation_tools.read_mutation_file(fixture["paths"][case["input"]], drop_duplicates=False)
        out = st.add_context_to_mutations(fixture["f_fasta"], df, n_up=case["n_up"], n_down=case["n_down"], N_proc=4,
                                          collapse=case["collapse"], on_device=on_device)
        tag = (case["input"], case["n_up"], case["n_down"], case["collapse"])
        assert out.to_csv(sep="\t", index=False, header=False) == case["expected"], tag
        assert [int(i) for i in out.index] == case["index"], tag
        assert list(out.columns) == case["columns"], tag
        assert [str(t) for t in out.dtypes] == case["dtypes"], tag


def test_mutation_contexts_by_chrom_matches_rule(_gpu, fixture):
    seqs = fasta_seqs(fixture["fasta"])
    df = mutation_tools.read_mutation_file(fixture["paths"]["snv_only"], drop_duplicates=False)
    part = df[df.CHROM == 2].copy()
    out = st.mutation_contexts_by_chrom(fixture["f_fasta"], part, n_up=2, n_down=2)
    want = rule3(seqs["chr2"], part.START.tolist(), part.REF.tolist(), 2, 2)
    assert out.CONTEXT.tolist() == [w for w in want if w]
    assert (out.MUT_TYPE == out.REF + ">" + out.ALT).all()


def test_cli_bytes_both_paths(_gpu, fixture, tmp_path):
    for case in fixture["cases"]:
        if case["collapse"]:
            continue
        up, down = str(case["n_up"]), str(case["n_down"])
        fout = str(tmp_path / "cli.tsv")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "DigPreprocess.py"), "addMutationContext",
                            fixture["paths"][case["input"]], fixture["f_fasta"], fout + ".gz", "--up", up, "--down", down,
                            "--n-procs", "7"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert not os.path.exists(fout + ".gz")
        with open(fout) as f:
            assert f.read() == case["expected"], case["input"]
        for native in (True, False):
            f2 = str(tmp_path / "api.tsv")
            path = st.write_mutation_contexts(fixture["paths"][case["input"]], fixture["f_fasta"], f2, n_up=case["n_up"],
                                              n_down=case["n_down"], native=native)
            assert path == ("native" if native and case["input"] != "nan_genes" else "pandas")
            with open(f2) as f:
                assert f.read() == case["expected"], (case["input"], native)


def _fuzz_genome(rng):
    seqs = {}
    for name, n in (("chr1", 90000), ("chr2", 70000), ("chr3", 40000)):
        s = rng.choice(np.array(list("ACGT")), n)
        for _ in range(60):
            a = int(rng.integers(0, n - 50))
            s[a:a + int(rng.integers(1, 40))] = "N"
        for _ in range(60):
            a = int(rng.integers(0, n))
            s[a] = rng.choice(np.array(list("RMYKSW")))
        s[:3] = "N"
        seqs[name] = "".join(s)
    return seqs


def test_fuzz_against_rule(_gpu):
    rng = np.random.default_rng(7)
    seqs = _fuzz_genome(rng)
    g = PackedGenome.from_sequences({k: v.lower() if i == 1 else v for i, (k, v) in enumerate(seqs.items())})
    names = list(seqs)
    n = 200000
    chrom_of_row = np.sort(rng.integers(0, 3, n))
    starts, refs = np.empty(n, np.int64), []
    i = 0
    while i < n:
        c = names[chrom_of_row[i]]
        L = len(seqs[c])
        s = int(rng.choice([rng.integers(0, L), rng.integers(0, 10), rng.integers(L - 10, L)], p=[0.9, 0.05, 0.05]))
        k = min(int(rng.geometric(0.4)), n - i)                  # a run of k rows with this START (same chromosome)
        k = int(np.sum(chrom_of_row[i:i + k] == chrom_of_row[i]))
        for _ in range(k):
            u = rng.random()
            base = seqs[c][s].upper()
            refs.append(base if u < 0.8 else str(rng.choice(["A", "C", "G", "T", "a", "AC", "N", "R"])))
            starts[i] = s
            i += 1
    chroms = np.array(names, dtype=object)[chrom_of_row]
    for n_up, n_down, collapse in ((1, 1, False), (2, 2, False), (1, 0, False), (0, 0, False), (7, 8, False), (3, 1, True)):
        want = []
        for ci, c in enumerate(names):
            sel = chrom_of_row == ci
            sub_s, sub_r = starts[sel], [r for r, m in zip(refs, sel) if m]
            if collapse:                                          # the reference indexes past a short window (IndexError)
                keep = sub_s >= n_up
                sub_s, sub_r = sub_s[keep], [r for r, m in zip(sub_r, keep) if m]
            want += rule3(seqs[c], sub_s.tolist(), sub_r, n_up, n_down, collapse)
        ch, sts, rf = chroms, starts, refs
        if collapse:
            keep = np.concatenate([starts[chrom_of_row == ci] >= n_up for ci in range(3)])
            ch, sts, rf = chroms[keep], starts[keep], [r for r, m in zip(refs, keep) if m]
        status, got = st._row_contexts(g, ch, sts, np.asarray(rf, dtype=object), n_up, n_down, collapse, True)
        assert got.tolist() == want, (n_up, n_down, collapse)
        s_h, c_h = engine.mutation_contexts(g, ch, sts, rf, n_up, n_down, collapse, on_device=False)
        s_d, c_d = engine.mutation_contexts(g, ch, sts, rf, n_up, n_down, collapse, on_device=True)
        assert np.array_equal(s_h, s_d.cpu().numpy()) and np.array_equal(c_h, c_d.cpu().numpy().view(np.uint32))
        assert (status == engine.MC_KEPT).sum() > n // 3 and (status == engine.MC_HOST).sum() > 0
        assert (status == engine.MC_DROPPED).sum() > 0 and (status == engine.MC_MISMATCH).sum() > 0
    with pytest.raises(ValueError):
        engine.mutation_contexts(g, ["chr1"], [len(seqs["chr1"])], ["A"], on_device=True)


def test_annotated_file_feeds_element_driver(_gpu, fixture, tmp_path):
    """An annotated file made here and the golden annotated file give elementDriver the same results."""
    from digdriver_amd.io import mapfile
    rng = np.random.default_rng(11)
    case = next(c for c in fixture["cases"] if (c["input"], c["n_up"], c["n_down"]) == ("plain", 1, 1))
    ours = str(tmp_path / "ours.tsv")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "DigPreprocess.py"), "addMutationContext",
                        fixture["paths"]["plain"], fixture["f_fasta"], ours], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    gold = write_file(tmp_path, "gold.tsv", case["expected"])
    E = 40
    names = ["elt%02d" % i for i in range(E)]
    chrom = rng.integers(1, 4, E)
    starts = rng.integers(0, 1400, E)
    sizes = rng.integers(50, 300, E)
    bed = tmp_path / "e.bed"
    with open(bed, "w") as f:
        for nm, c, s, z in zip(names, chrom, starts, sizes):
            f.write("%d\t%d\t%d\t%s\t0\t+\t%d\t%d\t.\t1\t%d,\t0,\n" % (c, s, s + z, nm, s, s, z))
    mu, sigma, pi = rng.gamma(9.0, 3.0, E), rng.gamma(4.0, 1.0, E), sizes / 10000.0
    frame = pd.DataFrame(dict(ELT=names, ELT_SIZE=sizes, FLAG=np.zeros(E, bool), R_SIZE=10000, R_OBS=rng.poisson(mu),
                              R_INDEL=rng.poisson(mu), MU=mu, SIGMA=sigma, MU_INDEL=mu, SIGMA_INDEL=sigma, P_SUM=pi, P_INDEL=pi))
    model = str(tmp_path / "cohort.map")
    mapfile.write_frame(model, "my_elts", frame)
    texts = []
    for tag, fmut in (("ours", ours), ("gold", gold)):
        outdir = tmp_path / tag
        outdir.mkdir()
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "DigDriver.py"), "elementDriver", fmut, model, "my_elts",
                            "--f-bed", str(bed), "--outpfx", "res", "--outdir", str(outdir), "--scale-factor-manual", "1.3",
                            "--scale-factor-indel-manual", "0.13"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        files = sorted(os.listdir(outdir))
        assert len(files) == 1
        with open(outdir / files[0]) as f:
            texts.append(f.read())
    assert texts[0] == texts[1] and len(texts[0].splitlines()) == E + 1
