"""Penta-nucleotide context counting without a GPU: a plain numpy statement of the reference's counting rule
(fetch_sequence + count_sequence_context + nonc_elt_context_count with n_up = n_down = 2) against the golden frames of the
reference, the column orders of the 1 024 / 512 / 3 072 layouts, sequence-model training on the golden inputs, and the
argument checks that fail before any device is touched."""
import gzip
import itertools as it
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN, ROOT
from digdriver_amd import engine
from digdriver_amd.data_tools import mutation_tools
from digdriver_amd.data_tools.genome import PackedGenome
from digdriver_amd.sequence_model import sequence_tools as st

_CODE = np.full(256, -1, np.int64)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _i
    _CODE[ord(_c.lower())] = _i
CTX5 = ["".join(t) for t in it.product("ACGT", repeat=5)]
_COMP = str.maketrans("ACGT", "TGCA")
REVCOMP5 = np.array([CTX5.index(c[::-1].translate(_COMP)) for c in CTX5])


def load_fixture():
    with gzip.open(os.path.join(GOLDEN, "penta_context_golden.json.gz"), "rt") as f:
        return json.load(f)


def fasta_seqs(text):
    seqs, name = {}, None
    for line in text.splitlines():
        if line.startswith(">"):
            name = line[1:].split()[0]
            seqs[name] = []
        elif line:
            seqs[name].append(line)
    return {k: "".join(v) for k, v in seqs.items()}


def codes_of(seq):
    """0-3 for ACGT in either case, -1 for every other letter."""
    return _CODE[np.frombuffer(seq.encode("ascii"), np.uint8)]


def rule5(codes, start, end, minus=False):
    """Counts [1024] (itertools.product('ACGT', repeat=5) order) of one region: centres [s, e), s = 2 if START == 0 else
    START, e = min(END, len - 2); a window holding a letter other than ACGT is skipped; '-' strand: out[ctx] =
    plus[revcomp(ctx)].  0 < START < 2 raises ValueError (the reference's fetch would start before the chromosome)."""
    if 0 < start < 2:
        raise ValueError("START %d" % start)
    s = 2 if start == 0 else int(start)
    e = min(int(end), len(codes) - 2)
    out = np.zeros(1024, np.int64)
    if e > s:
        win = codes[np.arange(s, e)[:, None] + np.arange(-2, 3)]
        ok = (win >= 0).all(axis=1)
        out = np.bincount((win[ok] * 4 ** np.arange(4, -1, -1)).sum(axis=1), minlength=1024).astype(np.int64)
    return out[REVCOMP5] if minus else out


def rule5_regions(seqs, chroms, starts, ends, minus=None):
    codes = {k: codes_of(v) for k, v in seqs.items()}
    minus = [False] * len(chroms) if minus is None else minus
    return np.stack([rule5(codes[c], s, e, m) for c, s, e, m in zip(chroms, starts, ends, minus)]) if len(chroms) \
        else np.zeros((0, 1024), np.int64)


def is_minus(strand):
    return strand == "-" or strand == -1


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


def test_fixture_size():
    assert os.path.getsize(os.path.join(GOLDEN, "penta_context_golden.json.gz")) < 512 * 1024


def test_statement_reproduces_region_counts(fx):
    seqs = fasta_seqs(fx["fasta"])
    r = fx["regions"]
    want = rule5_regions(seqs, r["chrom"], r["start"], r["end"])
    got = fx["by_regions"]
    assert np.array_equal(np.array(got["values"], np.int64), want)
    assert got["index"] == ["{}:{}-{}".format(c, s, e) for c, s, e in zip(r["chrom"], r["start"], r["end"])]
    # collapse=True: a context plus its reverse complement, pyrimidine-centred columns
    half = [CTX5.index(c) for c in fx["by_regions_collapse"]["columns"]]
    folded = want[:, half] + want[:, REVCOMP5[half]]
    assert np.array_equal(np.array(fx["by_regions_collapse"]["values"], np.int64), folded)


def test_statement_reproduces_nonc_counts(fx):
    seqs = {k[3:]: v for k, v in fasta_seqs(fx["fasta"]).items()}
    reg = fx["nonc_regions"]
    want = rule5_regions(seqs, [r[0] for r in reg], [r[1] for r in reg], [r[2] for r in reg], [is_minus(r[3]) for r in reg])
    cols = [CTX5.index(k.split(">")[0]) for k in fx["nonc"]["columns"]]
    assert np.array_equal(np.array(fx["nonc"]["values"], np.float64), want[:, cols].astype(np.float64))
    assert any(is_minus(r[3]) for r in reg) and not all(is_minus(r[3]) for r in reg)
    assert fx["nonc"]["index"] == ["chr{}:{}-{}".format(r[0], r[1], r[2]) for r in reg]


def test_statement_reproduces_genome_counts(fx):
    seqs = fasta_seqs(fx["fasta"])
    names = list(seqs)
    whole = rule5_regions(seqs, names, [0] * len(names), [len(seqs[n]) for n in names]).sum(axis=0)
    assert fx["genome_counts"]["index"] == CTX5
    assert np.array_equal(np.array(fx["genome_counts"]["values"], np.int64), whole)
    assert (whole > 0).all()


def test_column_orders(fx):
    assert list(st.mk_context_sequences(2, 2).keys()) == CTX5 == fx["by_regions"]["columns"]
    half = list(st.mk_context_sequences(2, 2, collapse=True).keys())
    assert len(half) == 512 and half == fx["by_regions_collapse"]["columns"]
    assert half == [c for c in CTX5 if c[2] in "CT"]
    trans = st.mk_trans_idx(2, 2)
    assert len(trans) == 3072 and trans == sorted(trans) == fx["nonc"]["columns"]
    assert sorted(set(k.split(">")[0] for k in trans)) == CTX5
    assert fx["freq_context"]["index"] == CTX5


def test_train_sequence_model_penta(fx, tmp_path):
    """train_sequence_model(n_up=2) on the reference's annotated mutations and genome counts gives its 3 072 / 1 024 tables
    (regions cover whole chromosomes: the bed whitelist keeps every row, as the golden's identity whitelist does)."""
    seqs = fasta_seqs(fx["fasta"])
    f_mut = tmp_path / "annotated.tsv"
    f_mut.write_text(fx["annotated"])
    df_mut = mutation_tools.read_mutation_file(str(f_mut), drop_duplicates=False)
    regions = np.array([[int(n[3:]), 0, len(s)] for n, s in seqs.items()])
    S = pd.Series(fx["genome_counts"]["values"], index=fx["genome_counts"]["index"])
    df_freq_mut, df_freq_context = st.train_sequence_model(regions, df_mut, S, n_up=2, n_down=2)
    want = fx["freq_mut"]
    assert list(df_freq_mut.columns) == want["columns"]
    assert list(df_freq_mut.MUT_TYPE) == want["MUT_TYPE"] and list(df_freq_mut.CONTEXT) == want["CONTEXT"]
    assert np.array_equal(df_freq_mut.COUNT.to_numpy(float), np.array(want["COUNT"]))
    np.testing.assert_allclose(df_freq_mut.FREQ.to_numpy(float), np.array(want["FREQ"]), rtol=1e-15, atol=0)
    assert list(df_freq_context.columns) == fx["freq_context"]["columns"]
    assert [str(i) for i in df_freq_context.index] == fx["freq_context"]["index"]
    np.testing.assert_allclose(df_freq_context.FREQ.to_numpy(float), np.array(fx["freq_context"]["FREQ"]), rtol=1e-12, atol=0)


def _tiny_genome():
    return PackedGenome.from_sequences({"chr1": "ACGTACGTAC" * 20})


def test_unsupported_pairs_raise_before_any_device_work():
    g = _tiny_genome()
    for up, down in ((1, 2), (2, 1), (3, 3), (0, 0)):
        with pytest.raises(NotImplementedError, match=r"\(1, 1\).*\(2, 2\)"):
            engine.count_contexts(g, ["chr1"], [10], [50], n_up=up, n_down=down, on_device=False)
        with pytest.raises(NotImplementedError):
            st.count_contexts_by_regions(g, ["chr1"], [10], [50], n_up=up, n_down=down)
        with pytest.raises(NotImplementedError):
            st.nonc_elt_context_count([("1", 10, 50, "+")], st.mk_trans_idx(1, 1), g, n_up=up, n_down=down)


def test_start_one_raises_value_error():
    with pytest.raises(ValueError, match="START 1"):
        engine.count_contexts(_tiny_genome(), ["chr1", "chr1"], [0, 1], [50, 50], n_up=2, n_down=2, on_device=False)


def test_cli_refuses_other_pairs(tmp_path):
    fa = tmp_path / "g.fa"
    fa.write_text(">chr1\n" + "ACGT" * 50 + "\n")
    bed = tmp_path / "w.bed"
    bed.write_text("1\t0\t100\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "DigPreprocess.py"), "countGenomeContext", str(fa),
                        str(tmp_path / "out.h5"), "--bed", str(bed), "--up", "3", "--down", "3"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "--up 1 --down 1" in r.stderr and "--up 2 --down 2" in r.stderr
