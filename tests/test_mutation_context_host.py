"""addMutationContext without a GPU: the native reader's fallback decision and its arrays against pandas, the native writer
against the golden bytes (contexts from a plain-Python statement of the reference's per-row rule), command-line errors."""
import ctypes
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from digdriver_amd import _lib
from digdriver_amd.data_tools import mutation_tools

_COMP = str.maketrans('NTCGA', 'NAGCT')


def load_fixture():
    with gzip.open(os.path.join(GOLDEN, "mutation_context_golden.json.gz"), "rt") as f:
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


def rule3(seq, starts, refs, n_up, n_down, collapse=False):
    """The reference's per-row rule for the rows of one chromosome, in order: seq[START] == REF, the run copy, the window with
    Python slice semantics, '' for a window holding N, the reverse complement of a G / A centre under collapse."""
    seq = seq.upper()
    out, prev_start, prev_ctx = [], None, None
    for s, r in zip(starts, refs):
        if s >= len(seq):
            raise IndexError(s)
        if seq[s] != r:
            ctx = ""
        elif s == prev_start:
            ctx = prev_ctx
        else:
            w = seq[s - n_up:s + n_down + 1]
            ctx = "" if "N" in w else (w[::-1].translate(_COMP) if collapse and w[n_up] in "GA" else w)
        out.append(ctx)
        prev_start, prev_ctx = s, ctx
    return out


def write_file(tmp_path, name, text):
    p = str(tmp_path / name)
    with open(p, "w") as f:
        f.write(text)
    return p


def native_parse(path):
    h, ns, ni = ctypes.c_void_p(), ctypes.c_int64(-1), ctypes.c_int64(0)
    _lib.call("dig_mutctx_file_parse_host", path.encode(), ctypes.byref(h), ctypes.byref(ns), ctypes.byref(ni))
    return h, ns.value, ni.value


def native_rows(path):
    h, ns, ni = native_parse(path)
    if ns < 0:
        return None
    try:
        chrom, start, ref = np.empty(ns, np.int32), np.empty(ns, np.int64), np.empty(ns, np.uint8)
        _lib.call("dig_mutctx_file_fetch_host", h, _lib.host_ptr(chrom), _lib.host_ptr(start), _lib.host_ptr(ref))
    finally:
        _lib.call("dig_mutctx_file_free_host", h)
    return chrom, start, ref, ni


def pandas_branches(path):
    df = mutation_tools.read_mutation_file(path, drop_duplicates=False)
    is_indel = df.ANNOT.str.contains('INDEL')
    snv = df[~is_indel]
    snv = snv.iloc[np.argsort(snv.CHROM.to_numpy(), kind='stable')]
    return snv, int(is_indel.sum())


def test_native_reader_takes_what_pandas_echoes(tmp_path):
    fx = load_fixture()
    for name, text in fx["inputs"].items():
        path = write_file(tmp_path, name + ".tsv", text)
        got = native_rows(path)
        if name == "nan_genes":                                   # NA / empty / nan / NULL labels: pandas rewrites them
            assert got is None
            continue
        chrom, start, ref, n_indel = got
        snv, want_indel = pandas_branches(path)
        assert n_indel == want_indel
        assert np.array_equal(chrom, snv.CHROM.to_numpy()) and np.array_equal(start, snv.START.to_numpy())
        codes = snv.REF.map(lambda r: "ACGT".index(r) if r in ("A", "C", "G", "T") else ord(r) if len(r) == 1 else 255)
        codes = codes.to_numpy(np.uint8)
        assert np.array_equal(ref, codes)


@pytest.mark.parametrize("text", [
    "1\t10\t11\tA\tT\tS1\tG1\t\"Missense\"\n",                 # quoting
    "1\t10\t11\tA\tT\tS1\tG1\tMissense\r\n",                    # CR
    "1\t010\t11\tA\tT\tS1\tG1\tMissense\n",                     # START not canonical
    "1\t10\t11.0\tA\tT\tS1\tG1\tMissense\n",                    # END not an integer
    "1\t10\t11\tA\tT\tS1\tG1\tMissense\n\n1\t12\t13\tA\tT\tS1\tG1\tMissense\n",     # empty line
    "1\t10\t11\tA\tT\tS1\tG1\tMissense\n1\t12\t13\tA\tT\tS1\tG1\n",                 # ragged
    "1\t10\t11\tA\tT\tS1\tNA\tMissense\n",                      # NaN spelling
    "1\t10\t11\tA\tT\tS\xe9\tG1\tMissense\n",                   # non-ASCII
])
def test_native_reader_falls_back(tmp_path, text):
    assert native_parse(write_file(tmp_path, "m.tsv", text))[1] == -1


def test_native_writer_gives_golden_bytes(tmp_path):
    """status / context as the kernel reports them, from rule3: full ACGT windows as codes (DIG_MC_KEPT), every other kept
    context as host text (DIG_MC_HOST), dropped rows as DIG_MC_MISMATCH -- the writer's bytes are the reference's."""
    fx = load_fixture()
    seqs = fasta_seqs(fx["fasta"])
    n_cases = 0
    for case in fx["cases"]:
        if case["collapse"] or case["input"] == "nan_genes":
            continue
        n_up, n_down = case["n_up"], case["n_down"]
        W = n_up + n_down + 1
        path = write_file(tmp_path, case["input"] + ".tsv", fx["inputs"][case["input"]])
        snv, _ = pandas_branches(path)
        ctx = []
        for c in snv.CHROM.unique():
            part = snv[snv.CHROM == c]
            ctx += rule3(seqs["chr%d" % c], part.START.tolist(), part.REF.tolist(), n_up, n_down)
        status = np.full(len(ctx), 1, np.uint8)
        code = np.zeros(len(ctx), np.uint32)
        host = []
        for k, s in enumerate(ctx):
            if len(s) == W and set(s) <= set("ACGT"):
                status[k] = 0
                code[k] = sum("ACGT".index(b) << (2 * j) for j, b in enumerate(s))
            elif s:
                status[k] = 3
                host.append(s)
        off = np.zeros(len(host) + 1, np.int64)
        np.cumsum([len(s) for s in host], out=off[1:])
        out = str(tmp_path / "out.tsv")
        h, ns, _ = native_parse(path)
        assert ns == len(ctx)
        try:
            _lib.call("dig_mutctx_file_write_host", h, out.encode(), _lib.host_ptr(status), _lib.host_ptr(code),
                      "".join(host).encode(), _lib.host_ptr(off), n_up, n_down)
        finally:
            _lib.call("dig_mutctx_file_free_host", h)
        with open(out) as f:
            assert f.read() == case["expected"], (case["input"], n_up, n_down)
        n_cases += 1
    assert n_cases >= 7


def _cli(*args, cwd=None):
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "DigPreprocess.py"), "addMutationContext"] + list(args),
                          capture_output=True, text=True, cwd=cwd, timeout=300)


def test_cli_argument_errors(tmp_path):
    fx = load_fixture()
    fa = write_file(tmp_path, "g.fa", fx["fasta"])
    good = write_file(tmp_path, "m.tsv", fx["inputs"]["plain"])
    r = _cli(good, fa)                                            # fout missing
    assert r.returncode == 2 and "fout" in r.stderr
    r = _cli(good, fa, str(tmp_path / "o.tsv"), "--up", "x")
    assert r.returncode == 2 and "--up" in r.stderr
    r = _cli(good, fa, str(tmp_path / "o.tsv"), "--up", "8", "--down", "8")
    assert r.returncode != 0 and "16" in r.stderr
    seven = write_file(tmp_path, "m7.tsv", "1\t10\t11\tA\tT\tS1\tMissense\n")
    r = _cli(seven, fa, str(tmp_path / "o.tsv"))
    assert r.returncode != 0 and "8-column" in r.stderr
    none_left = write_file(tmp_path, "mx.tsv", "X\t10\t11\tA\tT\tS1\tG1\tMissense\nchr1\t10\t11\tA\tT\tS1\tG1\tINDEL\n")
    r = _cli(none_left, fa, str(tmp_path / "o.tsv"))
    assert r.returncode != 0 and "no mutation left" in r.stderr
    assert not os.path.exists(str(tmp_path / "o.tsv"))


def test_packed_genome_side_table(tmp_path):
    from digdriver_amd.data_tools.genome import PackedGenome
    fx = load_fixture()
    seqs = fasta_seqs(fx["fasta"])
    fa = write_file(tmp_path, "g.fa", fx["fasta"])
    for attempt in range(2):                                      # packed, then from the cache
        g = PackedGenome.from_fasta(fa)
        for i, n in enumerate(g.names):
            assert g.letters(i, 0, len(seqs[n])).decode() == seqs[n].upper()
    d = dict(np.load(fa + ".dig4.npz"))                           # a cache without the table is repacked
    np.savez(fa + ".dig4.npz", **{k: v for k, v in d.items() if not k.startswith("other")})
    g = PackedGenome.from_fasta(fa)
    assert g.letters(0, 0, 50).decode() == seqs[g.names[0]][:50].upper()
    assert "other_pos" in np.load(fa + ".dig4.npz").files
