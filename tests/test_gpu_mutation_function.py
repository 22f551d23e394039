"""addMutationFunction on the MI355X: dig_mutation_function and its `_host` twin, the orchestration and the command lines against
the independent statement of the rule in mutfunc_statement.py (no golden from the reference exists: its R script needs
Bioconductor and refcds_hg19.rda).  Equality is exact everywhere."""
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pandas as pd
import pytest

import mutfunc_statement as S
from conftest import ROOT
from digdriver_amd import _lib, engine
from digdriver_amd.data_tools import gene_annotation, mutation_tools
from digdriver_amd.data_tools.genome import PackedGenome
from test_mutation_function_host import HAND_BED, HAND_SEQ

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def _gpu():
    _lib.require_device()


def fuzz_genome(rng, sizes=(("chr1", 300000), ("chr2", 200000)), n_runs=5, n_iupac=25, max_run=1500):
    seqs = {}
    for name, n in sizes:
        s = rng.choice(np.array(list("ACGT")), n)
        for _ in range(n_runs):
            a = int(rng.integers(0, n - 3000))
            s[a:a + int(rng.integers(1, max_run))] = "N"
        for _ in range(n_iupac):
            s[int(rng.integers(0, n))] = rng.choice(np.array(list("RMYKSW")))
        seqs[name] = "".join(s)
    return seqs


def fuzz_bed12(rng, seqs, n_genes, max_exons=12):
    """Random genes of 1 .. max_exons exons on both strands, anywhere (so they overlap each other), CDS length a multiple of 3."""
    rows = []
    chroms = list(seqs)
    for gi in range(n_genes):
        ch = chroms[int(rng.integers(0, len(chroms)))]
        k = int(rng.integers(1, max_exons + 1))
        sizes = rng.integers(1, 200, k)
        sizes[-1] += (3 - int(sizes.sum()) % 3) % 3
        gaps = rng.integers(2, 400, k - 1)
        starts = np.concatenate([[0], np.cumsum(sizes[:-1] + gaps)]).astype(int)
        span = int(starts[-1] + sizes[-1])
        s0 = int(rng.integers(10, len(seqs[ch]) - span - 10))
        strand = rng.choice(["+", "-", "1", "-1"])
        comma = "," if gi % 2 else ""
        rows.append("\t".join([ch[3:], str(s0), str(s0 + span), "g%d" % gi, "0", strand, str(s0), str(s0 + span), "0", str(k),
                               ",".join(map(str, sizes)) + comma, ",".join(map(str, starts)) + comma]))
    return "\n".join(rows) + "\n"


def load_both(tmp_path, bed_text, seqs):
    f = tmp_path / "genes.bed"
    f.write_text(bed_text)
    g = PackedGenome.from_sequences(seqs)
    genes, gch = gene_annotation.load_cds_bed12(str(f)).on_genome(g)
    stated = S.parse_bed12(bed_text)
    assert genes.names == [x["name"] for x in stated]
    return g, genes, gch, stated


def run_both(g, genes, gch, pairs):
    host = engine.mutation_function(g, genes, gch, *pairs, on_device=False)
    dev = engine.mutation_function(g, genes, gch, *pairs, on_device=True)
    for a, b in zip(host, dev):
        assert np.array_equal(a, b.cpu().numpy())
    return host


def test_kernel_fuzz_against_statement(_gpu, tmp_path):
    rng = np.random.default_rng(5)
    seqs = fuzz_genome(rng)
    g, genes, gch, stated = load_both(tmp_path, fuzz_bed12(rng, seqs, 400), seqs)
    assert len(stated) == 400 and {x["strand"] for x in stated} == {"+", "-"}
    n = 200000
    gene = rng.integers(0, len(stated), n)
    start, end = np.empty(n, np.int64), np.empty(n, np.int64)
    kind, ref, alt = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    want = []
    for i in range(n):
        x = stated[gene[i]]
        u = rng.random()
        if u < 0.9:                                                     # an SNV on a CDS base or a splice position of the gene
            if x["splice"] and rng.random() < 0.08:
                p = x["splice"][int(rng.integers(0, len(x["splice"])))]
            else:
                cds = S.cds_positions(x)
                p = cds[int(rng.integers(0, len(cds)))]
            base = S.letter(seqs, x["chrom"], p)
            r = "ACGT".index(base) if base in "ACGT" and rng.random() < 0.95 else int(rng.integers(0, 4))
            a = (r + int(rng.integers(1, 4))) % 4
            start[i] = end[i] = p
            ref[i], alt[i] = r, a
            want.append(S.pair_outputs(seqs, x, p, p, 0, "ACGT"[r], "ACGT"[a]))
        else:                                                           # an indel / MNV around the gene
            lo, hi = x["blocks"][0][0], x["blocks"][-1][1]
            p = int(rng.integers(lo - 5, hi + 5))
            q = p + int(rng.choice([0, 0, 1, 2, 3, 7, 30, 400]))
            kind[i] = 1 + int(rng.integers(0, 2))
            start[i], end[i] = p, q
            want.append(S.pair_outputs(seqs, x, p, q, int(kind[i]), "", ""))
    want = np.array(want, np.int64)
    got = run_both(g, genes, gch, (gene.astype(np.int32), start, end, kind, ref, alt))
    for k, name in enumerate(("impact", "status", "n_cds", "cds_min", "cds_max")):
        bad = np.flatnonzero(got[k].astype(np.int64) != want[:, k])
        assert bad.size == 0, (name, bad[:5], got[k][bad[:5]], want[bad[:5], k])
    snv = kind == 0
    assert (want[snv, 1] == S.HOST).mean() <= 0.05 and (want[snv, 1] == S.HOST).sum() > 0
    assert (want[snv, 1] == S.WRONG_REF).sum() > 0
    assert set(want[snv, 0]) == {0, 1, 2, 3, 4, 255} and ((want[:, 0] == 255) == (~snv | (want[:, 1] == S.HOST))).all()
    # every codon position on both strands, all 64 codons
    seen, codons = set(), set()
    for i in np.flatnonzero(snv & (want[:, 2] == 1))[:60000]:
        x = stated[gene[i]]
        cds = S.cds_positions(x)
        pi = int(want[i, 3])
        k = -(-pi // 3)
        cod = "".join(S.letter(seqs, x["chrom"], cds[t - 1]) for t in (3 * k - 2, 3 * k - 1, 3 * k))
        seen.add((x["strand"], pi - 3 * (k - 1)))
        codons.add("".join(S.COMP.get(c, c) for c in cod) if x["strand"] == "-" else cod)
    assert seen == {(s, k) for s in "+-" for k in (1, 2, 3)}
    assert len({c for c in codons if set(c) <= set("ACGT")}) == 64
    assert set(want[~snv, 2] > 0) == {True, False}


def test_pairs_left_to_the_host(_gpu, tmp_path):
    """Codons that touch N and IUPAC letters come back DIG_MF_HOST and are finished from the letters."""
    seq = list("ACGTTGCAAGGCTTAACCGGATATCGCGATGCATGCAACCGGTTAGCTAGCTAGGATCCAAGGTT" * 4)
    for p, c in ((12, "N"), (13, "N"), (30, "R"), (70, "Y"), (71, "N"), (100, "M")):
        seq[p] = c
    seqs = {"chr1": "".join(seq)}
    bed = "1\t5\t125\tgp\t0\t+\t5\t125\t0\t2\t45,45,\t0,75,\n1\t8\t128\tgm\t0\t-\t8\t128\t0\t3\t30,30,30,\t0,40,90,\n"
    g, genes, gch, stated = load_both(tmp_path, bed, seqs)
    gene, pos, ref, alt, want = [], [], [], [], []
    for gi, x in enumerate(stated):
        for p in S.cds_positions(x) + x["splice"]:
            for a in range(4):
                base = S.letter(seqs, "1", p)
                r = "ACGT".index(base) if base in "ACGT" else 1
                if a == r:
                    continue
                gene.append(gi), pos.append(p), ref.append(r), alt.append(a)
                want.append(S.snv_function(seqs, x, p, "ACGT"[r], "ACGT"[a]))
    n = len(gene)
    pairs = (np.array(gene, np.int32), np.array(pos, np.int64), np.array(pos, np.int64), np.zeros(n, np.uint8),
             np.array(ref, np.uint8), np.array(alt, np.uint8))
    got = run_both(g, genes, gch, pairs)
    host = np.array([w[2] for w in want])
    assert 10 < host.sum() < n and np.array_equal(got[1] == engine.MF_HOST, host)
    for on_device in (False, True):
        impact, wrong, _, _, _ = mutation_tools.classify_pairs_on_gpu(g, genes, gch, *pairs, on_device=on_device)
        assert [mutation_tools._MF_LABEL[i] for i in impact] == [w[0] for w in want]
        assert wrong.tolist() == [w[1] for w in want]
    assert {w[0] for w, h in zip(want, host) if h} >= {"Synonymous", "Missense"}     # X -> X and X -> an amino acid


def test_exhaustive_small_genes(_gpu, tmp_path):
    seqs = {"chr1": HAND_SEQ}
    g, genes, gch, stated = load_both(tmp_path, HAND_BED, seqs)
    gene, pos, ref, alt, want = [], [], [], [], []
    for gi, x in enumerate(stated):
        for p in range(x["blocks"][0][0], x["blocks"][-1][1] + 1):
            if p not in S.cds_positions(x) and p not in x["splice"]:
                continue
            for a in "ACGT":
                r = S.letter(seqs, "1", p)
                if a != r:
                    gene.append(gi), pos.append(p), ref.append("ACGT".index(r)), alt.append("ACGT".index(a))
                    want.append(S.pair_outputs(seqs, x, p, p, 0, r, a))
    n = len(gene)
    got = run_both(g, genes, gch, (np.array(gene, np.int32), np.array(pos, np.int64), np.array(pos, np.int64), np.zeros(n, np.uint8),
                                   np.array(ref, np.uint8), np.array(alt, np.uint8)))
    want = np.array(want)
    for k in range(5):
        assert np.array_equal(got[k].astype(np.int64), want[:, k]), k
    assert Counter(got[0].tolist()) == Counter(want[:, 0].tolist()) and set(got[0].tolist()) == {0, 1, 2, 3, 4}
    assert (got[1] == engine.MF_OK).all()
    # spans of every interval of up to 12 bases around the three-exon genes, as insertion and as deletion / MNV
    gene, st, en, kd, want = [], [], [], [], []
    for gi, x in enumerate(stated):
        for p in range(x["blocks"][0][0] - 3, x["blocks"][-1][1] + 3):
            for ln in (1, 2, 3, 5, 12):
                for k in (1, 2):
                    gene.append(gi), st.append(p), en.append(p + ln - 1), kd.append(k)
                    want.append(S.pair_outputs(seqs, x, p, p + ln - 1, k, "", ""))
    n = len(gene)
    got = run_both(g, genes, gch, (np.array(gene, np.int32), np.array(st, np.int64), np.array(en, np.int64), np.array(kd, np.uint8),
                                   np.zeros(n, np.uint8), np.zeros(n, np.uint8)))
    want = np.array(want)
    for k in range(5):
        assert np.array_equal(got[k].astype(np.int64), want[:, k]), k


def raw_calls(rng, seqs, stated, n, six_columns, chroms=("1", "2", "3")):
    """A raw call file: SNVs on and off the genes, indels of every kind, duplicates, REF == ALT rows, an empty field."""
    lines = []
    for i in range(n):
        u = rng.random()
        if u < 0.55 and stated:
            x = stated[int(rng.integers(0, len(stated)))]
            ch = x["chrom"]
            lo, hi = x["blocks"][0][0], x["blocks"][-1][1]
            p = int(rng.integers(max(lo - 8, 2), hi + 8))
        else:
            ch = chroms[int(rng.integers(0, len(chroms)))]
            p = int(rng.integers(2, len(seqs["chr" + ch]) - 50))
        base = S.letter(seqs, ch, p)
        v = rng.random()
        if v < 0.7:
            r = base if base in "ACGT" and rng.random() < 0.98 else "ACGT"[int(rng.integers(0, 4))]
            a = "ACGT"[int(rng.integers(0, 4))]                         # (sometimes REF == ALT: dropped)
        elif v < 0.76:
            r, a = base, base + "".join(rng.choice(list("ACGT"), int(rng.integers(1, 5))))          # insertion
        elif v < 0.8:
            r = seqs["chr" + ch][p - 1:p + 1]                                                            # insertion behind two bases
            a = r + "".join(rng.choice(list("ACGT"), 3))
        elif v < 0.9:
            k = int(rng.integers(1, 9))
            r, a = seqs["chr" + ch][p - 1:p + k], base                                                   # deletion from the base in front
        elif v < 0.94:
            r, a = seqs["chr" + ch][p - 1:p + int(rng.integers(0, 4))], "-"                              # deletion with a dash
        elif v < 0.97:
            r, a = "-", "".join(rng.choice(list("ACGT"), int(rng.integers(1, 4))))                   # insertion with a dash
        else:
            r, a = "AC", "GT"                                                                            # MNV
        sample = "S%d" % int(rng.integers(0, 6))
        lines.append("\t".join([ch, str(p - 1), str(p - 1 + len(r)), r, a, sample, "extra"] if six_columns else [ch, str(p), r, a, sample]))
        if rng.random() < 0.05:
            lines.append(lines[-1])                                     # an exact duplicate
    if not six_columns:
        lines.insert(len(lines) // 2, "1\t500\t\tA\tS1")                # an empty field
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    d = tmp_path_factory.mktemp("mutfunc")
    rng = np.random.default_rng(23)
    seqs = fuzz_genome(rng, sizes=(("chr1", 60000), ("chr2", 40000), ("chr3", 20000)), n_runs=1, n_iupac=6, max_run=300)
    bed = fuzz_bed12(rng, {k: seqs[k] for k in ("chr1", "chr2")}, 60, max_exons=8)
    bed += "7\t100\t109\tno_contig\t0\t+\t100\t109\t0\t1\t9,\t0,\n"     # a gene on a contig the FASTA does not hold
    bed += "1\t100\t110\tnot_codons\t0\t+\t100\t110\t0\t1\t10,\t0,\n"   # CDS length 10
    f_bed, f_fa = d / "cds.bed", d / "genome.fa"
    f_bed.write_text(bed)
    f_fa.write_text("".join(">%s\n%s\n" % (k, v) for k, v in seqs.items()))
    stated = [x for x in S.parse_bed12(bed) if x["chrom"] in ("1", "2")]
    return dict(dir=d, seqs=seqs, f_bed=str(f_bed), f_fa=str(f_fa), stated=stated)


@pytest.mark.parametrize("six_columns", [False, True])
def test_annotation_end_to_end(_gpu, world, six_columns):
    text = raw_calls(np.random.default_rng(31 + six_columns), world["seqs"], world["stated"], 6000, six_columns)
    f_mut = world["dir"] / ("raw%d.tsv" % six_columns)
    f_mut.write_text(text)
    want, wrong_n = S.annotate(text, world["stated"], world["seqs"])
    assert wrong_n > 0 and want.count("\n") > 5000
    for label in ("Synonymous", "Missense", "Nonsense", "Essential_Splice", "Noncoding\n", "Noncoding_INDEL", "cds_INDEL", "_mnv",
                  "insfrshift", "insinframe", "delfrshift", "delinframe"):
        assert label in want, label
    for on_device in (False, True):
        f_out = str(world["dir"] / "annot.tsv")
        counts = mutation_tools.annotate_mutation_function(str(f_mut), f_out, world["f_bed"], world["f_fa"], on_device=on_device)
        with open(f_out) as f:
            assert f.read() == want
        assert counts["wrong_ref"] == wrong_n and counts["n_rows"] == want.count("\n")
    # the 10 % rule: a genome of another assembly
    other = {k: v[::-1] for k, v in world["seqs"].items()}
    with pytest.raises(ValueError, match="wrong assembly"):
        S.annotate(text, world["stated"], other)
    with pytest.raises(ValueError, match="wrong assembly"):
        mutation_tools.annotate_mutation_function(str(f_mut), str(world["dir"] / "x.tsv"), world["f_bed"], PackedGenome.from_sequences(other),
                                                  on_device=False)


def test_command_lines(_gpu, world):
    from digdriver_amd.driver_model import transfer_tools
    text = raw_calls(np.random.default_rng(37), world["seqs"], world["stated"], 5000, True)
    d = world["dir"]
    f_mut = d / "cli_raw.tsv"
    f_mut.write_text(text)
    script = os.path.join(ROOT, "scripts", "DigPreprocess.py")
    env = dict(os.environ, DIG_CLI_ASSERT_NO_TORCH="1")

    def run(*args):
        r = subprocess.run([sys.executable, script] + [str(a) for a in args], capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0, r.stderr
        return r.stdout

    out = run("addMutationFunction", f_mut, str(d / "step1.tsv") + ".gz", "--cds-bed", world["f_bed"], "--fasta", world["f_fa"])
    assert "Dropping 1 genes on contigs the FASTA does not hold (or beyond their end): 7" in out
    assert "Dropping 1 genes whose CDS length is not a multiple of 3" in out and not os.path.exists(str(d / "step1.tsv") + ".gz")
    want, _ = S.annotate(text, world["stated"], world["seqs"])
    assert (d / "step1.tsv").read_text() == want
    run("addMutationContext", d / "step1.tsv", world["f_fa"], d / "step2.tsv")
    run("annotMutationFile", f_mut, world["f_fa"], d / "both.tsv", "--cds-bed", world["f_bed"], "--n-procs", "3")
    assert (d / "both.tsv").read_bytes() == (d / "step2.tsv").read_bytes()
    df = mutation_tools.read_mutation_file(str(d / "both.tsv"))
    assert list(df.columns) == mutation_tools._MUT_COLS[10] and len(df) > 3000
    table = mutation_tools.mutations_per_gene(transfer_tools.read_mutations_cds(str(d / "both.tsv")))
    # What the statement predicts per gene and class, with the context step and the reader stated here by hand: every coding SNV
    # row of step 1 has the genome's base as REF (the others were left out), so the context step keeps it unless its
    # trinucleotide window START - 1 .. START + 1 holds an N; indel and MNV rows all become ANNOT "INDEL", and
    # read_mutation_file keeps one such row per (CHROM, START, END, REF, ALT, GENE) whatever the sample.
    predicted, indels, dropped_n = Counter(), set(), 0
    for line in want.splitlines():
        c = line.split("\t")
        if c[6] == ".":
            continue
        if "INDEL" in c[7]:
            indels.add((c[0], c[1], c[2], c[3], c[4], c[6]))
        elif "N" in world["seqs"]["chr" + c[0]][int(c[1]) - 1:int(c[1]) + 2].upper():
            dropped_n += 1
        else:
            predicted[(c[6], c[7])] += 1
    for key in indels:
        predicted[(key[5], "INDEL")] += 1
    cols = {"Missense": "OBS_MIS", "Nonsense": "OBS_NONS", "Synonymous": "OBS_SYN", "Essential_Splice": "OBS_SPL", "INDEL": "OBS_INDEL"}
    print("predicted rows", sum(predicted.values()), "table", int(table.to_numpy().sum()), "SNV rows next to an N", dropped_n)
    assert sum(predicted.values()) > 1000
    for (gname, cls), k in predicted.items():
        assert int(table.loc[gname, cols.get(cls, cls)]) == k, (gname, cls)
    assert int(table.to_numpy().sum()) == sum(predicted.values())
    # ... and geneDriver runs on the annotated file: the chain raw calls -> results.txt with nothing from outside the repository
    # (a synthetic gene model over the same genes; the observed counts of the results are the predicted ones)
    from digdriver_amd.io import mapfile
    rng = np.random.default_rng(41)
    names = [x["name"] for x in world["stated"]]
    G = len(names)
    mu = rng.gamma(9.0, 3.0, G)
    frame = pd.DataFrame(dict(CHROM=[x["chrom"] for x in world["stated"]], GENE=names,
                              GENE_LENGTH=[len(S.cds_positions(x)) for x in world["stated"]], R_SIZE=40000, R_OBS=rng.poisson(mu * 8),
                              R_INDEL=rng.poisson(mu), MU=mu, SIGMA=rng.gamma(4.0, 1.0, G), MU_INDEL=mu, SIGMA_INDEL=rng.gamma(4.0, 1.0, G),
                              FLAG=0, P_MIS=rng.uniform(1e-3, 1e-2, G), P_NONS=rng.uniform(1e-4, 1e-3, G), P_SILENT=rng.uniform(1e-3, 1e-2, G),
                              P_SPLICE=rng.uniform(1e-4, 1e-3, G), P_TRUNC=rng.uniform(1e-3, 2e-3, G), P_INDEL=rng.uniform(1e-4, 1e-3, G)))
    model = str(d / "genes.map")
    mapfile.write_frame(model, "genic_model", frame)
    (d / "genes_CGC_ALL.txt").write_text("\n".join(names[:5]) + "\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "DigDriver.py"), "geneDriver", str(d / "both.tsv"), model,
                        "--panel-dir", str(d), "--outpfx", "cohort", "--outdir", str(d / "res")], capture_output=True, text=True,
                       timeout=900, env=env)
    assert r.returncode == 0, r.stderr
    res = pd.read_csv(d / "res" / "cohort.results.txt", sep="\t", index_col=0)
    assert sorted(res.index) == sorted(names) and "PVAL_MUT_BURDEN" in res.columns
    for cls, col in cols.items():
        assert res[col].to_dict() == {n: predicted.get((n, cls), 0) for n in names}, col
    # a wrong assembly ends the command with a message, not a traceback
    rev = d / "rev.fa"
    rev.write_text("".join(">%s\n%s\n" % (k, v[::-1]) for k, v in world["seqs"].items()))
    r = subprocess.run([sys.executable, script, "addMutationFunction", str(f_mut), str(d / "bad.tsv"), "--cds-bed", world["f_bed"],
                        "--fasta", str(rev)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode != 0 and "wrong assembly" in r.stderr and "Traceback" not in r.stderr
