"""The gene container on the MI355X: dig_gene_site_counts and its `_host` twin against the independent statement
(gene_counts_statement.py), conservation of the sites, the cross-check with the observed side (dig_mutation_function +
dig_mutation_contexts on the full enumeration of possible SNVs), the window counts against the reference's golden, and the chain of
command lines from a FASTA and a bed12 to geneDriver results.  Integers are compared exactly."""
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import gene_counts_statement as GS
import mutfunc_statement as S
from conftest import GOLDEN, ROOT
from digdriver_amd import _lib, engine
from digdriver_amd.data_tools import gene_annotation
from digdriver_amd.data_tools.genome import PackedGenome
from digdriver_amd.io import mapfile
from digdriver_amd.sequence_model import genic_driver_tools, sequence_tools
from test_gene_site_counts_host import golden_container
from test_gpu_host_mirror import _cmp_frame
from test_gpu_mutation_function import fuzz_bed12, fuzz_genome, raw_calls
from test_mutation_function_host import HAND_BED, HAND_SEQ

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def _gpu():
    _lib.require_device()


def load(tmp_path, bed_text, seqs):
    f = tmp_path / "genes.bed"
    f.write_text(bed_text)
    g = PackedGenome.from_sequences(seqs)
    genes, gch = gene_annotation.load_cds_bed12(str(f)).on_genome(g)
    stated = S.parse_bed12(bed_text)
    assert genes.names == [x["name"] for x in stated]
    return g, genes, gch, stated


def genes_at_contig_ends(seqs):
    n1, n2 = len(seqs["chr1"]), len(seqs["chr2"])
    return ("1\t0\t30\tat_start\t0\t+\t0\t30\t0\t2\t9,9,\t0,21,\n"
            "1\t%d\t%d\tat_end\t0\t-\t%d\t%d\t0\t2\t12,9,\t0,31,\n" % (n1 - 40, n1, n1 - 40, n1) +
            "2\t0\t12\tat_start2\t0\t-\t0\t12\t0\t1\t12,\t0,\n"
            "2\t%d\t%d\tnear_end2\t0\t+\t%d\t%d\t0\t1\t15,\t0,\n" % (n2 - 16, n2 - 1, n2 - 16, n2 - 1))


@pytest.fixture(scope="module")
def fuzz(tmp_path_factory):
    rng = np.random.default_rng(11)
    seqs = fuzz_genome(rng, n_runs=12, n_iupac=60)
    bed = fuzz_bed12(rng, seqs, 300) + genes_at_contig_ends(seqs)
    g, genes, gch, stated = load(tmp_path_factory.mktemp("genesites"), bed, seqs)
    want = [GS.gene_counts(seqs, x) for x in stated]
    return dict(seqs=seqs, g=g, genes=genes, gch=gch, stated=stated, L=np.array([w[0] for w in want], np.int32),
                nsl=np.array([w[1] for w in want], np.int32), other=np.array([w[2] for w in want], bool))


def test_kernel_fuzz_against_statement(_gpu, fuzz):
    stated, other = fuzz["stated"], fuzz["other"]
    assert len(stated) == 304 and {x["strand"] for x in stated} == {"+", "-"} and max(len(x["blocks"]) for x in stated) == 12
    assert 0 < other.mean() < 0.5 and other[-4:].tolist() == [True, True, True, False]       # (a gene that ends one base short is whole)
    for on_device in (False, True):
        L, nsl, status = engine.gene_site_counts(fuzz["g"], fuzz["genes"], fuzz["gch"], on_device=on_device, return_status=True)
        assert L.dtype == np.int32 and L.shape == (len(stated), 4, 192) and nsl.dtype == np.int32
        assert np.array_equal(status == engine.GS_HOST, other) and set(status.tolist()) == {engine.GS_OK, engine.GS_HOST}
        bad = np.flatnonzero((L != fuzz["L"]).any(axis=(1, 2)) | (nsl != fuzz["nsl"]))
        assert bad.size == 0, (on_device, [stated[b]["name"] for b in bad[:5]], other[bad[:5]])
    # the raw rows of the genes left to the host are zero
    G = len(stated)
    Lr, nr, st = np.full((G, 4, 192), -1, np.int32), np.full(G, -1, np.int32), np.full(G, 9, np.uint8)
    genes = fuzz["genes"]
    table = (fuzz["gch"], genes.minus, genes.blk_ptr, genes.blk_start, genes.blk_end, genes.cds_off, genes.spl_ptr, genes.spl_pos)
    h = _lib.host_ptr
    _lib.call("dig_gene_site_counts_host", *fuzz["g"].genome2_args(), *[h(a) for a in table], G, h(Lr), h(nr), h(st), 0)
    assert (Lr[other] == 0).all() and (nr[other] == 0).all() and np.array_equal(Lr[~other], fuzz["L"][~other])
    # every class and most columns are exercised
    assert (fuzz["L"].sum(axis=(0, 2)) > 0).all() and fuzz["nsl"].sum() > 0 and (fuzz["L"].sum(axis=0) > 0).mean() > 0.8       # (few types can make a stop)


def test_sites_are_conserved(_gpu, fuzz):
    L, nsl = engine.gene_site_counts(fuzz["g"], fuzz["genes"], fuzz["gch"], on_device=True)
    genes, whole = fuzz["genes"], ~fuzz["other"]
    assert np.array_equal((L[:, :3].sum(axis=(1, 2)) + nsl)[whole], 3 * genes.cds_len[whole])
    assert np.array_equal(L[:, 3].sum(axis=1)[whole], 3 * np.diff(genes.spl_ptr)[whole])
    # a gene with other letters loses exactly the sites the statement skips: never more sites than bases
    assert ((L[:, :3].sum(axis=(1, 2)) + nsl)[~whole] <= 3 * genes.cds_len[~whole]).all()


def test_expected_side_equals_the_observed_side(_gpu, fuzz, tmp_path):
    """Every possible SNV of every CDS and splice position, classified by dig_mutation_function and typed by
    dig_mutation_contexts, tallied per gene: the same [G, 4, 192] as dig_gene_site_counts."""
    stated = fuzz["stated"]
    # genes without other letters, and whose splice positions lie in their introns (an intron shorter than 5 bases puts the
    # donor + 5 into the next exon: the annotation calls such a base a splice site, the counts take it both ways)
    pick = [i for i, x in enumerate(stated) if not fuzz["other"][i]
            and not any(s <= p <= e for p in x["splice"] for s, e in x["blocks"])][:60]
    assert len(pick) == 60 and {stated[i]["strand"] for i in pick} == {"+", "-"}
    sub = fuzz["genes"].subset(np.array(pick))
    gch = fuzz["gch"][pick]
    gene, pos, ref, alt = [], [], [], []
    for k, i in enumerate(pick):
        x = stated[i]
        for p in S.cds_positions(x) + x["splice"]:
            r = "ACGT".index(S.letter(fuzz["seqs"], x["chrom"], p))
            for a in range(4):
                if a != r:
                    gene.append(k), pos.append(p), ref.append(r), alt.append(a)
    n = len(gene)
    gene, pos, ref, alt = np.array(gene, np.int32), np.array(pos, np.int64), np.array(ref, np.uint8), np.array(alt, np.uint8)
    impact, status, _, _, _ = [a.cpu().numpy() for a in engine.mutation_function(fuzz["g"], sub, gch, gene, pos, pos, np.zeros(n, np.uint8), ref, alt)]
    assert (status == engine.MF_OK).all() and n > 100000
    chroms = np.array(fuzz["g"].names, dtype=object)[gch[gene]]
    order = np.lexsort((pos, gch[gene]))                                 # rows in group order: chromosome-grouped
    mc_status, code = engine.mutation_contexts(fuzz["g"], chroms[order], pos[order] - 1, ref[order], n_up=1, n_down=1)
    assert (mc_status.cpu().numpy() == engine.MC_KEPT).all()
    ctx = np.empty(n, np.int64)
    ctx[order] = code.cpu().numpy().astype(np.int64)
    x, y, z = ctx & 3, (ctx >> 2) & 3, (ctx >> 4) & 3                    # window base k in bits 2 k, 2 k + 1
    minus = sub.minus[gene] != 0
    X, Y, Z, A = np.where(minus, 3 - z, x), np.where(minus, 3 - y, y), np.where(minus, 3 - x, z), np.where(minus, 3 - alt, alt)
    assert (y == ref).all()
    col = 3 * (16 * X + 4 * Y + Z) + A - (A > Y)
    cls = np.array([0, 1, 2, -1, 3])[impact]                            # MF_SYN, MF_MIS, MF_NONS, MF_STOP_LOSS, MF_SPLICE
    tally = np.zeros((len(pick), 4, 192), np.int32)
    keep = cls >= 0
    np.add.at(tally, (gene[keep], cls[keep], col[keep]), 1)
    stop_loss = np.bincount(gene[~keep], minlength=len(pick))
    L, nsl = engine.gene_site_counts(fuzz["g"], sub, gch, on_device=True)
    assert np.array_equal(L, tally) and np.array_equal(nsl, stop_loss) and nsl.sum() > 0
    assert np.array_equal(L, fuzz["L"][pick])


def test_hand_made_genes_and_empty_table(_gpu, tmp_path):
    seqs = {"chr1": HAND_SEQ}
    bed = HAND_BED + "1\t18\t31\tsp\t0\t+\t18\t31\t0\t2\t2,1,\t0,12,\n1\t99\t111\tsm\t0\t-\t99\t111\t0\t2\t2,1,\t0,11,\n"
    g, genes, gch, stated = load(tmp_path, bed, seqs)
    for on_device in (False, True):
        L, nsl, status = engine.gene_site_counts(g, genes, gch, on_device=on_device, return_status=True)
        assert (status == engine.GS_OK).all() and nsl.tolist() == [23, 8, 7, 0, 0]
        for k, x in enumerate(stated):
            assert L[k].tolist() == GS.gene_counts(seqs, x)[0], x["name"]
        L0, n0 = engine.gene_site_counts(g, genes.subset(np.zeros(0, np.int64)), gch[:0], on_device=on_device)
        assert L0.shape == (0, 4, 192) and n0.shape == (0,)
    with pytest.raises(ValueError, match="outside the genome"):
        engine.gene_site_counts(g, genes, gch + 1, on_device=False)


def test_window_counts_on_the_device_match_the_reference(_gpu, tmp_path):
    with open(os.path.join(GOLDEN, "si_count_golden.json")) as f:
        g = json.load(f)
    genome, f_genic = golden_container(tmp_path, g)
    for on_device in (False, True):
        frame = sequence_tools.si_count_parallel(f_genic, genome, g["window"], 2, on_device=on_device)
        assert list(frame.columns) == g["keys"] and np.array_equal(frame.values, np.array(g["counts"]))


def test_from_fasta_and_bed12_to_gene_driver_results(_gpu, tmp_path):
    rng = np.random.default_rng(77)
    w = 1000
    seqs = fuzz_genome(rng, sizes=(("chr1", 60000), ("chr2", 40000), ("chrX", 20000)), n_runs=2, n_iupac=4, max_run=200)
    bed = fuzz_bed12(rng, {k: seqs[k] for k in ("chr1", "chr2")}, 50, max_exons=6)
    bed += "X\t100\t160\ton_x\t0\t-\t100\t160\t0\t2\t30,9,\t0,51,\n" "Un\t100\t109\tunplaced\t0\t+\t100\t109\t0\t1\t9,\t0,\n"
    d = tmp_path
    (d / "cds.bed").write_text(bed)
    (d / "genome.fa").write_text("".join(">%s\n%s\n" % (k, v) for k, v in seqs.items()))
    (d / "windows.bed").write_text("".join("%s\t%d\t%d\n" % (c[3:], s, s + w) for c in ("chr1", "chr2") for s in range(0, len(seqs[c]), w)))
    stated = [x for x in S.parse_bed12(bed) if x["chrom"] in ("1", "2")]
    env = dict(os.environ, DIG_CLI_ASSERT_NO_TORCH="1")

    def run(script, *args):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script)] + [str(a) for a in args], capture_output=True, text=True,
                           timeout=900, env=env)
        assert r.returncode == 0, r.stderr
        return r.stdout

    run("DigPreprocess.py", "countGenomeContext", d / "genome.fa", d / "counts.map", "--bed", d / "windows.bed")
    # without a container of genes the command says what is missing
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "DigPreprocess.py"), "preprocess_genic_model", str(d / "genic.map"),
                        str(d / "genome.fa"), str(d / "si.map"), "--window", str(w)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode != 0 and "--cds-bed" in r.stderr and "Traceback" not in r.stderr
    run("DigPreprocess.py", "initialize_f_data", d / "genic.map", d / "counts.map")
    out = run("DigPreprocess.py", "preprocess_genic_model", d / "genic.map", d / "genome.fa", d / "si.map", "--window", w, "--out-key",
              "cds/window_1kb", "--cds-bed", d / "cds.bed", "--n-procs", 3)
    assert "Dropping 1 genes on contigs the FASTA does not hold (or beyond their end): Un" in out and "Note:" not in out
    names = mapfile.read_array(str(d / "genic.map"), "window_%d/genes/names" % w).astype(str).tolist()
    assert names == [x["name"] for x in stated] + ["on_x"]
    L = mapfile.read_array(str(d / "genic.map"), "window_%d/genes/L" % w)
    want_L = np.array([GS.gene_counts(seqs, x)[0] for x in S.parse_bed12(bed) if x["chrom"] != "Un"], np.int32)
    assert np.array_equal(L, want_L)
    si = mapfile.read_frame(str(d / "si.map"), "cds/window_1kb")
    assert list(si.index) == names and list(si.columns) == GS.NAMES
    # a second run without --cds-bed finds the genes and writes the same counts
    run("DigPreprocess.py", "preprocess_genic_model", d / "genic.map", d / "genome.fa", d / "si2.map", "--window", w)
    assert mapfile.read_frame(str(d / "si2.map"), "cds/window_10kb").equals(si)

    # a mutation map over the same windows: synthetic region parameters and sequence model
    idx = mapfile.read_array(str(d / "counts.map"), "idx")
    N = len(idx)
    pre = str(d / "pretrained.map")
    mapfile.write_frame(pre, "region_params", pd.DataFrame(dict(CHROM=idx[:, 0], START=idx[:, 1], END=idx[:, 2], Y_TRUE=rng.poisson(30, N),
                                                                Y_PRED=rng.gamma(9.0, 3.0, N), STD=rng.gamma(4.0, 1.0, N), FLAG=rng.random(N) < 0.05),
                                                           index=["chr{}:{}-{}".format(*r) for r in idx]))
    seq_model = sequence_tools.mk_mutation_context(n_up=1, n_down=1, return_df=True)
    seq_model["FREQ"] = rng.uniform(1e-7, 1e-5, len(seq_model))
    mapfile.write_frame(pre, "sequence_model_192", seq_model)
    mapfile.write_array(pre, "idx", idx.astype(np.int32))
    run("DigPretrain.py", "genicModel", pre, d / "genic.map")
    gm = mapfile.read_frame(pre, "genic_model")
    assert list(gm.GENE) == [x["name"] for x in stated] and list(gm.CHROM) == [x["chrom"] for x in stated]      # on_x is skipped
    # genic_driver_tools.py:114-123,147,158 on the statement's L and the mirror's window counts
    d_pr = genic_driver_tools.sorted_d_pr(seq_model)
    cc = si.loc[gm.GENE].values.astype(np.float64)
    t_pi = d_pr[None, :] / (cc * d_pr[None, :]).sum(axis=1, keepdims=True)
    P = (t_pi[:, None, :] * want_L[:len(stated)]).sum(axis=2)
    glen = np.array([len(S.cds_positions(x)) for x in stated])
    cols = ["P_SILENT", "P_MIS", "P_NONS", "P_SPLICE", "R_SIZE", "GENE_LENGTH"]
    vals = np.column_stack([P[:, 0], P[:, 1], P[:, 2], P[:, 3], (cc.sum(axis=1) / 3).astype(np.int64), glen])
    for c, v in zip(cols, vals.T):
        print(c, "max relative difference", float(np.max(np.abs(gm[c].values.astype(float) - v) / np.maximum(np.abs(v), 1e-300))))
    _cmp_frame(gm, cols, vals)
    assert (gm.P_SILENT > 0).all() and (gm.P_MIS > 0).all()

    # raw calls -> annotated file -> geneDriver on the model just made
    (d / "raw.tsv").write_text(raw_calls(np.random.default_rng(78), seqs, stated, 4000, True, chroms=("1", "2")))
    run("DigPreprocess.py", "annotMutationFile", d / "raw.tsv", d / "genome.fa", d / "annot.tsv", "--cds-bed", d / "cds.bed")
    (d / "genes_CGC_ALL.txt").write_text("\n".join(names[:5]) + "\n")
    run("DigDriver.py", "geneDriver", d / "annot.tsv", pre, "--panel-dir", d, "--outpfx", "cohort", "--outdir", d / "res")
    res = pd.read_csv(d / "res" / "cohort.results.txt", sep="\t", index_col=0)
    assert sorted(res.index) == sorted(x["name"] for x in stated) and "PVAL_MUT_BURDEN" in res.columns
    assert res.OBS_SYN.sum() > 0 and np.isfinite(res.PVAL_MUT_BURDEN).all()
