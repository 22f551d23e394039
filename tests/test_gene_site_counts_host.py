"""The gene container without a GPU: the column rule, the statement of the per-gene counts (gene_counts_statement.py) on hand-worked
cases, preprocess_genic's container with the kernel replaced by the statement (the `counts=` argument), and the window counts of
the genes (si_count_*) against the reference's own si_by_regions (tests/golden/si_count_golden.json) with the context-counting
kernel replaced by a per-base loop (the `count=` argument)."""
import json
import os

import numpy as np

import gene_counts_statement as GS
import mutfunc_statement as S
from conftest import GOLDEN
from digdriver_amd.data_tools.genome import PackedGenome
from digdriver_amd.io import mapfile
from digdriver_amd.sequence_model import sequence_tools
from test_mutation_function_host import HAND_BED, SEQS


def statement_counts(seqs, bed_text):
    """counts= of preprocess_genic from the statement (genes matched by name)."""
    stated = {x["name"]: x for x in S.parse_bed12(bed_text)}

    def counts(genome, genes, gene_chrom):
        got = [GS.gene_counts(seqs, stated[n]) for n in genes.names]
        return np.array([g[0] for g in got], np.int32).reshape(len(got), 4, 192), np.array([g[1] for g in got], np.int32)
    return counts


def loop_counter(genome, chroms, starts, ends, minus):
    """count= of si_by_regions / si_count_*: the reference's fetch and per-position loop on the genome's letters."""
    ctx = list(sequence_tools.mk_context_sequences(1, 1))
    out = np.zeros((len(chroms), 64), np.int64)
    for r, (c, s, e, m) in enumerate(zip(genome.chrom_index(chroms), starts, ends, minus)):
        s = 1 if s == 0 else int(s)
        seq = genome.letters(c, s - 1, min(int(e) + 1, int(genome.lengths[c]))).decode()
        if m:
            seq = sequence_tools.reverse_complement(seq)
        for i in range(1, len(seq) - 1):
            w = seq[i - 1:i + 2]
            if all(x in "ACGT" for x in w):
                out[r, ctx.index(w)] += 1
    return out


def test_column_formula_is_the_sorted_substitution_index():
    keys = sorted(sequence_tools.mk_trans_idx(1, 1))
    assert keys == GS.NAMES and len(keys) == 192
    for x in range(4):
        for y in range(4):
            for z in range(4):
                for a in range(4):
                    if a != y:
                        name = "ACGT"[x] + "ACGT"[y] + "ACGT"[z] + ">" + "ACGT"[x] + "ACGT"[a] + "ACGT"[z]
                        assert keys[3 * (16 * x + 4 * y + z) + a - (a > y)] == name


def as_dict(row):
    return {GS.NAMES[i]: v for i, v in enumerate(row) if v}


def test_statement_on_hand_worked_cases():
    plus3, minus3, single = S.parse_bed12(HAND_BED)
    # `single` (+, 10-18): GCT TGG TAA with the genome's G in front and C behind.
    #   GCT: G (GGC) and C (GCT) change the amino acid whatever the letter; T (CTT): GCN is Ala -> 3 silent
    #   TGG: T (TTG) -> 3 missense; first G (TGG): TAG stop, TCG, TTG; second G (GGT): TGA stop, TGC, TGT
    #   TAA: T (GTA) -> 3 stop losses; A (TAA): TGA stays a stop, 2 losses; A (AAC): TAG stays a stop, 2 losses
    L, stop_loss, other = GS.gene_counts(SEQS, single)
    assert stop_loss == 7 and not other
    assert as_dict(L[0]) == {"CTT>CAT": 1, "CTT>CCT": 1, "CTT>CGT": 1, "TAA>TGA": 1, "AAC>AGC": 1}
    assert as_dict(L[1]) == {"GGC>GAC": 1, "GGC>GCC": 1, "GGC>GTC": 1, "GCT>GAT": 1, "GCT>GGT": 1, "GCT>GTT": 1, "TTG>TAG": 1,
                             "TTG>TCG": 1, "TTG>TGG": 1, "TGG>TCG": 1, "TGG>TTG": 1, "GGT>GCT": 1, "GGT>GTT": 1}
    assert as_dict(L[2]) == {"TGG>TAG": 1, "GGT>GAT": 1} and as_dict(L[3]) == {}
    # + strand, one codon over an intron: 19, 20 | 31 reads CG|G (Arg); the flanks are the genome's neighbours -- 20 is followed
    # by the intron's T (CGT, not CGG), 31 is preceded by the intron's A (AGT)
    #   C (ACG): AGG is Arg -> silent, GGG, TGG missense; G (CGT): CAG, CCG, CTG missense; G (AGT): CGN is Arg -> 3 silent
    # its intron 21-30: donor 21 (GTG), 22 (TGT), 25 (AAG), acceptor 29 (CCA), 30 (CAG)
    sp = S.parse_bed12("1\t18\t31\tsp\t0\t+\t18\t31\t0\t2\t2,1,\t0,12,\n")[0]
    assert S.cds_positions(sp) == [19, 20, 31] and sp["splice"] == [21, 22, 25, 29, 30]
    L, stop_loss, other = GS.gene_counts(SEQS, sp)
    assert stop_loss == 0 and not other and as_dict(L[2]) == {}
    assert as_dict(L[0]) == {"ACG>AAG": 1, "AGT>AAT": 1, "AGT>ACT": 1, "AGT>ATT": 1}
    assert as_dict(L[1]) == {"ACG>AGG": 1, "ACG>ATG": 1, "CGT>CAT": 1, "CGT>CCT": 1, "CGT>CTT": 1}
    assert as_dict(L[3]) == {k + ">" + k[0] + a + k[2]: 1 for k in ("GTG", "TGT", "AAG", "CCA", "CAG") for a in "ACGT" if a != k[1]}
    # - strand, one codon over an intron: 111 | 101, 100 reads (complemented) G|TG (Val); the genome around 111 is A C G -> CGT,
    # around 101 C A C -> GTG, around 100 C C A -> TGG
    #   G (CGT): ATG, CTG, TTG missense; T (GTG): GAG, GCG, GGG missense; G (TGG): GTN is Val -> 3 silent
    sm = S.parse_bed12("1\t99\t111\tsm\t0\t-\t99\t111\t0\t2\t2,1,\t0,11,\n")[0]
    assert S.cds_positions(sm) == [111, 101, 100]
    L, stop_loss, other = GS.gene_counts(SEQS, sm)
    assert stop_loss == 0 and not other and as_dict(L[2]) == {}
    assert as_dict(L[0]) == {"TGG>TAG": 1, "TGG>TCG": 1, "TGG>TTG": 1}
    assert as_dict(L[1]) == {"CGT>CAT": 1, "CGT>CCT": 1, "CGT>CTT": 1, "GTG>GAG": 1, "GTG>GCG": 1, "GTG>GGG": 1}
    # - strand splice sites of that intron (102-110): donor 110, 109, 106 (in front of the right-hand exon), acceptor 102, 103; the
    # genome around 110 is T A C -> GTA
    assert sm["splice"] == [102, 103, 106, 109, 110] and L[3][GS.COLUMN["GTA>GCA"]] == 1 and sum(L[3]) == 15
    # the three-exon genes: every site lands in exactly one place
    for gene in (plus3, minus3):
        L, stop_loss, other = GS.gene_counts(SEQS, gene)
        assert not other and sum(map(sum, L[:3])) + stop_loss == 3 * len(S.cds_positions(gene)) and sum(L[3]) == 3 * len(gene["splice"])
    assert GS.gene_counts(SEQS, plus3)[1] == 23 and GS.gene_counts(SEQS, minus3)[1] == 8     # TAA + TGA + TAG; TAG
    # letters other than ACGT and contig ends: the site is skipped, the codon translates to X (X -> X is silent)
    seqs = {"chr1": "ATGNCTTAA"}
    edge = S.parse_bed12("1\t0\t9\tedge\t0\t+\t0\t9\t0\t1\t9,\t0,\n")[0]
    L, stop_loss, other = GS.gene_counts(seqs, edge)
    # A at 1 has no left neighbour; T (ATG), G (TGN), N (GNC), C (NCT) -> only T at 2 of codon 1 counts; codon 2 is X: T at 6
    # (CTT) silent x 3; TAA: T (TTA) 3 losses, A (TAA) 1 silent + 2 losses, the last A has no right neighbour
    assert other and stop_loss == 5
    assert as_dict(L[0]) == {"CTT>CAT": 1, "CTT>CCT": 1, "CTT>CGT": 1, "TAA>TGA": 1}
    assert as_dict(L[1]) == {"ATG>AAG": 1, "ATG>ACG": 1, "ATG>AGG": 1} and as_dict(L[2]) == {}


def test_preprocess_genic_container(tmp_path, capsys):
    seqs = dict(SEQS, chrX="ACGT" * 30, chrY="TTGCA" * 20, chrUn_gl1="ACGGT" * 20)
    bed = HAND_BED + ("X\t3\t12\tonx\t0\t-\t3\t12\t0\t1\t9,\t0,\n" "chrY\t10\t31\tony\t0\t+\t10\t31\t0\t2\t6,6,\t0,15,\n"
                      "Un_gl1\t3\t12\tunplaced\t0\t+\t3\t12\t0\t1\t9,\t0,\n" "9\t3\t12\tnowhere\t0\t+\t3\t12\t0\t1\t9,\t0,\n"
                      "2\t3\t13\tten\t0\t+\t3\t13\t0\t1\t10,\t0,\n" "2\t20\t29\tontwo\t0\t1\t20\t29\t0\t1\t9,\t0,\n")
    f_bed = tmp_path / "cds.bed"
    f_bed.write_text(bed)
    f_genic = str(tmp_path / "genic.map")
    genes = sequence_tools.preprocess_genic(str(f_bed), PackedGenome.from_sequences(seqs), f_genic, 50, counts=statement_counts(seqs, bed))
    out = capsys.readouterr().out
    assert "Dropping 1 genes whose CDS length is not a multiple of 3" in out
    assert "Dropping 1 genes on contigs the FASTA does not hold (or beyond their end): 9" in out
    assert "Dropping 1 genes on contigs other than the numbered ones, X and Y: Un_gl1" in out
    names = ["plus3", "minus3", "single", "onx", "ony", "ontwo"]
    assert genes.names == names
    rd = lambda k: mapfile.read_array(f_genic, "window_50/genes/" + k)
    assert rd("names").astype(str).tolist() == names and rd("chrom_str").astype(str).tolist() == ["1", "1", "1", "X", "Y", "2"]
    assert rd("chrom").dtype == np.int32 and rd("chrom").tolist()[:3] == [1, 1, 1] and rd("chrom").tolist()[5] == 2
    assert rd("strand").astype(str).tolist() == ["+", "-", "+", "-", "+", "+"]
    assert rd("blk_ptr").tolist() == [0, 3, 6, 7, 8, 10, 11]
    assert rd("blk_start").tolist() == [7, 32, 53, 72, 93, 111, 10, 4, 11, 26, 21]
    assert rd("blk_end").tolist() == [21, 40, 61, 79, 101, 117, 18, 12, 16, 31, 29]
    L, nsl = rd("L"), rd("n_stop_loss")
    assert L.shape == (6, 4, 192) and L.dtype == np.int32 and nsl.dtype == np.int32 and nsl.tolist()[:3] == [23, 8, 7]
    stated = {x["name"]: x for x in S.parse_bed12(bed)}
    for g, n in enumerate(names):
        want = GS.gene_counts(seqs, stated[n])
        assert L[g].tolist() == want[0] and nsl[g] == want[1]
    assert (L[:, :3].sum(axis=(1, 2)) + nsl == 3 * genes.cds_len).all()
    # what genic_model reads: GENE_LENGTH from the closed blocks, X / Y skipped by chrom_str
    from digdriver_amd.sequence_model import genic_driver_tools
    elts = genic_driver_tools._element_set(f_genic, 50, "genes", names=["minus3", "ontwo"])
    assert elts["strand_minus"].tolist() == [1, 0] and elts["L"].shape == (2, 4, 192) and elts["chrom"].tolist() == [1, 2]
    assert (elts["blk_end"] - elts["blk_start"] + 1).sum() == 24 + 9


def golden():
    with open(os.path.join(GOLDEN, "si_count_golden.json")) as f:
        return json.load(f)


def golden_container(tmp_path, g):
    """The genes of the golden as a bed12 and the container preprocess_genic makes of them (L is not looked at here)."""
    rows = []
    for x in g["genes"]:
        s0 = x["blocks"][0][0] - 1
        rows.append("\t".join([x["chrom"], str(s0), str(x["blocks"][-1][1]), x["name"], "0", x["strand"], str(s0), str(x["blocks"][-1][1]), "0",
                               str(len(x["blocks"])), ",".join(str(e - s + 1) for s, e in x["blocks"]), ",".join(str(s - 1 - s0) for s, _ in x["blocks"])]))
    f_bed = tmp_path / "golden.bed"
    f_bed.write_text("\n".join(rows) + "\n")
    f_genic = str(tmp_path / "golden_genic.map")
    zeros = lambda genome, genes, gene_chrom: (np.zeros((len(genes), 4, 192), np.int32), np.zeros(len(genes), np.int32))
    genome = PackedGenome.from_sequences(g["seqs"])
    genes = sequence_tools.preprocess_genic(str(f_bed), genome, f_genic, g["window"], counts=zeros)
    assert genes.names == [x["name"] for x in g["genes"]]                # (CDS lengths are multiples of 3: nothing is dropped)
    return genome, f_genic


def test_window_counts_match_the_reference(tmp_path):
    g = golden()
    genome, f_genic = golden_container(tmp_path, g)
    frame = sequence_tools.si_count_parallel(f_genic, genome, g["window"], 3, count=loop_counter)
    assert list(frame.index) == [x["name"] for x in g["genes"]] and list(frame.columns) == g["keys"] == GS.NAMES
    assert frame.values.dtype.kind == "i" and np.array_equal(frame.values, np.array(g["counts"]))
    # every substitution column holds its context's count; the windows cut off at a contig end and the N runs are in the fixture
    assert (frame.values[:, 0::3] == frame.values[:, 1::3]).all() and (frame.values[:, 0::3] == frame.values[:, 2::3]).all()
    assert frame.loc["last_window_1"].sum() // 3 < 500 - 2 and frame.loc["over_edges"].sum() // 3 < 4 * 500 - 60
    # a subset in the caller's order, and si_by_regions on one gene's windows
    sub = sequence_tools.si_count_pretrain(["on_x", "over_edges"], f_genic, genome, g["window"], count=loop_counter)
    assert np.array_equal(sub.values, frame.loc[["on_x", "over_edges"]].values)
    one = sequence_tools.si_by_regions(genome, g["keys"], ["chr1:0-500", "chr1:500-1000", "chr1:1000-1500", "chr1:1500-2000"], strand=-1,
                                       count=loop_counter)
    assert list(one.index) == g["keys"] and np.array_equal(one[0].values, frame.loc["over_edges"].values)
    plus = sequence_tools.si_by_regions(genome, g["keys"], ["chr1:0-500"], strand="+", count=loop_counter)
    assert np.array_equal(plus[0].values, frame.loc["first_window"].values)


def test_host_finish_of_genes_with_other_letters(tmp_path):
    """What engine.gene_site_counts does with a DIG_GS_HOST gene (from PackedGenome.letters) equals the statement."""
    from digdriver_amd import engine
    from digdriver_amd.data_tools import gene_annotation
    seq = list("ACGTTGCAAGGCTTAACCGGATATCGCGATGCATGCAACCGGTTAGCTAGCTAGGATCCAAGGTT" * 4)
    for p, c in ((12, "N"), (13, "N"), (30, "R"), (70, "Y"), (71, "n"), (100, "M"), (129, "N")):
        seq[p] = c
    seqs = {"chr1": "".join(seq), "chr2": "ATGNCTTAA"}
    bed = ("1\t5\t125\tgp\t0\t+\t5\t125\t0\t2\t45,45,\t0,75,\n1\t8\t128\tgm\t0\t-\t8\t128\t0\t3\t30,30,30,\t0,40,90,\n"
           "2\t0\t9\tedge\t0\t+\t0\t9\t0\t1\t9,\t0,\n2\t0\t9\tedge_minus\t0\t-\t0\t9\t0\t1\t9,\t0,\n")
    f_bed = tmp_path / "n.bed"
    f_bed.write_text(bed)
    genome = PackedGenome.from_sequences(seqs)
    genes, gch = gene_annotation.load_cds_bed12(str(f_bed)).on_genome(genome)
    for g, x in enumerate(S.parse_bed12(bed)):
        want = GS.gene_counts(seqs, x)
        L, nsl = engine._gene_sites_from_letters(genome, genes, gch, g)
        assert want[2] and L.tolist() == want[0] and nsl == want[1], x["name"]
        assert L.sum() > 0
