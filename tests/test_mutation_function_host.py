"""addMutationFunction without a GPU: the gene table from a bed12 file, the statement of the rule (mutfunc_statement.py) on
hand-worked cases, and the product's host code (reading, de-duplication, row order, labels, the 10 % rule) with its two GPU steps
-- the join and the per-pair kernel -- replaced by the statement through the `join=` / `classify=` arguments."""
import os

import numpy as np
import pytest

import mutfunc_statement as S
from conftest import GOLDEN
from digdriver_amd.data_tools import gene_annotation, mutation_tools

# chr1, 1-based.  plus3 (+): exons 7-21, 32-40, 53-61: ATG GCT TGG TAA CGT | TAT TGC TGA | CCC AAA TAG;
# minus3 (-): exons 72-79, 93-101, 111-117, read from 117 downwards: ATG CCC G|TG GCT GAA T|GT AAA TAG; single (+): 10-18 inside plus3
HAND_SEQ = ("TTGACC" "ATGGCTTGGTAACGT" "GTAAGTCCAG" "TATTGCTGA" "GTGAGTTTTCAG" "CCCAAATAG" "TTTTTTTTTT"
            "CTATTTACC" "CTGAAAACTCAC" "ATTCAGCCA" "CTGGACTTAC" "GGGCAT" "AACCAACC")
HAND_BED = ("1\t6\t61\tplus3\t0\t+\t6\t61\t0\t3\t15,9,9,\t0,25,46,\n"
            "1\t71\t117\tminus3\t0\t-1\t71\t117\t0\t3\t8,9,7\t0,21,39\n"
            "1\t9\t18\tsingle\t0\t1\t9\t18\t0\t1\t9,\t0,\n")
SEQS = {"chr1": HAND_SEQ, "chr2": "ACGT" * 30}


def write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_hand_made_gene_table(tmp_path):
    genes = gene_annotation.load_cds_bed12(write(tmp_path, "hand.bed", HAND_BED))
    assert genes.names == ["plus3", "minus3", "single"] and genes.chrom.tolist() == ["1", "1", "1"]
    assert genes.minus.tolist() == [0, 1, 0]
    assert genes.blk_ptr.tolist() == [0, 3, 6, 7]
    assert genes.blk_start.tolist() == [7, 32, 53, 72, 93, 111, 10]
    assert genes.blk_end.tolist() == [21, 40, 61, 79, 101, 117, 18]
    assert genes.cds_off.tolist() == [0, 15, 24, 0, 8, 17, 0]
    assert genes.cds_len.tolist() == [33, 24, 9]
    # + gene: donor end + 1, + 2, + 5 and acceptor start - 1, - 2 of each intron
    assert genes.spl_pos[genes.spl_ptr[0]:genes.spl_ptr[1]].tolist() == [22, 23, 26, 30, 31, 41, 42, 45, 51, 52]
    # - gene: mirrored -- the donor lies in front of the right-hand exon (start - 1, - 2, - 5), the acceptor behind the left-hand one
    assert genes.spl_pos[genes.spl_ptr[1]:genes.spl_ptr[2]].tolist() == [80, 81, 88, 91, 92, 102, 103, 106, 109, 110]
    assert genes.spl_ptr.tolist() == [0, 10, 20, 20]
    # the statement's table is the same one
    stated = S.parse_bed12(HAND_BED)
    assert [x["splice"] for x in stated] == [genes.spl_pos[genes.spl_ptr[g]:genes.spl_ptr[g + 1]].tolist() for g in range(3)]
    assert [x["blocks"] for x in stated] == [list(zip(genes.blk_start[a:b].tolist(), genes.blk_end[a:b].tolist()))
                                             for a, b in zip(genes.blk_ptr[:-1], genes.blk_ptr[1:])]
    # the ranges handed to the join: blocks and one-base splice intervals, sorted by (chrom, start), with their gene
    chrom, start, end, gene = genes.ranges()
    assert len(start) == 7 + 20 and (np.diff(start) >= 0).all() and set(chrom) == {"1"}
    assert sorted(zip(start.tolist(), end.tolist(), gene.tolist()))[:4] == [(7, 21, 0), (10, 18, 2), (22, 22, 0), (23, 23, 0)]
    other = gene_annotation.load_cds_bed12(write(tmp_path, "hand.bed", HAND_BED), splice_offsets={"donor": (1,), "acceptor": (-1,)})
    assert other.spl_pos[:4].tolist() == [22, 31, 41, 52]


def test_gene_table_rules(tmp_path, capsys):
    row = "1\t100\t%d\t%s\t0\t+\t100\t110\t0\t1\t%d,\t0,\n"
    genes = gene_annotation.load_cds_bed12(write(tmp_path, "a.bed", row % (109, "ok", 9) + row % (110, "ten", 10) + row % (112, "ok2", 12)))
    assert genes.names == ["ok", "ok2"] and "1 genes whose CDS length is not a multiple of 3" in capsys.readouterr().out
    with pytest.raises(ValueError, match="twice"):
        gene_annotation.load_cds_bed12(write(tmp_path, "b.bed", row % (109, "dup", 9) + row % (109, "dup", 9)))
    with pytest.raises(ValueError, match="strand"):
        gene_annotation.load_cds_bed12(write(tmp_path, "c.bed", (row % (109, "s", 9)).replace("+", "?")))
    with pytest.raises(ValueError, match="ascending"):
        gene_annotation.load_cds_bed12(write(tmp_path, "d.bed", "1\t0\t30\tg\t0\t+\t0\t30\t0\t2\t6,6,\t0,3,\n"))

    class FakeGenome:
        names, lengths = ["chr1"], np.array([200], np.int64)

        def chrom_index(self, chroms):
            if chroms[0] not in ("1", "chr1"):
                raise KeyError(chroms[0])
            return np.array([0], np.int32)

    both = gene_annotation.load_cds_bed12(write(tmp_path, "e.bed", row % (109, "here", 9) + (row % (109, "there", 9)).replace("1\t", "7\t", 1)
                                                + "1\t300\t309\tbeyond\t0\t+\t300\t309\t0\t1\t9,\t0,\n"))
    kept, idx = both.on_genome(FakeGenome())
    assert kept.names == ["here"] and idx.tolist() == [0] and "Dropping 2 genes" in capsys.readouterr().out


def test_excerpt_of_the_shipped_gene_file():
    f_bed = os.path.join(GOLDEN, "cds_bed12_excerpt.bed")
    genes = gene_annotation.load_cds_bed12(f_bed)
    with open(f_bed) as f:
        text = f.read()
    stated = S.parse_bed12(text)
    assert len(genes) == len(stated) == 300 and genes.names == [x["name"] for x in stated]
    assert genes.names[:3] == ["OR4F5", "AL627309.1", "OR4F29"] and genes.blk_start[0] == 69091 and genes.blk_end[0] == 70008
    for g, x in enumerate(stated):
        a, b = genes.blk_ptr[g], genes.blk_ptr[g + 1]
        assert list(zip(genes.blk_start[a:b].tolist(), genes.blk_end[a:b].tolist())) == x["blocks"]
        assert genes.spl_pos[genes.spl_ptr[g]:genes.spl_ptr[g + 1]].tolist() == x["splice"]
        assert bool(genes.minus[g]) == (x["strand"] == "-")
        sizes = [e - s + 1 for s, e in x["blocks"]]
        assert genes.cds_off[a:b].tolist() == [sum(sizes[:k]) for k in range(len(sizes))] and genes.cds_len[g] == sum(sizes)
    assert (genes.cds_len % 3 == 0).all() and (np.diff(genes.blk_ptr) > 1).sum() > 200


def test_statement_on_hand_worked_cases():
    plus3, minus3, single = S.parse_bed12(HAND_BED)
    f = lambda gene, pos, alt: S.snv_function(SEQS, gene, pos, S.letter(SEQS, "1", pos), alt)[0]
    # the hand-made sequence spells what the comment above says
    assert "".join(S.letter(SEQS, "1", p) for p in S.cds_positions(plus3)) == "ATGGCTTGGTAACGTTATTGCTGACCCAAATAG"
    assert "".join(S.COMP[S.letter(SEQS, "1", p)] for p in S.cds_positions(minus3)) == "ATGCCCGTGGCTGAATGTAAATAG"
    # + strand, a codon inside one exon: GCT (Ala) third position -> synonymous; TGG (Trp) -> TGA stop gain, -> TGT missense
    assert f(plus3, 12, "C") == "Synonymous" and f(plus3, 15, "A") == "Nonsense" and f(plus3, 15, "T") == "Missense"
    # the in-frame stop TAA at 16-18: TAA -> TAG synonymous, -> CAA stop loss
    assert f(plus3, 18, "G") == "Synonymous" and f(plus3, 16, "C") == "Stop_loss"
    # + strand, exon 2 (TAT TGC TGA) and the last codon TAG
    assert f(plus3, 34, "A") == "Nonsense" and f(plus3, 61, "C") == "Stop_loss"
    # - strand, the codon GTG split over two exons: CDS indices 7-9 = genome 111 | 101, 100 (complemented)
    assert S.cds_positions(minus3)[6:9] == [111, 101, 100]
    assert f(minus3, 100, "T") == "Synonymous"                          # GTG -> GTA: the + strand C at 100 becomes T
    assert f(minus3, 101, "G") == "Missense"                            # GTG -> GCG (Ala)
    assert S.snv_function(SEQS, minus3, 111, "C", "A")[:2] == ("Missense", False)     # GTG -> TTG (Leu)
    # - strand, the codon TGT split the other way: CDS indices 16-18 = genome 93 | 79, 78; TGT -> TGA is a stop gain
    assert S.cds_positions(minus3)[15:18] == [93, 79, 78] and f(minus3, 78, "T") == "Nonsense"
    assert f(minus3, 74, "G") == "Stop_loss"                            # the last codon TAG -> CAG
    # + strand, a codon split over two exons: 7-20 | 31-40 reads ... TAA CG|G TAT TGC TGA
    split = S.parse_bed12("1\t6\t40\tsplit\t0\t+\t6\t40\t0\t2\t14,10,\t0,24,\n")[0]
    assert S.cds_positions(split)[12:15] == [19, 20, 31]
    assert S.snv_function(SEQS, split, 31, "G", "A")[:2] == ("Synonymous", False)     # CGG -> CGA, both Arg
    assert S.snv_function(SEQS, split, 20, "G", "A")[:2] == ("Missense", False)       # CGG -> CAG (Gln)
    assert S.snv_function(SEQS, split, 19, "C", "T")[:2] == ("Missense", False)       # CGG -> TGG (Trp)
    # the donor + 5 of the first intron of plus3 is 26; of minus3's first intron (transcript order) 106
    assert f(plus3, 26, "A") == "Essential_Splice" and f(minus3, 106, "C") == "Essential_Splice"
    # a wrong REF is reported with the class of ALT on the genome's codon
    assert S.snv_function(SEQS, plus3, 15, "C", "A")[:2] == ("Nonsense", True)
    # indel labels: CDS indices in transcript direction
    assert S.indel_label(plus3, 10, 12, "GCT", "-") == "INDEL_4_6_delinframe"
    assert S.indel_label(plus3, 10, 11, "GC", "-") == "INDEL_4_5_delfrshift"
    assert S.indel_label(plus3, 20, 24, "GTGTA", "-") == "INDEL_14_15_delfrshift"         # runs into the intron
    assert S.indel_label(plus3, 10, 10, "G", "GA") == "INDEL_3_4_insfrshift"              # the base in front is added
    assert S.indel_label(plus3, 10, 10, "G", "GAAAA") == "INDEL_3_4_insfrshift"
    assert S.indel_label(plus3, 7, 7, "-", "AAA") == "INDEL_1_1_insfrshift"               # 6 is not CDS
    # "inframe" counts the CDS positions of start - 1 .. end, not the inserted bases: three bases behind ONE reference base cover
    # 9, 10 (two positions: frshift), the same three bases behind TWO reference bases cover 9, 10, 11 (three: inframe)
    assert S.indel_label(plus3, 10, 10, "G", "GAAA") == "INDEL_3_4_insfrshift"
    assert S.indel_label(plus3, 10, 11, "GC", "GCAAA") == "INDEL_3_5_insinframe"
    assert S.indel_label(plus3, 10, 11, "GC", "GCA") == "INDEL_3_5_insinframe"            # one inserted base, still three positions
    assert S.indel_label(minus3, 115, 116, "CA", "CAGGG") == "INDEL_2_4_insinframe"       # 114, 115, 116 read from 117 downwards
    assert S.indel_label(single, 10, 11, "GC", "GCAAA") == "INDEL_1_2_insfrshift"         # 9 lies in front of the gene
    assert S.indel_label(plus3, 10, 11, "GC", "TT") == "INDEL_4_5_mnv"
    assert S.indel_label(plus3, 22, 23, "GT", "-") == "cds_INDEL"                         # splice positions only
    assert S.indel_label(minus3, 115, 117, "CAT", "-") == "INDEL_1_3_delinframe"
    assert S.indel_label(minus3, 78, 79, "AC", "-") == "INDEL_17_18_delfrshift"
    assert S.indel_label(minus3, 100, 111, "C" * 12, "-") == "INDEL_7_9_delinframe"       # over an intron: 111 | 101, 100
    assert single["splice"] == [] and S.hits([plus3, minus3, single], "1", 12, 12) == [0, 2]


def statement_join(r_chrom, r_start, r_end, m_chrom, m_start, m_end):
    pairs = [(m, r) for m in range(len(m_start)) for r in range(len(r_start))
             if r_chrom[r] == m_chrom[m] and r_start[r] <= m_end[m] and m_start[m] <= r_end[r]]
    return np.array([p[0] for p in pairs], np.int64), np.array([p[1] for p in pairs], np.int64)


def statement_classifier(seqs, stated):
    def classify(genome, genes, gene_chrom, gene, start, end, kind, ref, alt):
        assert genes.names == [x["name"] for x in stated]
        out = [S.pair_outputs(seqs, stated[g], int(s), int(e), int(k), "ACGT"[r], "ACGT"[a])
               for g, s, e, k, r, a in zip(gene, start, end, kind, ref, alt)]
        labels = [S.snv_function(seqs, stated[g], int(s), "ACGT"[r], "ACGT"[a])[:2] if k == 0 else ("Synonymous", False)
                  for g, s, k, r, a in zip(gene, start, kind, ref, alt)]
        impact = np.array([S.IMPACT_CODE[l[0]] for l in labels], np.uint8)
        wrong = np.array([l[1] for l in labels], bool)
        o = np.array(out, np.int64).reshape(-1, 5)
        return impact, wrong, o[:, 2], o[:, 3], o[:, 4]
    return classify


def annotate_on_cpu(tmp_path, text, bed=HAND_BED, seqs=SEQS):
    stated = S.parse_bed12(bed)
    f_out = str(tmp_path / "out.tsv")
    counts = mutation_tools.annotate_mutation_function(write(tmp_path, "raw.tsv", text), f_out, write(tmp_path, "g.bed", bed), None,
                                                       join=statement_join, classify=statement_classifier(seqs, stated))
    with open(f_out) as f:
        return f.read(), counts


HAND_CALLS_5 = "\n".join([
    "2\t10\tG\tT\tS1",                # a contig without genes
    "1\t12\tT\tC\tS2",                # plus3 Synonymous and single (two rows)
    "1\t12\tT\tC\tS2",                # exact duplicate
    "1\t12\tT\tC\tS1",                # another sample: kept
    "1\t15\tG\tG\tS1",                # REF == ALT
    "1\t15\tG\tA\tS1",                # Nonsense in plus3 and in single
    "1\t26\tG\tA\tS1",                # donor + 5
    "1\t\tG\tA\tS1",                  # an empty field
    "1\t9\tCAT\tC\tS3",               # deletion written from the base in front: start 10
    "1\t10\tG\tGAA\tS3",              # insertion
    "1\t3\tG\tGA\tS3",                # noncoding insertion
    "1\t78\tA\tT\tS1",                # minus3 Nonsense, a codon split over two exons
    "1\t100\tCA\tGT\tS1",             # MNV at the exon edge of minus3
    "1\t5\tC\tA\tS9",                 # noncoding
    "1\t61\tG\tC\tS1",                # Stop_loss
    "1\t22\tGT\t-\tS1",               # only splice positions
    "1\t10\tGC\tGCAAA\tS4",           # insertion behind two reference bases: positions 9-11, in frame in plus3
]) + "\n"


def test_host_code_rows_and_order(tmp_path, capsys):
    stated = S.parse_bed12(HAND_BED)
    want, _ = S.annotate(HAND_CALLS_5, stated, SEQS)
    got, counts = annotate_on_cpu(tmp_path, HAND_CALLS_5)
    assert got == want
    rows = [ln.split("\t") for ln in got.splitlines()]
    assert ["1", "11", "12", "T", "C", "S2", "plus3", "Synonymous"] in rows and ["1", "11", "12", "T", "C", "S2", "single", "Synonymous"] in rows
    assert sum(r[:6] == ["1", "11", "12", "T", "C", "S2"] for r in rows) == 2 and ["1", "11", "12", "T", "C", "S1", "plus3", "Synonymous"] in rows
    assert ["1", "9", "11", "CAT", "C", "S3", "plus3", "INDEL_4_5_delfrshift"] in rows              # start shifted to 10
    assert ["1", "9", "10", "G", "GAA", "S3", "plus3", "INDEL_3_4_insfrshift"] in rows
    assert ["1", "9", "11", "GC", "GCAAA", "S4", "plus3", "INDEL_3_5_insinframe"] in rows
    assert ["1", "9", "11", "GC", "GCAAA", "S4", "single", "INDEL_1_2_insfrshift"] in rows
    assert [r[3:7] for r in rows if r[:3] == ["1", "9", "11"]] == [["CAT", "C", "S3", "plus3"], ["CAT", "C", "S3", "single"],
                                                                   ["GC", "GCAAA", "S4", "plus3"], ["GC", "GCAAA", "S4", "single"]]
    assert ["1", "2", "3", "G", "GA", "S3", ".", "Noncoding_INDEL"] in rows and ["2", "9", "10", "G", "T", "S1", ".", "Noncoding"] in rows
    assert ["1", "25", "26", "G", "A", "S1", "plus3", "Essential_Splice"] in rows and ["1", "77", "78", "A", "T", "S1", "minus3", "Nonsense"] in rows
    assert ["1", "60", "61", "G", "C", "S1", "plus3", "Stop_loss"] in rows and ["1", "21", "23", "GT", "-", "S1", "plus3", "cds_INDEL"] in rows
    assert ["1", "99", "101", "CA", "GT", "S1", "minus3", "INDEL_8_9_mnv"] in rows
    # ties of (CHROM, START, END): coding SNVs first (input order, genes in table order), then coding others
    tie = [r[5:] for r in rows if r[:3] == ["1", "9", "10"]]
    assert tie == [["S3", "plus3", "INDEL_3_4_insfrshift"], ["S3", "single", "INDEL_1_1_insfrshift"]]
    assert [r[5:7] for r in rows if r[:3] == ["1", "11", "12"]] == [["S2", "plus3"], ["S2", "single"], ["S1", "plus3"], ["S1", "single"]]
    assert counts["n_mutations"] == 14 and counts["n_rows"] == len(rows) and "duplicated because they overlap multiple genes" in capsys.readouterr().out
    # the same calls as a 6-column file (0-based START, a further column) give the same bytes; so does a space-separated file
    six = "".join("\t".join([c[0], str(int(c[1]) - 1) if c[1] else "", "0", c[2], c[3], c[4], "x"]) + "\n"
                  for c in (ln.split("\t") for ln in HAND_CALLS_5.splitlines()))
    assert annotate_on_cpu(tmp_path, six)[0] == want and S.annotate(six, stated, SEQS)[0] == want
    spaced = "".join(" ".join(ln.split("\t")) + "\n" for ln in HAND_CALLS_5.splitlines() if "\t\t" not in ln)
    assert annotate_on_cpu(tmp_path, spaced)[0] == want


def test_chromosomes_sort_as_bytes_and_coordinates_stay_integers(tmp_path):
    bed = HAND_BED
    calls = "X\t100000\tA\tC\tS1\n10\t5\tA\tC\tS1\n1\t100000\tA\tC\tS1\n2\t7\tA\tC\tS1\nchr1\t3\tA\tC\tS1\n"
    got, _ = annotate_on_cpu(tmp_path, calls, bed=bed)
    assert [ln.split("\t")[:3] for ln in got.splitlines()] == [["1", "99999", "100000"], ["10", "4", "5"], ["2", "6", "7"], ["X", "99999", "100000"],
                                                               ["chr1", "2", "3"]]
    assert got == S.annotate(calls, S.parse_bed12(bed), SEQS)[0]


def test_wrong_reference_rule(tmp_path, capsys):
    stated = S.parse_bed12(HAND_BED)
    good = ["1\t%d\t%s\t%s\tS1" % (p, HAND_SEQ[p - 1], "A" if HAND_SEQ[p - 1] != "A" else "C") for p in range(7, 22)] + \
           ["1\t%d\t%s\t%s\tS1" % (p, HAND_SEQ[p - 1], "A" if HAND_SEQ[p - 1] != "A" else "C") for p in range(53, 62)]
    bad = "1\t35\t%s\tA\tS1" % ("C" if HAND_SEQ[34] != "C" else "G")
    # plus3 pairs: 24 good + 1 bad; single pairs: 9 good (positions 10-18) -> 1 of 34 pairs: a warning, the row is left out
    text = "\n".join(good + [bad]) + "\n"
    want, wrong_n = S.annotate(text, stated, SEQS)
    got, counts = annotate_on_cpu(tmp_path, text)
    assert got == want and wrong_n == counts["wrong_ref"] == 1 and "\t34\t35\t" not in got
    assert "1 (2.9%) mutations have a wrong reference base" in capsys.readouterr().out
    # 4 of 34 + 3 pairs is above 10 %: an error in both
    more = ["1\t%d\t%s\tA\tS1" % (p, "C" if HAND_SEQ[p - 1] != "C" else "G") for p in (36, 37, 38)]
    text = "\n".join(good + [bad] + more) + "\n"
    with pytest.raises(ValueError, match="wrong assembly"):
        S.annotate(text, stated, SEQS)
    with pytest.raises(ValueError, match="wrong assembly"):
        annotate_on_cpu(tmp_path, text)
    # exactly 10 %: 27 good pairs (80 is a splice position of minus3) + 3 bad ones -> an error ("10 % or more")
    ten = [g for g in good if int(g.split("\t")[1]) >= 53] + ["1\t%d\t%s\t%s\tS1" % (p, HAND_SEQ[p - 1], "A" if HAND_SEQ[p - 1] != "A" else "C")
                                                             for p in range(32, 41)] + \
          ["1\t%d\t%s\t%s\tS1" % (p, HAND_SEQ[p - 1], "A" if HAND_SEQ[p - 1] != "A" else "C") for p in range(72, 81)]
    text = "\n".join(ten + ["1\t%d\t%s\tA\tS1" % (p, "C" if HAND_SEQ[p - 1] != "C" else "G") for p in (94, 95, 96)]) + "\n"
    with pytest.raises(ValueError, match="wrong assembly"):
        annotate_on_cpu(tmp_path, text)
    with pytest.raises(ValueError, match="wrong assembly"):
        S.annotate(text, stated, SEQS)


def test_short_rows_and_unfinished_pairs(tmp_path):
    stated = S.parse_bed12(HAND_BED)
    # a tab-separated row shorter than the first one has empty fields: dropped, as a row with an empty field is
    text = "1\t12\tT\tC\tS2\n1\t15\tG\n1\t15\tG\tA\tS1\n"
    got, counts = annotate_on_cpu(tmp_path, text)
    assert got == S.annotate(text, stated, SEQS)[0] and counts["n_mutations"] == 2 and got.count("\n") == 4
    # a classifier that leaves an SNV pair without a class (DIG_MF_NONE) is an error, not a splice label
    inner = statement_classifier(SEQS, stated)

    def unfinished(*args):
        impact, wrong, n, lo, hi = inner(*args)
        impact[0] = 255
        return impact, wrong, n, lo, hi

    with pytest.raises(ValueError, match="without an effect class"):
        mutation_tools.annotate_mutation_function(write(tmp_path, "raw.tsv", text), str(tmp_path / "o.tsv"), write(tmp_path, "g.bed", HAND_BED),
                                                  None, join=statement_join, classify=unfinished)


def test_product_without_gpu_has_no_fallback(tmp_path):
    """Without the two functions the orchestration calls the HIP library: without a GPU (or without a built library) that is an
    error, never a CPU result."""
    from digdriver_amd import _lib
    try:
        has_gpu = _lib.device_count() > 0
    except _lib.DigHipError:
        has_gpu = False                                                 # (the library has not been built: the call below says so)
    if has_gpu:
        pytest.skip("a GPU is present")
    from digdriver_amd.data_tools.genome import PackedGenome
    with pytest.raises(_lib.DigHipError):
        mutation_tools.annotate_mutation_function(write(tmp_path, "raw.tsv", HAND_CALLS_5), str(tmp_path / "o.tsv"),
                                                  write(tmp_path, "g.bed", HAND_BED), PackedGenome.from_sequences(SEQS), on_device=False)
