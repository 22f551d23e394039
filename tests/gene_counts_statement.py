"""An independent statement of the per-gene counts of possible substitutions (the L of the gene container) in plain Python:
strings, a per-base loop, the dict codon table of mutfunc_statement.py.

Written from the rule, not from the kernel.  For every CDS base of a gene, in transcript direction, and each of the three other
letters: the codon with the letter in place is translated; same amino acid -> silent (class 0), a new stop -> nonsense (2), a
changed amino acid of a codon that was no stop -> missense (1), a stop that is lost -> no class, counted on its own.  Every
essential-splice position adds its three other letters to class 3.  The substitution's name is "XYZ>XaZ" with XYZ the three
letters of the GENOME around the base, reverse-complemented for a gene on the - strand; its column is its place in the sorted
list of the 192 names.  A site whose three letters hold anything but ACGT, or that has no neighbour because the contig ends,
has no name and is skipped; a codon with such a letter elsewhere translates to X.
"""
import mutfunc_statement as S

NAMES = sorted(x + y + z + ">" + x + a + z for x in "ACGT" for y in "ACGT" for z in "ACGT" for a in "ACGT" if a != y)
COLUMN = {name: i for i, name in enumerate(NAMES)}
SILENT, MISSENSE, NONSENSE, SPLICE = 0, 1, 2, 3


def reverse_complement(s):
    return "".join(S.COMP.get(c, c) for c in reversed(s))


def contig(seqs, chrom):
    return (seqs[chrom] if chrom in seqs else seqs["chr" + chrom]).upper()


def site_name_prefix(seq, pos, minus):
    """The three letters around 1-based `pos` as the gene's strand reads them; None when there are not three ACGT letters."""
    if pos - 1 < 1 or pos + 1 > len(seq):
        return None
    tri = seq[pos - 2:pos + 1]
    if any(c not in "ACGT" for c in tri):
        return None
    return reverse_complement(tri) if minus else tri


def gene_counts(seqs, gene):
    """(L: 4 lists of 192 counts, stop-loss count, True when a letter the gene reads is not ACGT or a neighbour is missing)."""
    seq = contig(seqs, gene["chrom"])
    minus = gene["strand"] == "-"
    L = [[0] * 192 for _ in range(4)]
    stop_loss, other = 0, False
    cds = S.cds_positions(gene)
    for i, pos in enumerate(cds):
        first = i - i % 3
        codon = []
        for p in cds[first:first + 3]:
            c = seq[p - 1]
            codon.append(S.COMP.get(c, c) if minus else c)
        tri = site_name_prefix(seq, pos, minus)
        if tri is None:
            other = True
            continue
        assert tri[1] == codon[i % 3]
        old_aa = S.translate(codon)
        for alt in "ACGT":
            if alt == tri[1]:
                continue
            new = list(codon)
            new[i % 3] = alt
            new_aa = S.translate(new)
            col = COLUMN[tri + ">" + tri[0] + alt + tri[2]]
            if new_aa == old_aa:
                L[SILENT][col] += 1
            elif new_aa == "*":
                L[NONSENSE][col] += 1
            elif old_aa != "*":
                L[MISSENSE][col] += 1
            else:
                stop_loss += 1
    for pos in gene["splice"]:
        tri = site_name_prefix(seq, pos, minus)
        if tri is None:
            other = True
            continue
        for alt in "ACGT":
            if alt != tri[1]:
                L[SPLICE][COLUMN[tri + ">" + tri[0] + alt + tri[2]]] += 1
    return L, stop_loss, other
