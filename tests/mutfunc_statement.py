"""An independent statement of addMutationFunction in plain Python: strings, a dict codon table, per-position loops.

Written from the annotation rule (the gene table from a bed12 of coding exons, essential-splice positions per intron, the
eight steps from the raw call file to the sorted 8-column file) and from reading the reference's R script; it shares no code
with digdriver_amd.  The tests compare the product -- the gene table, the kernel's per-pair outputs, the written file -- with it.
"""

_TCAG = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
CODON = {a + b + c: _TCAG[16 * i + 4 * j + k] for i, a in enumerate("TCAG") for j, b in enumerate("TCAG") for k, c in enumerate("TCAG")}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
DONOR, ACCEPTOR = (1, 2, 5), (1, 2)              # bases into the intron, from the exon in front of it / behind it (transcript)
IMPACT_CODE = {"Synonymous": 0, "Missense": 1, "Nonsense": 2, "Stop_loss": 3, "Essential_Splice": 4}
OK, WRONG_REF, HOST = 0, 1, 2


def translate(codon):
    return CODON.get("".join(codon), "X")


def parse_bed12(text, donor=DONOR, acceptor=ACCEPTOR):
    """bed12 text -> list of genes (dicts: name, chrom, strand '+'/'-', blocks [(start, end)] 1-based closed ascending, splice: sorted
    list).  Genes whose CDS length is not a multiple of 3 are left out; a repeated name raises ValueError."""
    genes, seen = [], set()
    for line in text.splitlines():
        if not line.strip():
            continue
        c = line.split("\t")
        name = c[3]
        if name in seen:
            raise ValueError("duplicate gene " + name)
        seen.add(name)
        strand = {"+": "+", "1": "+", "-": "-", "-1": "-"}[c[5]]
        sizes = [int(x) for x in c[10].split(",") if x != ""]
        starts = [int(x) for x in c[11].split(",") if x != ""]
        blocks = [(int(c[1]) + s + 1, int(c[1]) + s + z) for s, z in zip(starts, sizes)]
        if sum(e - s + 1 for s, e in blocks) % 3 != 0:
            continue
        splice = set()
        for (_, left_end), (right_start, _) in zip(blocks[:-1], blocks[1:]):
            if strand == "+":                     # transcript runs left to right: donor behind the left exon
                splice |= {left_end + k for k in donor} | {right_start - k for k in acceptor}
            else:                                 # right to left: donor in front of the right exon (in genome order)
                splice |= {right_start - k for k in donor} | {left_end + k for k in acceptor}
        genes.append(dict(name=name, chrom=c[0], strand=strand, blocks=blocks, splice=sorted(splice)))
    return genes


def cds_positions(gene):
    """Genome positions of the CDS in transcript direction (index 0 is CDS index 1)."""
    if "_cds" not in gene:                         # (kept with the gene: the tests ask for it per pair)
        pos = [p for s, e in gene["blocks"] for p in range(s, e + 1)]
        gene["_cds"] = pos[::-1] if gene["strand"] == "-" else pos
    return gene["_cds"]


def letter(seqs, chrom, pos):
    s = seqs[chrom] if chrom in seqs else seqs["chr" + chrom]
    return s[pos - 1].upper()


def snv_function(seqs, gene, pos, ref, alt):
    """(label, wrong_ref, touches_other, pos_ind or 0) of an SNV at `pos` (1-based) inside the gene's ranges."""
    minus = gene["strand"] == "-"
    base = letter(seqs, gene["chrom"], pos)
    wrong = base != ref
    if pos in gene["splice"]:
        return "Essential_Splice", wrong, base not in "ACGT", 0
    cds = cds_positions(gene)
    pos_ind = cds.index(pos) + 1
    k = -(-pos_ind // 3)
    old = []
    for t in (3 * k - 2, 3 * k - 1, 3 * k):
        c = letter(seqs, gene["chrom"], cds[t - 1])
        old.append(COMP.get(c, c) if minus else c)
    new = list(old)
    new[pos_ind - 3 * (k - 1) - 1] = COMP[alt] if minus else alt
    old_aa, new_aa = translate(old), translate(new)
    if new_aa == old_aa:
        label = "Synonymous"
    elif new_aa == "*":
        label = "Nonsense"
    elif old_aa != "*":
        label = "Missense"
    else:
        label = "Stop_loss"
    return label, wrong, any(c not in "ACGT" for c in old) or base not in "ACGT", pos_ind


def cds_span(gene, start, end, insertion):
    """(count, min, max) of the CDS indices of positions start .. end (start - 1 .. end for an insertion); (0, 0, 0) if none."""
    cds = cds_positions(gene)
    wanted = set(range(start - 1 if insertion else start, end + 1))
    idx = [i + 1 for i, p in enumerate(cds) if p in wanted]
    return (len(idx), min(idx), max(idx)) if idx else (0, 0, 0)


def indel_label(gene, start, end, ref, alt):
    r, a = len(ref.replace("-", "")), len(alt.replace("-", ""))
    n, lo, hi = cds_span(gene, start, end, r < a)
    if n == 0:
        return "cds_INDEL"
    if r == a:
        return "INDEL_%d_%d_mnv" % (lo, hi)
    return "INDEL_%d_%d_%s%s" % (lo, hi, "ins" if r < a else "del", "inframe" if n % 3 == 0 else "frshift")


def pair_outputs(seqs, gene, start, end, kind, ref, alt):
    """What the kernel reports for one pair: (impact, status, n_cds, cds_min, cds_max); kind 0 SNV, 1 insertion, 2 other."""
    if kind == 0:
        label, wrong, other, pos_ind = snv_function(seqs, gene, start, ref, alt)
        status = HOST if other else WRONG_REF if wrong else OK
        return 255 if other else IMPACT_CODE[label], status, 1 if pos_ind else 0, pos_ind, pos_ind
    return (255, OK) + cds_span(gene, start, end, kind == 1)


def read_rows(text):
    """Steps 1-3: [(chrom, pos, ref, alt, sample, start, end)] in file order."""
    lines = [ln for ln in text.split("\n") if ln.strip() != ""]
    if not lines:
        return []
    tabbed = "\t" in lines[0]
    split = (lambda s: [x.strip() for x in s.rstrip("\r").split("\t")]) if tabbed else (lambda s: s.split())
    width = len(split(lines[0]))
    rows, seen = [], set()
    for ln in lines:
        f = split(ln)
        f = f + [""] * (width - len(f))
        if width == 5:
            chrom, pos, ref, alt, sample = f[:5]
        else:
            chrom, pos, _, ref, alt, sample = f[:6]
        if "" in (chrom, pos, ref, alt, sample) or ref == alt:
            continue
        pos = int(pos) + (0 if width == 5 else 1)
        if (sample, chrom, pos, ref, alt) in seen:
            continue
        seen.add((sample, chrom, pos, ref, alt))
        start, end = pos, pos + len(ref) - 1
        if ref[0] == alt[0] and len(ref) > len(alt):
            start += 1
        rows.append((chrom, pos, ref, alt, sample, start, end))
    return rows


def hits(genes, chrom, start, end):
    """Indices of the genes (table order) with a CDS block or a splice position inside [start, end] on `chrom`."""
    out = []
    for gi, g in enumerate(genes):
        if g["chrom"] != chrom:
            continue
        if any(s <= end and start <= e for s, e in g["blocks"]) or any(start <= p <= end for p in g["splice"]):
            out.append(gi)
    return out


def annotate(text, genes, seqs):
    """Steps 1-8 -> (the text of the output file, number of wrong-REF pairs).  ValueError when 10 % or more of the coding SNV pairs
    have a wrong REF."""
    coding_snv, nonc_snv, coding_other, nonc_other = [], [], [], []
    wrong_n = 0
    for chrom, pos, ref, alt, sample, start, end in read_rows(text):
        snv = ref in ("A", "C", "G", "T") and alt in ("A", "C", "G", "T")
        row = (chrom, start - 1, end, ref, alt, sample)
        gis = hits(genes, chrom, start, end)
        if not gis:
            (nonc_snv if snv else nonc_other).append(row + (".", "Noncoding" if snv else "Noncoding_INDEL"))
        for gi in gis:
            if snv:
                label, wrong, _, _ = snv_function(seqs, genes[gi], pos, ref, alt)
                wrong_n += wrong
                coding_snv.append((row + (genes[gi]["name"], label), wrong))
            else:
                coding_other.append(row + (genes[gi]["name"], indel_label(genes[gi], start, end, ref, alt)))
    if coding_snv and 10 * wrong_n >= len(coding_snv):
        raise ValueError("wrong assembly?")
    rows = [r for r, wrong in coding_snv if not wrong] + nonc_snv + coding_other + nonc_other
    rows.sort(key=lambda r: (r[0].encode(), r[1], r[2]))            # (list.sort is stable)
    return "".join("\t".join(str(x) for x in r) + "\n" for r in rows), wrong_n
