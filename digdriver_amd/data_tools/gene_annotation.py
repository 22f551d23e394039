"""The gene table of addMutationFunction: the coding exons of every gene, from a bed12 file.

The reference's scripts/mutationFunction.R loads all of this from dNdScv's refcds_hg19.rda (intervals_cds, intervals_splice, strand and
the expanded CDS strings of every gene, plus `gr_genes`, the ranges the mutations are overlapped with).  Here it is derived from a
bed12 file of the coding exons (the reference ships DIGDriver/data/genes.MARTINCORENA.bed) -- strand in column 6, the CDS blocks in
columns 10-12 -- and the CDS letters come from the FASTA at annotation time (dig_mutation_function).

Essential-splice positions are derived per intron from SPLICE_OFFSETS.  UNPINNED: this is dNdScv's published definition (donor
+1, +2, +5 and acceptor -1, -2) as far as the authors of this module can tell; it has not been compared with the intervals_splice
of refcds_hg19.rda.
"""
import numpy as np

# counted from the exon edge into the intron, in transcript direction: the donor site follows an exon (+k = the k-th intron base
# behind it), the acceptor site precedes the next exon (-k = the k-th intron base in front of it); mirrored for - genes
SPLICE_OFFSETS = {"donor": (1, 2, 5), "acceptor": (-1, -2)}


class GeneSet:
    """names: list of str; chrom: the label as in the file (object array of str); minus: u8; CSR blk_ptr with blk_start / blk_end
    (1-based closed, ascending and disjoint inside a gene) and cds_off (CDS length in front of each block, genome order); cds_len per
    gene; CSR spl_ptr with spl_pos (ascending inside a gene).  All positions int64."""

    def __init__(self, names, chrom, minus, blk_ptr, blk_start, blk_end, spl_ptr, spl_pos):
        self.names = list(names)
        self.chrom = np.asarray(chrom, dtype=object)
        self.minus = np.ascontiguousarray(minus, np.uint8)
        self.blk_ptr = np.ascontiguousarray(blk_ptr, np.int64)
        self.blk_start = np.ascontiguousarray(blk_start, np.int64)
        self.blk_end = np.ascontiguousarray(blk_end, np.int64)
        self.spl_ptr = np.ascontiguousarray(spl_ptr, np.int64)
        self.spl_pos = np.ascontiguousarray(spl_pos, np.int64)
        size = self.blk_end - self.blk_start + 1
        before = np.cumsum(size) - size                                  # over all blocks; minus the gene's first block's value
        nblk = np.diff(self.blk_ptr)
        self.cds_off = np.ascontiguousarray(before - np.repeat(before[self.blk_ptr[:-1][nblk > 0]], nblk[nblk > 0]), np.int64) \
            if len(size) else np.zeros(0, np.int64)
        total = np.concatenate([[0], np.cumsum(size)])
        self.cds_len = total[self.blk_ptr[1:]] - total[self.blk_ptr[:-1]]

    def __len__(self):
        return len(self.names)

    def subset(self, keep):
        """The genes keep (bool mask or indices), in order."""
        keep = np.flatnonzero(keep) if np.asarray(keep).dtype == bool else np.asarray(keep, np.int64)
        take = lambda ptr, a: np.concatenate([a[ptr[g]:ptr[g + 1]] for g in keep] or [np.zeros(0, np.int64)])
        ptr = lambda p: np.concatenate([[0], np.cumsum((p[1:] - p[:-1])[keep])])
        return GeneSet([self.names[g] for g in keep], self.chrom[keep], self.minus[keep], ptr(self.blk_ptr),
                       take(self.blk_ptr, self.blk_start), take(self.blk_ptr, self.blk_end), ptr(self.spl_ptr),
                       take(self.spl_ptr, self.spl_pos))

    def on_genome(self, genome):
        """(genes, chrom_index): the genes whose contig `genome` (a PackedGenome) holds -- '1' and 'chr1' name the same contig, as
        for every other command here -- and lie inside it, with the contig's index per gene; the others are dropped with a
        message."""
        idx = np.full(len(self), -1, np.int32)
        for lab in dict.fromkeys(self.chrom.tolist()):
            try:
                idx[self.chrom == lab] = genome.chrom_index([lab])[0]
            except KeyError:
                pass
        ok = idx >= 0
        last = self.blk_end[np.maximum(self.blk_ptr[1:] - 1, 0)] if len(self.blk_end) else np.zeros(len(self), np.int64)
        ok &= (np.diff(self.blk_ptr) == 0) | (last <= genome.lengths[np.maximum(idx, 0)])
        if not ok.all():
            print("Dropping {} genes on contigs the FASTA does not hold (or beyond their end): {}".format(
                int((~ok).sum()), ", ".join(sorted(set(self.chrom[~ok].tolist())))))
            return self.subset(ok), idx[ok]
        return self, idx

    def ranges(self):
        """The ranges mutations are overlapped with (the R script's gr_genes): every CDS block and every splice position as a
        one-base interval -> (chrom labels, start, end (1-based closed), gene index), sorted by (chrom as text, start)."""
        gene = np.concatenate([np.repeat(np.arange(len(self)), np.diff(self.blk_ptr)), np.repeat(np.arange(len(self)), np.diff(self.spl_ptr))])
        start = np.concatenate([self.blk_start, self.spl_pos])
        end = np.concatenate([self.blk_end, self.spl_pos])
        chrom = self.chrom[gene].astype(str) if len(gene) else np.zeros(0, str)
        _, code = np.unique(chrom, return_inverse=True) if len(gene) else (None, np.zeros(0, np.int64))
        order = np.lexsort((gene, start, code))
        return chrom[order], start[order], end[order], gene[order].astype(np.int64)


def splice_positions(blk_start, blk_end, minus, splice_offsets=None):
    """Essential-splice positions (ascending, unique) of one gene from its ascending 1-based closed CDS blocks."""
    offs = SPLICE_OFFSETS if splice_offsets is None else splice_offsets
    donor, acceptor = [abs(int(k)) for k in offs["donor"]], [abs(int(k)) for k in offs["acceptor"]]
    out = []
    for left_end, right_start in zip(blk_end[:-1], blk_start[1:]):       # one intron: left_end + 1 .. right_start - 1
        after_left, before_right = (acceptor, donor) if minus else (donor, acceptor)
        out += [int(left_end) + k for k in after_left] + [int(right_start) - k for k in before_right]
    return sorted(set(out))


def _strand_minus(s):
    s = str(s).strip()
    if s in ("+", "1", "+1"):
        return 0
    if s in ("-", "-1"):
        return 1
    raise ValueError("strand %r (column 6) is neither +/- nor 1/-1" % s)


def load_cds_bed12(f_bed, splice_offsets=None):
    """bed12 of coding exons -> GeneSet.  Block i of a row is chromStart + blockStarts[i] + 1 .. chromStart + blockStarts[i] +
    blockSizes[i] (1-based closed); a trailing comma in the block lists is allowed.  A gene whose CDS length is not a multiple of 3
    is dropped (count printed); a duplicate gene name, an unsorted or overlapping block list raise ValueError."""
    names, chrom, minus, blk_ptr, bs, be, spl_ptr, sp = [], [], [], [0], [], [], [0], []
    seen, dropped = set(), 0
    with open(f_bed) as f:
        for ln, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line or line.startswith(("#", "track", "browser")):
                continue
            c = line.split("\t")
            if len(c) < 12:
                raise ValueError("%s line %d: %d columns, a bed12 row has 12" % (f_bed, ln, len(c)))
            name = c[3]
            if name in seen:
                raise ValueError("%s line %d: gene name %r appears twice" % (f_bed, ln, name))
            seen.add(name)
            sizes = [int(x) for x in c[10].rstrip(",").split(",")]
            starts = [int(x) for x in c[11].rstrip(",").split(",")]
            if len(sizes) != len(starts) or len(sizes) != int(c[9]) or min(sizes) < 1:
                raise ValueError("%s line %d (%s): blockCount, blockSizes and blockStarts disagree" % (f_bed, ln, name))
            s = [int(c[1]) + x + 1 for x in starts]
            e = [int(c[1]) + x + z for x, z in zip(starts, sizes)]
            if any(e[i] >= s[i + 1] for i in range(len(s) - 1)):
                raise ValueError("%s line %d (%s): blocks must be ascending and disjoint" % (f_bed, ln, name))
            mi = _strand_minus(c[5])
            if sum(sizes) % 3:
                dropped += 1
                continue
            names.append(name)
            chrom.append(c[0])
            minus.append(mi)
            bs += s
            be += e
            blk_ptr.append(len(bs))
            sp += splice_positions(s, e, mi, splice_offsets)
            spl_ptr.append(len(sp))
    if dropped:
        print("Dropping {} genes whose CDS length is not a multiple of 3".format(dropped))
    return GeneSet(names, chrom, minus, blk_ptr, bs, be, spl_ptr, sp)
