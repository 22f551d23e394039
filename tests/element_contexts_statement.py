"""The plain statement of engine.element_context_counts (dig_element_context_counts) over FASTA strings: a loop over the centres,
nothing shared with the library or with sequence_tools.

out[e] = the sum over the blocks of element e of the trinucleotide counts of the block on the element's strand:
  centres max(start, 1) .. min(end, chrom_len - 1) - 1 (the reference's fetch is widened by one base, START == 0 becomes 1, and it
  is truncated at the chromosome end: sequence_tools.py:21-29); a triplet with a letter other than ACGT is skipped (:42-55); a '-'
  element counts the reverse complement (:527-566); context index 16 b0 + 4 b1 + b2 with A C G T = 0 .. 3."""
import numpy as np

_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def block_counts(seq, start, end, minus):
    """int64 [64] of one block of a chromosome given as a string (any case)."""
    out = np.zeros(64, np.int64)
    for c in range(max(int(start), 1), min(int(end), len(seq) - 1)):
        tri = seq[c - 1:c + 2].upper()
        if len(tri) != 3 or any(x not in _CODE for x in tri):
            continue
        b0, b1, b2 = (_CODE[x] for x in tri)
        if minus:
            b0, b1, b2 = 3 - b2, 3 - b1, 3 - b0
        out[16 * b0 + 4 * b1 + b2] += 1
    return out


def element_counts(seqs, elt_chrom, elt_minus, blk_ptr, blk_start, blk_end):
    """int64 [E, 64]; seqs: dict chromosome label -> string, elt_chrom: labels of seqs."""
    E = len(elt_chrom)
    out = np.zeros((E, 64), np.int64)
    for e in range(E):
        for b in range(int(blk_ptr[e]), int(blk_ptr[e + 1])):
            out[e] += block_counts(seqs[elt_chrom[e]], blk_start[b], blk_end[b], bool(elt_minus[e]))
    return out
