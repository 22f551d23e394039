"""A plain statement of the training labels (scripts/DataExtractor.py:525-572 add_objectives without --cnv), the CPU yardstick of
dig_window_pair_keys / dig_window_sample_hits / dig_window_objectives -- loops, sets and dictionaries, nothing shared with the product.

    rows   (CHROM label, START, END, REF, ALT, SAMPLE, GENE, ANNOT) in file order
    idx    [N, 3] integers: CHROM, START, END

  1. window i is named 'CHROM:START-END'
  2. a row meets a window of the same chromosome label (compared as text) when the half-open intervals overlap, an empty interval
     taken as one base; of the joined rows with one (CHROM, START, END, REF, ALT, SAMPLE, window) the first counts, as OBS_INDEL when
     its ANNOT is 'INDEL' and as OBS_SNV otherwise; one table row per (window, SAMPLE)
  3. the per-(window, sample) cap clips OBS_MUT only: nothing the label is made of
  4. sample_filter_stdev k: a sample's load is its number of table rows (the windows it hits); samples with load > std * k go,
     std with ddof = 1 (not a number for a single sample: nobody goes)
  5. max_muts_per_sample m: samples with load > m go
  6. 0 and None switch an option off
  7. label[i] = the sum of OBS_SNV over the remaining table rows of window i
"""
import math


def sample_loads(idx, rows):
    """({(window name, sample): [snv, indel]}, {sample: number of windows it hits})"""
    by_chrom = {}
    for c, s, e in idx:
        by_chrom.setdefault(str(int(c)), []).append((int(s), int(e), '{}:{}-{}'.format(int(c), int(s), int(e))))
    seen, table = set(), {}
    for ch, s, e, ref, alt, samp, _gene, annot in rows:
        if samp is None:
            continue
        m_end = e if e > s else s + 1
        for ws, we, name in by_chrom.get(str(ch), ()):
            if s < (we if we > ws else ws + 1) and ws < m_end:
                ident = (str(ch), s, e, ref, alt, samp, name)
                if ident in seen:
                    continue
                seen.add(ident)
                table.setdefault((name, samp), [0, 0])[1 if annot == 'INDEL' else 0] += 1
    loads = {}
    for _name, samp in table:
        loads[samp] = loads.get(samp, 0) + 1
    return table, loads


def stdev(values):
    n = len(values)
    if n < 2:
        return float('nan')
    mean = sum(values) / n
    return math.sqrt(sum((v - mean) ** 2 for v in values) / (n - 1))


def window_labels(idx, rows, max_muts_per_sample=None, sample_filter_stdev=None, max_muts_per_elt_per_sample=None):
    """label per window (a list of N ints) for one cohort"""
    table, loads = sample_loads(idx, rows)
    gone = set()
    if sample_filter_stdev:
        limit = stdev(list(loads.values())) * sample_filter_stdev
        gone |= {s for s, n in loads.items() if n > limit}
    if max_muts_per_sample:
        gone |= {s for s, n in loads.items() if n > max_muts_per_sample}
    per_window = {}
    for (name, samp), (snv, _indel) in table.items():
        if samp not in gone:
            per_window[name] = per_window.get(name, 0) + snv
    return [per_window.get('{}:{}-{}'.format(int(c), int(s), int(e)), 0) for c, s, e in idx]
