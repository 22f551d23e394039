"""The plain statement of engine.sequence_counts (dig_overlap_join_* + dig_sequence_counts) in numpy, nothing shared with the product:
a row counts once, under (its cohort, its type), when at least one window overlaps it and its type is a table row.  Also the rule
that makes the per-window genome counts of the sequence-model tests (tests/golden/make_sequence_models_golden.py uses it too)."""
import numpy as np


def sequence_counts(win_chrom, win_start, win_end, row_chrom, row_start, row_end, row_type, row_cohort, K, C):
    wc, ws, we, rc, rs, re, rt, rk = (np.asarray(x, np.int64) for x in (win_chrom, win_start, win_end, row_chrom, row_start, row_end,
                                                                         row_type, row_cohort))
    we, re = np.where(we == ws, ws + 1, we), np.where(re == rs, rs + 1, re)      # an empty interval: its first base, as in the join
    hit = np.zeros(len(rc), bool)
    for c, s, e in zip(wc, ws, we):
        hit |= (rc == c) & (rs < e) & (s < re)
    counts = np.zeros((C, K), np.int64)
    sel = hit & (rt < K)
    np.add.at(counts, (rk[sel], rt[sel]), 1)
    return counts


def genome_frame(n_windows, contexts):
    """all_window_genome_counts of the tests: a row per window, a column per context, every entry 1 .. 101."""
    import pandas as pd
    w, j = np.arange(n_windows)[:, None], np.arange(len(contexts))[None, :]
    return pd.DataFrame(1 + (7 * w + 13 * j) % 101, columns=list(contexts))
