"""The copy-number training labels (DataExtractor addObjectives --cnv) stated per base in plain numpy: for every window a difference
track over its W positions, its cumulative sum, and the mean -- the yardstick for shapes the reference golden
(tests/golden/make_cnv_golden.py) is too small for, itself pinned to that golden by tests/test_cnv_objectives_host.py.

A window is [s, s + W).  A segment (chromosome, start, end, cp_num) of the window's chromosome overlaps it iff start < s + W and
end > s; it then covers the positions max(start, s) .. min(end, s + W) - 1 and adds there
    cp_num == 2: 1 to column 1 (copy-neutral / LOH)      cp_num < 2: 2 - cp_num to column 2 (deletions)
    cp_num > 2: cp_num - 2 to column 0 (duplications).
Nothing is de-duplicated; windows are taken one by one, so their order, repeats and overlaps cannot matter."""
import numpy as np


def class_and_weight(cp_num):
    cp = np.asarray(cp_num, np.int64)
    return np.where(cp == 2, 1, np.where(cp < 2, 2, 0)), np.where(cp == 2, 1, np.abs(cp - 2))


def window_means(win_chrom, win_start, W, seg_chrom, seg_start, seg_end, seg_cp, seg_cohort, C):
    """labels float64 [N, 3, C]; every argument an integer array (chromosomes as ids)."""
    win_chrom, win_start = np.asarray(win_chrom, np.int64), np.asarray(win_start, np.int64)
    seg_chrom, seg_start, seg_end, seg_cohort = (np.asarray(x, np.int64) for x in (seg_chrom, seg_start, seg_end, seg_cohort))
    col, wt = class_and_weight(seg_cp)
    out = np.zeros((len(win_chrom), 3, C))
    for i, (ch, s) in enumerate(zip(win_chrom.tolist(), win_start.tolist())):
        hit = np.flatnonzero((seg_chrom == ch) & (seg_start < s + W) & (seg_end > s))
        track = np.zeros((W + 1, 3, C), np.int64)                       # (row W: where a segment that runs through the window ends)
        first = np.maximum(seg_start[hit], s) - s
        behind = np.minimum(seg_end[hit], s + W) - s
        np.add.at(track, (first, col[hit], seg_cohort[hit]), wt[hit])
        np.subtract.at(track, (behind, col[hit], seg_cohort[hit]), wt[hit])
        out[i] = np.mean(np.cumsum(track[:W], axis=0), axis=0)
    return out


def rows_as_arrays(cohorts, chrom_ids):
    """Text rows (chr, start, end, cp_num, ...) of several cohorts -> (chrom, start, end, cp_num, cohort) integer arrays; a row
    whose chromosome label is no key of chrom_ids (label -> id, compared as text) is left out."""
    cols = [[], [], [], [], []]
    for c, rows in enumerate(cohorts):
        for r in rows:
            if r[0] in chrom_ids:
                for dst, v in zip(cols, (chrom_ids[r[0]], int(r[1]), int(r[2]), int(float(r[3])), c)):
                    dst.append(v)
    return [np.array(x, np.int64) for x in cols]
