"""The counts by sample of the per-base route, stated in plain Python (DESIGN.md "Samples in the per-base route"): dictionaries and
loops, one row at a time.  The yardstick of test_tile_samples_host.py, test_gpu_tile_samples.py and
test_gpu_tile_samples_guarded.py.

Regions: a list of (chrom, start, end, first_pos, n_valid) -- chromosome label, the half-open interval the rows are joined with, and
what base_tile_probs says about the region.  Rows: a list of (chrom, start, end, cohort, sample) with `sample` the GLOBAL sample.
A row is paired with every region of its chromosome that its interval [start, end) overlaps (a zero-length region counts as one
base); a pair COUNTS for tile t = (start - first_pos) // binsize of its region unless
    start < first_pos,  or  t >= n_valid (or t >= n_tiles),  or  the cohort is outside [0, C),  or  keep[sample] == 0.
n[(cohort, region, tile, sample)] is the number of pairs that count there.
"""


def pair_tile(row, region, binsize, n_tiles, C, keep=None):
    """The (cohort, tile, sample) one (row, region) pair counts for, or None."""
    chrom, start, end, cohort, sample = row
    r_chrom, r_start, r_end, first, n_valid = region
    if r_end == r_start:
        r_end = r_start + 1
    if chrom != r_chrom or not (start < r_end and end > r_start):
        return None                                            # not a pair of the join
    if start < first:
        return None
    t = (start - first) // binsize
    if t >= n_valid or t >= n_tiles:
        return None
    if cohort < 0 or cohort >= C:
        return None
    if keep is not None and not keep[sample]:
        return None
    return cohort, t, sample


def counts_by_sample(regions, rows, C, binsize, n_tiles, keep=None):
    """n: dict (cohort, region, tile, sample) -> rows."""
    n = {}
    for row in rows:
        for r, region in enumerate(regions):
            at = pair_tile(row, region, binsize, n_tiles, C, keep)
            if at is not None:
                key = (at[0], r, at[1], at[2])
                n[key] = n.get(key, 0) + 1
    return n


def tile_sample_counts(regions, rows, C, binsize, n_tiles, keep=None, cap=None):
    """(k_cap, k_samples): nested lists [C][R][n_tiles].  k_cap = sum over the samples of min(n, cap) (cap None: of n), k_samples =
    the samples with n > 0."""
    R = len(regions)
    k_cap = [[[0] * n_tiles for _ in range(R)] for _ in range(C)]
    k_samples = [[[0] * n_tiles for _ in range(R)] for _ in range(C)]
    for (c, r, t, _), n in counts_by_sample(regions, rows, C, binsize, n_tiles, keep).items():
        k_cap[c][r][t] += n if cap is None else min(n, cap)
        k_samples[c][r][t] += 1
    return k_cap, k_samples


def keep_from_max_muts(row_samples, n_samples, max_muts_per_sample):
    """keep [n_samples]: 0 for a sample with MORE than max_muts_per_sample rows (None: nobody is dropped)."""
    total = [0] * n_samples
    for s in row_samples:
        total[s] += 1
    return [1 if max_muts_per_sample is None or total[s] <= max_muts_per_sample else 0 for s in range(n_samples)]


def thinned_rows(regions, rows, C, binsize, n_tiles, keep=None, cap=None):
    """The rows a host would leave in the file so that the row-counting route (dig_tile_mut_counts) gives k_cap: the rows of dropped
    samples removed, and of every (cohort, region, tile, sample) only the first min(n, cap) rows.  Rows that count nowhere stay.
    For regions that do not overlap (a row then counts in at most one tile).  Returns the indices of the rows that stay."""
    seen, stay = {}, []
    for i, row in enumerate(rows):
        if keep is not None and not keep[row[4]]:
            continue
        where = [(r, pair_tile(row, region, binsize, n_tiles, C, keep)) for r, region in enumerate(regions)]
        where = [(r, at) for r, at in where if at is not None]
        assert len(where) <= 1, "thinned_rows is stated for regions that do not overlap"
        if where:
            r, (c, t, s) = where[0]
            seen[(c, r, t, s)] = seen.get((c, r, t, s), 0) + 1
            if cap is not None and seen[(c, r, t, s)] > cap:
                continue
        stay.append(i)
    return stay


# ---- hand-worked cases: (regions, rows, C, binsize, n_tiles, keep, cap, k_cap, k_samples) ---------------------------------------------
# one region chr1:[100, 130), first position 100, 3 tiles of 10
_REG = [("1", 100, 130, 100, 3)]
HAND_CASES = {
    # sample 0 five times in tile 0, sample 1 once in tile 0 and once in tile 2: OBS 6 -> capped at 2: 2 + 1
    "cap": (_REG, [("1", 100 + i, 101 + i, 0, 0) for i in range(5)] + [("1", 109, 110, 0, 1), ("1", 125, 126, 0, 1)], 1, 10, 3, None, 2,
            [[[3, 0, 1]]], [[[2, 0, 1]]]),
    # the same without a cap: the plain row count
    "no_cap": (_REG, [("1", 100 + i, 101 + i, 0, 0) for i in range(5)] + [("1", 109, 110, 0, 1), ("1", 125, 126, 0, 1)], 1, 10, 3, None,
               None, [[[6, 0, 1]]], [[[2, 0, 1]]]),
    # sample 0 dropped: only sample 1 is left
    "dropped": (_REG, [("1", 100 + i, 101 + i, 0, 0) for i in range(5)] + [("1", 109, 110, 0, 1), ("1", 125, 126, 0, 1)], 1, 10, 3, [0, 1],
                None, [[[1, 0, 1]]], [[[1, 0, 1]]]),
    # the skip rules: START in front of the region (a multi-base row that overlaps it), a tile at n_valid (n_valid 2 of 3 tiles), a
    # cohort outside [0, 2), another chromosome; cohort 1's sample 2 counts once
    "skips": ([("1", 100, 130, 100, 2)], [("1", 98, 103, 0, 0), ("1", 120, 121, 0, 0), ("1", 105, 106, 2, 0), ("1", 105, 106, -1, 0),
                                           ("2", 105, 106, 0, 0), ("1", 119, 120, 1, 2)], 2, 10, 3, None, 1,
              [[[0, 0, 0]], [[0, 1, 0]]], [[[0, 0, 0]], [[0, 1, 0]]]),
    # two adjacent regions and a row across their border: it counts in the region that holds its START
    "border": ([("1", 100, 110, 100, 1), ("1", 110, 120, 110, 1)], [("1", 108, 113, 0, 0), ("1", 110, 111, 0, 0), ("1", 111, 112, 0, 0)],
               1, 10, 1, None, 1, [[[1], [1]]], [[[1], [1]]]),
}
