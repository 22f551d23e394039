"""The sparse per-base scan stated in plain Python (DESIGN.md "Sparse per-base scan"): dictionaries and loops, one position and one
row at a time.  The yardstick of test_sparse_tiles_host.py, test_gpu_sparse_tiles.py and test_gpu_sparse_tiles_guarded.py.

seqs: dict chromosome label -> sequence.  regions: a list of (chrom, start, end).  tables: per cohort a dict context -> S_prob (the
(2 n_up + 1)-mers in ACGT).  rows: a list of (chrom, start, end, cohort).

A region's positions (fetch_sequence, sequence_tools.py:21-29): first = n_up when start == 0, else start; they run to
min(end, len - n_up).  Tile t holds the positions first + t binsize .. ; a position whose window holds a letter other than ACGT adds
nothing.  denom[c][r] = the sum of the table over the region's positions, pt of a tile = its sum / denom.
"""
import math


def region_positions(seqs, region, n_up):
    """(first position, number of positions)."""
    chrom, start, end = region
    first = n_up if start == 0 else start
    stop = min(end, len(seqs[chrom]) - n_up)
    return first, max(stop - first, 0)


def context(seq, p, n_up):
    """The window of position p, or None when it holds a letter other than ACGT."""
    win = seq[p - n_up:p + n_up + 1].upper()
    return win if len(win) == 2 * n_up + 1 and all(ch in "ACGT" for ch in win) else None


def census(seqs, regions, tables, n_up, binsize, n_tiles):
    """(first_pos [R], n_valid [R], denom [C][R], n_positive [C][R]) -- n_positive: the tiles below n_valid that hold a window whose
    table entry is > 0."""
    C = len(tables)
    first_pos, n_valid = [], []
    denom = [[0.0] * len(regions) for _ in range(C)]
    n_positive = [[0] * len(regions) for _ in range(C)]
    for r, region in enumerate(regions):
        first, n_pos = region_positions(seqs, region, n_up)
        tiles = min((n_pos + binsize - 1) // binsize, n_tiles)
        first_pos.append(first)
        n_valid.append(tiles)
        seq = seqs[region[0]]
        for c in range(C):
            positive = set()
            for i in range(n_pos):
                ctx = context(seq, first + i, n_up)
                if ctx is not None:
                    denom[c][r] += tables[c][ctx]
                    if tables[c][ctx] > 0 and i // binsize < tiles:
                        positive.add(i // binsize)
            n_positive[c][r] = len(positive)
    return first_pos, n_valid, denom, n_positive


def pair_tile(row, region, first, n_valid, binsize, n_tiles, C):
    """The (cohort, tile) a (row, region) pair counts for, or None: the rules of dig_tile_mut_counts."""
    chrom, start, end, cohort = row
    r_chrom, r_start, r_end = region
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
    return cohort, t


def mutated_tiles(seqs, regions, rows, tables, n_up, binsize, n_tiles):
    """dict (cohort, region, tile) -> (k, pt): the tiles that hold a row, k = its rows, pt = the tile's sum in position order / denom
    (NaN for denom == 0)."""
    C = len(tables)
    first_pos, n_valid, denom, _ = census(seqs, regions, tables, n_up, binsize, n_tiles)
    k = {}
    for row in rows:
        for r, region in enumerate(regions):
            at = pair_tile(row, region, first_pos[r], n_valid[r], binsize, n_tiles, C)
            if at is not None:
                k[(at[0], r, at[1])] = k.get((at[0], r, at[1]), 0) + 1
    out = {}
    for (c, r, t), n in k.items():
        first, n_pos = region_positions(seqs, regions[r], n_up)
        total = 0.0
        for i in range(t * binsize, min((t + 1) * binsize, n_pos)):
            ctx = context(seqs[regions[r][0]], first + i, n_up)
            if ctx is not None:
                total += tables[c][ctx]
        out[(c, r, t)] = (n, total / denom[c][r] if denom[c][r] != 0 else float("nan"))
    return out


def gamma(mu, sigma):
    """(alpha, theta) = (mu^2 / sigma^2, sigma^2 / mu) with IEEE results for a zero divisor."""
    def div(a, b):
        if a != a or b != b:
            return float("nan")
        if b == 0:
            return float("nan") if a == 0 else math.copysign(float("inf"), a) * math.copysign(1.0, b)
        return a / b
    return div(mu * mu, sigma * sigma), div(sigma * sigma, mu)


def testable_region(mu, sigma):
    """An EMPTY tile with pt > 0 has a p-value: alpha a finite number > 0, theta a number > 0 (the NB mean is then > 0 = k and the
    lower tail is evaluated; otherwise the upper tail betainc(0, alpha, .) is NaN)."""
    alpha, theta = gamma(mu, sigma)
    return alpha == alpha and 0 < alpha < float("inf") and theta == theta and theta > 0


def mutated_tile_has_pvalue(k, pt, mu, sigma):
    """A tile with k >= 1 rows has a p-value: inside a testable region with pt > 0 always; with pt == 0 (every window holds an N)
    p = 1 and the upper tail is 0 whenever alpha is a finite number > 0 and theta is finite; never with pt NaN or in another region."""
    alpha, theta = gamma(mu, sigma)
    if pt != pt:
        return False
    if pt == 0:
        return alpha == alpha and 0 < alpha < float("inf") and theta == theta and abs(theta) < float("inf")
    return testable_region(mu, sigma)


def zero_floor(denom_c, smax, mu_c, sigma_c, binsize):
    """floor of one cohort: min over its testable regions with denom > 0 of (1 + theta u)^(-alpha), u = min(1, binsize smax / denom);
    +inf without such a region."""
    floor = float("inf")
    for d, m, s in zip(denom_c, mu_c, sigma_c):
        if d > 0 and testable_region(m, s):
            alpha, theta = gamma(m, s)
            u = min(1.0, binsize * smax / d)
            floor = min(floor, math.exp(-alpha * math.log1p(theta * u)))
    return floor


def n_testable(seqs, regions, rows, tables, mu, sigma, n_up, binsize, n_tiles):
    """Per cohort the existing tiles with a p-value: the tiles with pt > 0 of the testable regions, plus the mutated tiles outside that
    set that have one."""
    _, _, _, n_positive = census(seqs, regions, tables, n_up, binsize, n_tiles)
    out = [sum(n_positive[c][r] for r in range(len(regions)) if testable_region(mu[c][r], sigma[c][r])) for c in range(len(tables))]
    for (c, r, t), (k, pt) in mutated_tiles(seqs, regions, rows, tables, n_up, binsize, n_tiles).items():
        counted = testable_region(mu[c][r], sigma[c][r]) and pt > 0
        if not counted and mutated_tile_has_pvalue(k, pt, mu[c][r], sigma[c][r]):
            out[c] += 1
    return out


# ---- hand-worked cases -----------------------------------------------------------------------------------------------------
# one chromosome ACGNACGTAC (10 bases, an N at 3), n_up = 1, the region 1:0-10: first position 1, last 8 (a window must fit).
# The windows of 2, 3, 4 hold the N.  Valid: 1 ACG, 5 ACG, 6 CGT, 7 GTA, 8 TAC.
# Cohort 0: table 1 for a C in the middle, else 0.  Cohort 1: 2 everywhere.
def _tables():
    import itertools
    ctx = ["".join(t) for t in itertools.product("ACGT", repeat=3)]
    return [{k: (1.0 if k[1] == "C" else 0.0) for k in ctx}, {k: 2.0 for k in ctx}]


HAND = dict(
    seqs={"1": "ACGNACGTAC"}, regions=[("1", 0, 10)], tables=_tables(), n_up=1, binsize=2, n_tiles=4,
    # cohort 0 twice at 5 (tile 2), cohort 1 once at 3 (tile 1: both windows hold the N), one row of a cohort that does not exist
    rows=[("1", 5, 6, 0), ("1", 5, 6, 0), ("1", 3, 4, 1), ("1", 6, 7, 2)],
    mu=[[4.0], [2.0]], sigma=[[2.0], [2.0]],
    first_pos=[1], n_valid=[4],
    denom=[[2.0], [10.0]],                  # positions 1 and 5; five valid windows times 2
    n_positive=[[2], [3]],                  # tiles {1,2} {3,4} {5,6} {7,8}: C-centred windows in tiles 0 and 2; any valid window in 0, 2, 3
    tiles={(0, 0, 2): (2, 0.5), (1, 0, 1): (1, 0.0)},
    # cohort 0: alpha 4, theta 1, u = min(1, 2 * 1 / 2) = 1 -> 2^-4; cohort 1: alpha 1, theta 2, u = 2 * 2 / 10 -> 1 / 1.8
    floor=[0.0625, 1.0 / 1.8],
    n_testable=[2, 4],                      # cohort 1: its three tiles with pt > 0 and the mutated tile with pt = 0 (PVAL 0)
)
# the same region cut into tiles of 3 with room for two of them only: tile 2 (positions 7, 8) does not exist for the counts, the
# denominators still cover it; the row at 7 counts nowhere
HAND_CAPPED = dict(HAND, binsize=3, n_tiles=2, rows=[("1", 7, 8, 0), ("1", 1, 2, 0)], n_valid=[2], n_positive=[[2], [2]],
                   tiles={(0, 0, 0): (1, 0.5)}, floor=[0.0625, 1.0 / 2.2], n_testable=[2, 2])        # (cohort 1: u = 3 * 2 / 10)
# regions that are not testable: mu NaN, mu 0, sigma 0 -- no empty tile counts, and a mutated tile with pt > 0 has no p-value either
HAND_UNTESTABLE = dict(HAND, rows=[("1", 5, 6, 0), ("1", 3, 4, 1)], mu=[[float("nan")], [0.0]], floor=[float("inf"), float("inf")],
                       tiles={(0, 0, 2): (1, 0.5), (1, 0, 1): (1, 0.0)}, n_testable=[0, 0])
HAND_CASES = {"n_run": HAND, "capped": HAND_CAPPED, "untestable": HAND_UNTESTABLE}
