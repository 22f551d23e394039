"""The sparse sliding-window scan stated in plain Python (DESIGN.md "Sparse sliding windows"): sets and loops, one window and one
position at a time.  The yardstick of test_sparse_windows_host.py, test_gpu_sparse_windows.py and test_gpu_sparse_windows_guarded.py.
Regions, tables, rows and the position rule are those of sparse_tiles_statement.py.

With nv = min(n_valid, T) tiles in a region and m the width: n_windows = 0 when nv <= 0, else max(nv - m + 1, 1); window w covers the
tiles w .. min(w + m, nv) - 1 (a region with fewer than m tiles has one window over all of them).  A mutated window of a row (cohort,
region) is a window below n_windows that covers a tile with a mutation row of that cohort.
"""
import sparse_tiles_statement as T1


def n_windows(nv, m):
    return 0 if nv <= 0 else max(nv - m + 1, 1)


def window_tiles(w, nv, m):
    return range(w, min(w + m, nv))


# ---- the mutated windows of one row ----------------------------------------------------------------------------------------------
def mutated_windows(tiles, nv, m):
    """Brute force: the windows below n_windows that cover one of `tiles` (tiles at or past nv count nowhere)."""
    tiles = set(t for t in tiles if 0 <= t < nv)
    return set(w for w in range(n_windows(nv, m)) if any(t in tiles for t in window_tiles(w, nv, m)))


def k_window(k_by_tile, w, nv, m):
    """The rows of window w: k_by_tile is dict tile -> rows."""
    return sum(k_by_tile.get(t, 0) for t in window_tiles(w, nv, m))


def owned(t_prev, t, nv, m):
    """[lo, hi): the windows whose FIRST mutated tile is t, when the mutated tile in front of it in the row is t_prev (-1: none)."""
    return max(t_prev + 1, t - m + 1, 0), min(t + 1, n_windows(nv, m))


def windows_by_owner(tiles, nv, m):
    """The enumeration of the kernels: every mutated tile in ascending order names the windows it owns.  A list (with repeats, if the
    rule were wrong) in the order the flat list has."""
    out, t_prev = [], -1
    for t in sorted(set(t for t in tiles if 0 <= t < nv)):
        lo, hi = owned(t_prev, t, nv, m)
        out.extend(range(lo, hi))
        t_prev = t
    return out


def counts_from_keys(keys, T, nv_by_row, m):
    """dig_sparse_window_count on a sorted key list, key = row T + tile: (counts per key, the flat list of (row, window)).  The head
    of a run of equal keys reads its predecessor from its left neighbour: the same row iff prev // T == key // T."""
    counts, flat = [], []
    for i, key in enumerate(keys):
        n = 0
        if 0 <= key < len(nv_by_row) * T and (i == 0 or keys[i - 1] != key):
            row, t = divmod(key, T)
            nv = min(nv_by_row[row], T)
            if t < nv:
                prev = keys[i - 1] if i > 0 else -1
                t_prev = prev - row * T if prev >= 0 and prev // T == row else -1
                lo, hi = owned(t_prev, t, nv, m)
                n = max(hi - lo, 0)
                flat.extend((row, w) for w in range(lo, hi))
        counts.append(n)
    return counts, flat


# ---- the windows with a positive tile --------------------------------------------------------------------------------------------
def positive_windows_brute(positive, nv, m):
    """The windows below n_windows that cover a tile of `positive`."""
    return len(mutated_windows(positive, nv, m))


def positive_windows_runs(positive, nv, m):
    """The closed form of dig_tile_window_census: n_windows minus, over the maximal runs of Z consecutive tiles outside `positive`,
    max(Z - m + 1, 0); below m tiles one window, counted when any tile is positive."""
    positive = set(t for t in positive if 0 <= t < nv)
    if nv <= 0:
        return 0
    if nv < m:
        return 1 if positive else 0
    zero_w, run = 0, 0
    for t in range(nv + 1):
        if t < nv and t not in positive:
            run += 1
        else:
            zero_w += max(run - m + 1, 0)
            run = 0
    return n_windows(nv, m) - zero_w


def positive_tiles(seqs, regions, tables, n_up, binsize, n_tiles):
    """[C][R] sets: the tiles below n_valid that hold a window whose table entry is > 0 (the rule of n_positive), and n_valid [R]."""
    out = [[set() for _ in regions] for _ in tables]
    n_valid = []
    for r, region in enumerate(regions):
        first, n_pos = T1.region_positions(seqs, region, n_up)
        tiles = min((n_pos + binsize - 1) // binsize, n_tiles)
        n_valid.append(tiles)
        for i in range(min(n_pos, tiles * binsize)):
            ctx = T1.context(seqs[region[0]], first + i, n_up)
            if ctx is not None:
                for c, table in enumerate(tables):
                    if table[ctx] > 0:
                        out[c][r].add(i // binsize)
    return out, n_valid


def window_census(seqs, regions, tables, n_up, binsize, n_tiles, m):
    """(n_windows [R], n_positive_w [C][R]); the brute-force count and the run form are compared on the way."""
    positive, n_valid = positive_tiles(seqs, regions, tables, n_up, binsize, n_tiles)
    npw = [[positive_windows_brute(positive[c][r], n_valid[r], m) for r in range(len(regions))] for c in range(len(tables))]
    runs = [[positive_windows_runs(positive[c][r], n_valid[r], m) for r in range(len(regions))] for c in range(len(tables))]
    assert npw == runs, (npw, runs)
    return [n_windows(nv, m) for nv in n_valid], npw


# ---- the mutated windows of a problem --------------------------------------------------------------------------------------------
def window_sum(seqs, region, table, n_up, binsize, w, nv, m):
    """The sum of the table over the window's positions in ascending order, valid contexts only, started at 0.0."""
    first, n_pos = T1.region_positions(seqs, region, n_up)
    total = 0.0
    for i in range(w * binsize, min(min(w + m, nv) * binsize, n_pos)):
        ctx = T1.context(seqs[region[0]], first + i, n_up)
        if ctx is not None:
            total += table[ctx]
    return total


def mutated_window_table(seqs, regions, rows, tables, n_up, binsize, n_tiles, m):
    """dict (cohort, region, window) -> (k_w, pt_w) over the mutated windows: pt_w = the window's sum / denom, ONE division (NaN for
    denom == 0).  The windows of every row come from the brute-force set; the enumeration by owners must name the same, each once."""
    first_pos, n_valid, denom, _ = T1.census(seqs, regions, tables, n_up, binsize, n_tiles)
    k = {}
    for (c, r, t), (n, _) in T1.mutated_tiles(seqs, regions, rows, tables, n_up, binsize, n_tiles).items():
        k.setdefault((c, r), {})[t] = n
    out = {}
    for (c, r), by_tile in k.items():
        nv = min(n_valid[r], n_tiles)
        wins = mutated_windows(by_tile, nv, m)
        assert windows_by_owner(by_tile, nv, m) == sorted(wins)
        for w in wins:
            total = window_sum(seqs, regions[r], tables[c], n_up, binsize, w, nv, m)
            out[(c, r, w)] = (k_window(by_tile, w, nv, m), total / denom[c][r] if denom[c][r] != 0 else float("nan"))
    return out


# ---- hand-worked cases -----------------------------------------------------------------------------------------------------------
# one row: (nv, m, mutated tiles) -> (mutated windows, owned intervals in tile order)
HAND_ROWS = {
    # T = nv = 8, m = 3: windows 0 .. 5; tile 1 is the first mutated tile of 0, 1; tile 2 of 2; tile 6 of 4, 5.  Window 3 (tiles 3-5): none
    "three_tiles": dict(nv=8, m=3, tiles=[1, 2, 6], windows={0, 1, 2, 4, 5}, owned=[(0, 2), (2, 3), (4, 6)], k={1: 2, 2: 1, 6: 5},
                        k_w={0: 3, 1: 3, 2: 1, 4: 5, 5: 5}),
    # fewer tiles than the width: the single window over both
    "short_region": dict(nv=2, m=3, tiles=[1], windows={0}, owned=[(0, 1)], k={1: 4}, k_w={0: 4}),
    # a mutated tile in the LAST tile with nv >= m: the last window (nv - m) holds it, hi is cut at n_windows
    "last_tile": dict(nv=8, m=3, tiles=[7], windows={5}, owned=[(5, 6)], k={7: 1}, k_w={5: 1}),
    # a tile at nv (of the next row's key space) counts nowhere
    "no_region": dict(nv=0, m=2, tiles=[0], windows=set(), owned=[], k={}, k_w={}),
}
# two rows next to each other in the key order, T = 8: the last tile of row 0 and the first tile of row 1.  The keys 7 and 8 are
# neighbours, but 7 / 8 != 8 / 8: tile 0 of row 1 has no predecessor, its windows start at 0.
HAND_NEIGHBOUR_ROWS = dict(T=8, m=3, nv=[8, 8], keys=[7, 8], counts=[1, 1], windows=[(0, 5), (1, 0)])
