"""The distinct samples of the sliding windows of the per-base route (dig_tile_window_sample_keys, dig_tile_window_samples,
nb_model.nb_model_window_hits(window_samples=True)), stated in plain Python (DESIGN.md "Samples in sliding windows").  The yardstick
of test_window_samples_host.py, test_gpu_window_samples.py and test_gpu_window_samples_guarded.py; nothing here is computed by the
library.

n[(cohort, region, tile, sample)] is tile_samples_statement.counts_by_sample: the rows of a kept sample that count in a tile.  A region
has nv = min(n_valid, T) tiles (n_valid <= 0: none), and for a width m the windows of tile_windows_statement: n_windows = 0 when
nv <= 0, else max(nv - m + 1, 1); window t covers the tiles t .. min(t + m, nv) - 1.  Then
    s_w[c][r][t] = len({s : n[(c, r, u, s)] > 0 for a tile u of window t})        for t < n_windows, else 0.
`window_counts_row` says that with one `set` per window.  `interval_differences` states the library's algorithm (a tile is the FIRST
tile of its sample in the windows [lo, hi)), and `window_counts_row_marked` marks, per sample, the windows that hold one of its tiles
in a bool array -- a form that takes milliseconds on rows of 10 000 tiles.  test_window_samples_host.py checks the three against
each other."""
import numpy as np

import tile_samples_statement as SS
import tile_windows_statement as WS

NO_KEY = (1 << 63) - 1                 # INT64_MAX: a pair that counts nowhere


def window_counts_row(tiles_by_sample, n_valid, T, m):
    """s_w of one row as a list of T ints.  tiles_by_sample: dict sample -> the tiles (any iterable) in which it has a counted row."""
    nv, nw = max(min(int(n_valid), T), 0), WS.n_windows(n_valid, T, m)
    at = {}                                                    # tile -> its samples
    for s, tiles in tiles_by_sample.items():
        for t in tiles:
            if 0 <= t < nv:
                at.setdefault(t, set()).add(s)
    out = [0] * T
    for t in range(nw):
        here = set()
        for u in range(t, min(t + m, nv)):
            here |= at.get(u, set())
        out[t] = len(here)
    return out


def interval_differences(tiles_by_sample, n_valid, T, m):
    """The difference array of one row as the library forms it: tile t of a sample whose previous tile is t_prev (-1: none) adds +1 at
    lo = max(t_prev + 1, t - m + 1, 0) and -1 at hi = min(t + 1, n_windows) (when hi < T), nothing when lo >= hi."""
    nv, nw = max(min(int(n_valid), T), 0), WS.n_windows(n_valid, T, m)
    d = [0] * T
    for s, tiles in tiles_by_sample.items():
        t_prev = -1
        for t in sorted(set(u for u in tiles if 0 <= u < nv)):
            lo, hi = max(t_prev + 1, t - m + 1, 0), min(t + 1, nw)
            if lo < hi:
                d[lo] += 1
                if hi < T:
                    d[hi] -= 1
            t_prev = t
    return d


def prefix_sums(d):
    out, run = [], 0
    for x in d:
        run += x
        out.append(run)
    return out


def window_counts_row_marked(tiles_by_sample, n_valid, T, m):
    """window_counts_row through one bool array per sample: the windows [t - m + 1, t] (cut to [0, n_windows)) hold tile t."""
    nv, nw = max(min(int(n_valid), T), 0), WS.n_windows(n_valid, T, m)
    out = np.zeros(T, np.int64)
    for s, tiles in tiles_by_sample.items():
        holds = np.zeros(T, bool)
        for t in tiles:
            if 0 <= t < nv:
                holds[max(t - m + 1, 0):min(t + 1, nw)] = True
        out += holds
    return [int(x) for x in out]


def tiles_by_row(n):
    """counts_by_sample's dict -> dict (cohort, region) -> dict sample -> set of tiles."""
    rows = {}
    for (c, r, t, s), count in n.items():
        if count > 0:
            rows.setdefault((c, r), {}).setdefault(s, set()).add(t)
    return rows


def window_sample_planes(n, C, n_valid, T, m, marked=False):
    """s_w int32 [C, R, T] from counts_by_sample's dict; marked: the bool-array form (long rows)."""
    R = len(n_valid)
    rows = tiles_by_row(n)
    form = window_counts_row_marked if marked else window_counts_row
    out = np.zeros((C, R, T), np.int32)
    for (c, r), by_sample in rows.items():
        out[c, r] = form(by_sample, n_valid[r], T, m)
    return out


def window_sample_counts(regions, rows, C, binsize, n_tiles, m, keep=None):
    """s_w int32 [C, R, n_tiles] from regions and rows as tile_samples_statement takes them."""
    n = SS.counts_by_sample(regions, rows, C, binsize, n_tiles, keep)
    return window_sample_planes(n, C, [reg[4] for reg in regions], n_tiles, m)


# ---- the keys, as integer arithmetic ------------------------------------------------------------------------------------------------
def sample_bits(n_samples):
    """The bits that hold the values 0 .. n_samples (at least one): the sample field of either key."""
    b = 1
    while b < 62 and (1 << b) < n_samples + 1:
        b += 1
    return b


def tile_major_keys(n, R, T, sb):
    """The keys of dig_tile_sample_keys for counts_by_sample's dict, one per counted row, ascending."""
    return sorted(k for (c, r, t, s), count in n.items() for k in [(((c * R + r) * T + t) << sb) | s] * count)


def rekey(key, T, sb, slots):
    """dig_tile_window_sample_keys of one key: ((row T + tile) << sb) | sample -> ((row << sb) | sample) T + tile."""
    if key < 0 or key == NO_KEY or (key >> sb) >= slots:
        return NO_KEY
    slot, sample = key >> sb, key & ((1 << sb) - 1)
    row, tile = divmod(slot, T)
    return ((row << sb) | sample) * T + tile


# ---- hand-worked cases: name -> (tiles_by_sample, n_valid, T, m, differences, s_w) ---------------------------------------------------
HAND_CASES = {
    # sample A in the tiles 1, 2, 6, sample B in tile 2; width 3 of 8 tiles: six windows
    "two samples": ({"A": [1, 2, 6], "B": [2]}, 8, 8, 3, [2, 0, 0, -2, 1, 0, -1, 0], [2, 2, 2, 0, 1, 1, 0, 0]),
    # a region with fewer tiles than the width: ONE window; tile 0 gives [0, 1), tile 1 an empty interval
    "short region": ({"A": [0, 1]}, 2, 8, 3, [1, -1, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0]),
    # one sample with tiles m - 1, m and m + 1 apart (m = 3: 0, 2, 5, 9): the windows of 0 and 2 overlap, those of 2 and 5 touch,
    # between those of 5 and 9 lies window 6, which holds none of them
    "gaps around the width": ({"A": [0, 2, 5, 9]}, 12, 12, 3, [1, 0, 0, 0, 0, 0, -1, 1, 0, 0, -1, 0], [1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 0, 0]),
    # width 1: the tiles themselves; a tile at n_valid counts nowhere
    "width one": ({"A": [0, 3], "B": [3, 4]}, 4, 5, 1, [1, -1, 0, 2, -2], [1, 0, 0, 2, 0]),
    # the last window is the row's last tile (width 1, n_valid = T): the interval ends at T and no -1 is written
    "row end": ({"A": [7]}, 8, 8, 1, [0, 0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0, 0, 1]),
    "no tiles": ({"A": [0]}, 0, 4, 2, [0, 0, 0, 0], [0, 0, 0, 0]),
}
