"""A plain statement of the sliding windows of the per-base route (dig_tile_window_test, nb_model.nb_model_window_hits), and the
hand-worked cases that pin it.  Nothing here is computed by the library.

One row (c, r) of the base planes holds the T tiles of a region: pt (float64) and k (integer counts); the region has nv =
min(n_valid[r], T) tiles (n_valid <= 0: none).  For a width m >= 1:
  n_windows       0 when nv <= 0, else max(nv - m + 1, 1)
  window t        covers the tiles t .. min(t + m, nv) - 1: full windows only, or ONE window over all tiles of a region with fewer than m
  pt_w[t]         the window's pt values added LEFT TO RIGHT in float64, the first term taken as it is: ((pt[t] + pt[t + 1]) + ...)
  k_w[t]          the integer sum
  t >= n_windows  pt_w NaN, k_w 0
`window_row` says it term by term in plain Python; `window_planes` says the same for whole planes -- per row, one vector addition
per step j = 1 .. m - 1 that adds term t + j to every window t at once: every window's additions happen in the same left-to-right
order (IEEE float64 addition is the same operation in numpy and in Python) -- so that a row of 10 000 tiles at width 1 024 takes
milliseconds.  test_tile_windows_host.py checks the two against each other.

The hits: per cohort and width, the windows t < n_windows with PVAL <= pval_max, or with a Benjamini-Hochberg q <= fdr over that
width's windows whose p-value is a number; `peaks` marks the hits that no better hit of the same region overlaps."""
import numpy as np

NAN = float("nan")


def n_windows(n_valid, T, m):
    nv = min(int(n_valid), int(T))
    return 0 if nv <= 0 else max(nv - m + 1, 1)


def window_row(pt, k, n_valid, m):
    """(pt_w, k_w, n_windows) of one row: pt, k lists of T values."""
    T = len(pt)
    nv, nw = max(min(int(n_valid), T), 0), n_windows(n_valid, T, m)
    pt_w, k_w = [NAN] * T, [0] * T
    for t in range(nw):
        s, n = pt[t], k[t]
        for j in range(t + 1, min(t + m, nv)):
            s = s + pt[j]
            n = n + k[j]
        pt_w[t], k_w[t] = s, n
    return pt_w, k_w, nw


def window_planes(pt, k, n_valid, m):
    """(pt_w f64 [C, R, T], k_w i32 [C, R, T], n_windows i32 [R]) of whole planes (numpy arrays)."""
    pt, k = np.asarray(pt, np.float64), np.asarray(k, np.int32)
    C, R, T = pt.shape
    pt_w, k_w = np.full((C, R, T), np.nan), np.zeros((C, R, T), np.int32)
    nwin = np.array([n_windows(v, T, m) for v in n_valid], np.int32)
    for r in range(R):
        nv, nw = max(min(int(n_valid[r]), T), 0), int(nwin[r])
        if nw == 0:
            continue
        length = min(m, nv)                              # of every window of the region: nw > 1 only with full windows
        acc, cnt = pt[:, r, :nw].copy(), k[:, r, :nw].astype(np.int64)
        for j in range(1, length):
            acc = acc + pt[:, r, j:j + nw]
            cnt = cnt + k[:, r, j:j + nw]
        pt_w[:, r, :nw], k_w[:, r, :nw] = acc, cnt.astype(np.int32)
    return pt_w, k_w, nwin


def peaks(region, tile, score, m):
    """PEAK of the hits of one cohort at one width: per region, the hits in the order of (score, tile); a hit is a peak unless a hit
    already marked as a peak overlaps it (|t1 - t2| < m)."""
    out = [False] * len(tile)
    for i in sorted(range(len(tile)), key=lambda i: (region[i], score[i], tile[i])):
        if not any(out[j] and region[j] == region[i] and abs(tile[j] - tile[i]) < m for j in range(len(tile))):
            out[i] = True
    return out


def q_values(p):
    """Benjamini-Hochberg q-values of a list of numbers (statsmodels' operations: p / (rank / n), running minimum from behind, cap 1)."""
    p = np.asarray(p, np.float64)
    n = len(p)
    if n == 0:
        return p.copy()
    order = np.argsort(p, kind="stable")
    q = p[order] / (np.arange(1, n + 1) / float(n))
    q = np.minimum(np.minimum.accumulate(q[::-1])[::-1], 1.0)
    out = np.empty(n)
    out[order] = q
    return out


def window_hits(idx, mu, sigma, first, n_pos, n_valid, binsize, widths, planes, pval_max=None, fdr=None):
    """The frame of one cohort as a dict of columns (lists / arrays in row order), its index and its attrs.  idx [R, 3]; mu, sigma,
    first, n_pos, n_valid [R]; planes: per width dict(pt, k, exp, pval [R, T], n_windows [R]) -- the cohort's full window planes."""
    names = ["CHROM", "POS", "OBS", "EXP", "PVAL", "Pi", "MU", "SIGMA", "REGION", "WIDTH", "PEAK"] + (["QVAL"] if fdr is not None else [])
    cols, index, n_testable, n_win = {n: [] for n in names}, [], [], []
    T = len(planes[0]["pval"][0]) if len(idx) else 0
    for m, pl in zip(widths, planes):
        rows = [(r, t) for r in range(len(idx)) for t in range(int(pl["n_windows"][r]))]
        p = np.array([pl["pval"][r][t] for r, t in rows], np.float64)
        number = ~np.isnan(p)
        q = np.full(len(rows), np.nan)
        q[number] = q_values(p[number])
        hit = (q <= fdr) if fdr is not None else (p <= pval_max)
        at = [i for i in range(len(rows)) if hit[i]]
        pk = peaks([rows[i][0] for i in at], [rows[i][1] for i in at], [p[i] for i in at], m)
        for i, is_peak in zip(at, pk):
            r, t = rows[i]
            nv = max(min(int(n_valid[r]), T), 0)
            lo = int(first[r]) + t * binsize
            hi = min(lo + min(m, nv - t) * binsize, int(first[r]) + int(n_pos[r])) - 1
            vals = [float(idx[r][0]), (lo + hi) / 2.0, float(pl["k"][r][t]), pl["exp"][r][t], p[i], pl["pt"][r][t], mu[r], sigma[r],
                    "{}:{}-{}".format(*idx[r]), float(hi - lo + 1), bool(is_peak)] + ([q[i]] if fdr is not None else [])
            for n, v in zip(names, vals):
                cols[n].append(v)
            index.append(i)
        n_testable.append(int(number.sum()))
        n_win.append(len(rows))
    return cols, index, dict(n_testable=n_testable, n_windows=n_win)


# ---- hand-worked cases: name -> (pt, k, n_valid, m, pt_w, k_w, n_windows) ---------------------------------------------------------
_PT = [0.1, 0.2, 0.3, 0.4, NAN]
HAND_CASES = {
    # width 1: the tiles themselves; the tile behind n_valid stays NaN / 0 whatever it held
    "width one": (_PT, [1, 0, 2, 0, 9], 4, 1, [0.1, 0.2, 0.3, 0.4, NAN], [1, 0, 2, 0, 0], 4),
    # width 2 of 4 tiles: three full windows
    "pairs": (_PT, [1, 0, 2, 0, 9], 4, 2, [0.1 + 0.2, 0.2 + 0.3, 0.3 + 0.4, NAN, NAN], [1, 2, 2, 0, 0], 3),
    # width 3 does not divide 4: two windows
    "triples": (_PT, [1, 0, 2, 5, 9], 4, 3, [(0.1 + 0.2) + 0.3, (0.2 + 0.3) + 0.4, NAN, NAN, NAN], [3, 7, 0, 0, 0], 2),
    # width = the tiles of the region: one window
    "all": (_PT, [1, 0, 2, 5, 9], 4, 4, [((0.1 + 0.2) + 0.3) + 0.4, NAN, NAN, NAN, NAN], [8, 0, 0, 0, 0], 1),
    # a region with fewer tiles than the width: ONE window over all of them
    "short region": (_PT, [1, 0, 2, 5, 9], 4, 7, [((0.1 + 0.2) + 0.3) + 0.4, NAN, NAN, NAN, NAN], [8, 0, 0, 0, 0], 1),
    # the order of the additions shows: (1e16 + 1) + 1 = 1e16, while 1e16 + (1 + 1) = 1e16 + 2
    "left to right": ([1e16, 1.0, 1.0], [0, 0, 0], 3, 3, [1e16, NAN, NAN], [0, 0, 0], 1),
    "right to left would differ": ([1.0, 1.0, 1e16], [0, 0, 0], 3, 3, [1e16 + 2.0, NAN, NAN], [0, 0, 0], 1),
    # a region without tiles, by 0 and by a negative n_valid; n_valid above T counts as T
    "no tiles": ([0.5, 0.5], [3, 3], 0, 1, [NAN, NAN], [0, 0], 0),
    "negative n_valid": ([0.5, 0.5], [3, 3], -2, 2, [NAN, NAN], [0, 0], 0),
    "n_valid above T": ([0.5, 0.25], [3, 4], 5, 2, [0.75, NAN], [7, 0], 1),
    # a NaN or a zero inside a window goes through the sum as IEEE says
    "nan term": ([0.5, NAN, 0.25, 0.0], [1, 1, 1, 1], 4, 2, [NAN, NAN, 0.25, NAN], [2, 2, 2, 0], 3),
}
assert (1e16 + 1.0) + 1.0 == 1e16 and 1e16 + 2.0 != 1e16

# PEAK: name -> (region, tile, score, m, peaks)
PEAK_CASES = {
    # the best hit is a peak; its neighbours within m - 1 tiles are not; tile 5 is m away from tile 3: not overlapped
    "one cluster": ([0, 0, 0, 0], [2, 3, 4, 5], [1e-4, 1e-6, 1e-5, 1e-3], 2, [False, True, False, True]),
    # a hit overlapped only by a NON-peak is a peak: tile 4 (1e-5) loses to tile 3, tile 5 is overlapped by 4 alone (m = 2)
    "chain": ([0, 0, 0], [3, 4, 5], [1e-6, 1e-5, 1e-4], 2, [True, False, True]),
    # ties on the score go to the lower tile
    "tie": ([0, 0, 0], [7, 6, 8], [1e-5, 1e-5, 1e-5], 2, [False, True, True]),
    "tie at width three": ([0, 0, 0, 0], [6, 7, 8, 9], [1e-5, 1e-5, 1e-5, 1e-5], 3, [True, False, False, True]),
    # regions do not interact; width 1 makes every hit a peak
    "two regions": ([0, 1], [4, 4], [1e-3, 1e-9], 5, [True, True]),
    "width one": ([0, 0, 0], [1, 2, 3], [0.1, 0.2, 0.3], 1, [True, True, True]),
    "none": ([], [], [], 3, []),
}
