"""The problems of test_gpu_tile_windows.py and test_gpu_tile_windows_guarded.py.  Host data made from seeds; nothing is computed by
the library.

The small problem is that of tile_samples_cases.py (six regions: whole, one tile short, all N, cut at a contig's end, without a
position, two adjacent; C = 3; bin sizes 50 and 1).  Its widths, per bin size with T tiles per region:
  1, 2, 3 (does not divide T = 8 or 400), T, T + 1, and one more than the tiles of the region that is cut at the contig's end (3
  tiles of 50 positions, 149 of 1): that region then has ONE window over all its tiles while its neighbours have many.

The long problem has rows longer than what a workgroup of tile_window_kernel stages: bin size 1 on two regions of 10 000 and 9 950
positions (T = 10 000), C = 2.  CHUNK names the kernel's outputs per workgroup (kWinChunk, csrc/dig_tilewindows.hip): the chunk
borders of a row lie at the tiles 1 024 j.  Cohort 0 has a row on either side of every border (tiles 1 024 j - 1 and 1 024 j), so at
any width >= 2 a window with k_w > 0 straddles each of them; cohort 1 has rows one halo behind every border (tile 1 024 j + 1 022,
the last term of the width-1 024 window that starts at tile 1 024 j - 1), and both have background rows."""
import itertools

import numpy as np

import tile_samples_cases as K

CHUNK = 1024                       # kWinChunk
MAX_WIDTH = 2048                   # DIG_TILE_WINDOW_MAX_WIDTH
SHORT_TILES = {50: 3, 1: 149}      # n_valid of region 3 of tile_samples_cases


def widths(binsize):
    T = -(-400 // binsize)
    return [1, 2, 3, T, T + 1, SHORT_TILES[binsize] + 1]


# ---- the long rows ------------------------------------------------------------------------------------------------------------------
LONG_T = 10000
LONG_IDX = np.array([[1, 50, 10050], [2, 40, 9990]], np.int64)
LONG_LENGTHS = {"1": 10100, "2": 10100}
LONG_WIDTHS = (7, 1024)
LONG_C = 2


def long_genome_sequences():
    rng = np.random.default_rng(23)
    return {name: "".join(rng.choice(list("ACGT"), n)) for name, n in LONG_LENGTHS.items()}


def long_s_prob(c):
    rng = np.random.default_rng(300 + c)
    return {"".join(k): float(v) for k, v in zip(itertools.product("ACGT", repeat=3), rng.uniform(0.5, 1.5, 64) * 1e-3)}


def long_mu_sigma():
    mu = np.array([[40.0, 35.0], [60.0, 45.0]])
    return mu, 0.3 * mu


def long_rows():
    """Per cohort (chrom labels, start, end) arrays."""
    rng = np.random.default_rng(29)
    out = []
    for c in range(LONG_C):
        chrom, start = [], []
        for ch, first, _ in LONG_IDX:
            borders = np.arange(CHUNK, LONG_T, CHUNK)
            at = np.concatenate([borders - 1, borders]) if c == 0 else borders + CHUNK - 2
            at = np.concatenate([at[at < LONG_T - 60], rng.integers(0, LONG_T - 60, 40)])
            chrom += [str(ch)] * len(at)
            start += list(first + at)
        start = np.array(start, np.int64)
        out.append((np.array(chrom), start, start + 1))
    return out
