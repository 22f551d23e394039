"""Writes tests/golden/pair_fisher_golden.npz: 2 x 2 tables (n, r, k, a) with the two exact one-sided Fisher tails, computed on Python
integers (tests/pair_fisher_statement.exact_tails) and rounded once to double.

  every table with n <= 12                         1 819
  60 each with n in {64, 100, 2 800, 16 384, 65 536}  300: r over the whole range (0 and n among them), k <= 600 so that the supports
                                                   stay narrow and this runs in seconds; a = lo, hi, the mode, one either side of it,
                                                   and places in between.  Tails down to 0 (below 1e-250 the kernel only has to be small).

Run from the repository root: python tests/golden/make_pair_fisher_golden.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pair_fisher_statement import exact_tails  # noqa: E402

LARGE_N = (64, 100, 2800, 16384, 65536)
PER_N = 60


def small_tables():
    return [(n, r, k, a) for n in range(1, 13) for r in range(n + 1) for k in range(n + 1)
            for a in range(max(0, r + k - n), min(r, k) + 1)]


def large_tables(rng):
    out = []
    for n in LARGE_N:
        rs = [0, n, 1, n - 1, n // 2, n // 3, 7, min(n, 600), n - 7, n - n // 5]
        ks = [0, n if n <= 600 else 600, 1, 2, 13, min(n, 100), min(n, 311), min(n, 599), min(n - 1, 57), min(n, 600)]
        tables = []
        for i in range(PER_N):
            r = rs[i % len(rs)] if i < 2 * len(rs) else int(rng.integers(1, n))
            k = ks[(i // 2) % len(ks)] if i < 2 * len(ks) else int(rng.integers(1, min(n, 600) + 1))
            lo, hi = max(0, r + k - n), min(r, k)
            mode = min(max((r + 1) * (k + 1) // (n + 2), lo), hi)
            places = [lo, hi, mode, max(lo, mode - 1), min(hi, mode + 1), (lo + mode) // 2, (mode + hi + 1) // 2,
                      int(rng.integers(lo, hi + 1))]
            tables.append((n, r, k, places[i % len(places)]))
        if n >= 2800:                                    # the far ends of wide supports: tails below 1e-250, down to 0
            far = [(n // 3, 600, 1), (n - n // 5, 600, 0), (n // 2, 599, 1), (n // 2, 311, 0), (n // 7, 450, 1), (n - n // 7, 450, 0),
                   (n // 2, 600, 1), (n // 2, 600, 0), (n // 4, 500, 1), (n - n // 4, 520, 0)]
            for i, (r, k, top) in enumerate(far):
                lo, hi = max(0, r + k - n), min(r, k)
                tables[PER_N - 1 - i] = (n, r, k, (hi - i // 2 * 15) if top else (lo + i // 2 * 15))
        out += tables
    return out


def main():
    rng = np.random.default_rng(20261021)
    tables = small_tables()
    assert len(tables) == 1819
    tables += large_tables(rng)
    t = np.array(tables, np.int64)
    exact = np.array([exact_tails(*map(int, row)) for row in t], np.float64)
    tiny = (exact < 1e-250).any(1)
    assert tiny.sum() >= 8 and (exact == 0).any() and ((exact > 0) & (exact < 1e-250)).any() and ((exact >= 1e-250) & (exact < 1e-100)).any()
    assert (exact.max(1) >= 0.5 - 1e-12).all() and (exact <= 1.0).all()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pair_fisher_golden.npz")
    np.savez_compressed(path, n=t[:, 0].astype(np.int32), r=t[:, 1].astype(np.int32), k=t[:, 2].astype(np.int32), a=t[:, 3].astype(np.int32),
                        pval_cooccur=exact[:, 0], pval_exclusive=exact[:, 1])
    print("%d tables, %d with a tail below 1e-250, smallest positive tail %.3g -> %s (%d bytes)"
          % (len(t), int(tiny.sum()), exact[exact > 0].min(), path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
