"""The statement of the pairs rule (include/dig_hip.h, "pairs of the element route") in numpy and plain double: bit rows from keys, the
intersection counts by np.bitwise_and and a popcount, the two tails by the rule's own evaluation with math.lgamma.  And exact_tails:
the same two sums on Python integers, correctly rounded to double -- what the golden file holds."""
import math

import numpy as np

TINY = 1e-250                     # below this exact value a result only has to be small (the tolerance contract of the README)


def pair_words(n_max):
    return max(2, 2 * ((int(n_max) + 127) // 128))


def pair_index(i, j, H):
    return i * (2 * H - i - 1) // 2 + (j - i - 1)


def bits_from_keys(row, sample, H_total, W):
    """u64 [H_total, W]: bit sample % 64 of word sample / 64 of row `row`, for every key with a row inside the matrix."""
    bits = np.zeros((H_total, W), np.uint64)
    for r, s in zip(np.asarray(row).tolist(), np.asarray(sample).tolist()):
        if 0 <= r < H_total and 0 <= s < 64 * W:
            bits[r, s >> 6] |= np.uint64(1) << np.uint64(s & 63)
    return bits


def bits_from_bool(m, W):
    """u64 [H, W] of a bool [H, n] matrix."""
    m = np.asarray(m, bool)
    padded = np.zeros((m.shape[0], 64 * W), np.uint8)
    padded[:, :m.shape[1]] = m
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(m.shape[0], W)


def popcount(x):
    """Bits set per row of a u64 [..., W] array."""
    x = np.ascontiguousarray(x, np.uint64)
    return np.unpackbits(x.view(np.uint8).reshape(x.shape[:-1] + (-1,)), axis=-1).sum(-1).astype(np.int32)


def tails(n, r, k, a):
    """(PVAL_COOCCUR, PVAL_EXCLUSIVE) of the table by the rule's evaluation, in double."""
    if r == 0 or k == 0 or r == n or k == n:
        return 1.0, 1.0
    lo, hi = max(0, r + k - n), min(r, k)
    assert lo <= a <= hi
    lf = lambda x: math.lgamma(x + 1.0)
    mode = (r + 1) * (k + 1) // (n + 2)
    d = n - k - r + a
    logp = ((lf(k) - lf(a) - lf(k - a)) + (lf(n - k) - lf(r - a) - lf(d))) - (lf(n) - lf(r) - lf(n - r))
    pa = math.exp(logp) if logp > -745.2 else 0.0
    t = s = pa
    up = a >= mode
    x = a
    if up:
        while x < hi:
            t *= ((k - x) * (r - x)) / ((x + 1) * (n - k - r + x + 1))
            s += t
            x += 1
            if not t > s * 2.0 ** -56:
                break
    else:
        while x > lo:
            t *= (x * (n - k - r + x)) / ((k - x + 1) * (r - x + 1))
            s += t
            x -= 1
            if not t > s * 2.0 ** -56:
                break
    small, large = min(1.0, s), min(1.0, (1.0 - s) + pa)
    return (small, large) if up else (large, small)


def exact_tails(n, r, k, a):
    """(sum_{x >= a} pmf(x), sum_{x <= a} pmf(x)) of the hypergeometric density on Python integers, each correctly rounded to
    double: one math.comb for the first term, exact integer recurrences for the others; the total must be C(n, r)."""
    lo, hi = max(0, r + k - n), min(r, k)
    assert 0 <= r <= n and 0 <= k <= n and lo <= a <= hi
    term = math.comb(n - k, r) if lo == 0 else math.comb(k, lo)              # C(k, lo) C(n - k, r - lo); r - lo = n - k where lo > 0
    total = upper = lower = 0
    for x in range(lo, hi + 1):
        total += term
        if x >= a:
            upper += term
        if x <= a:
            lower += term
        if x < hi:
            q, rem = divmod(term * (k - x) * (r - x), (x + 1) * (n - k - r + x + 1))
            assert rem == 0
            term = q
    assert total == math.comb(n, r)
    return upper / total, lower / total


def pair_counts(bits, rows, n_samples):
    """n_row i32 [H_total] and, per pair in pair order, cohort after cohort: n_both i32 and the table's (n, r, k) as i64 [n_pairs, 3]."""
    bits = np.ascontiguousarray(bits).view(np.uint64)
    n_row = popcount(bits) if bits.shape[0] else np.zeros(0, np.int32)
    both, nrk = [np.zeros(0, np.int32)], [np.zeros((0, 3), np.int64)]
    r0 = 0
    for H, n in zip(rows, n_samples):
        for i in range(H - 1):
            both.append(popcount(bits[r0 + i][None, :] & bits[r0 + i + 1:r0 + H]))
            k = n_row[r0 + i + 1:r0 + H].astype(np.int64)
            nrk.append(np.stack([np.full_like(k, n), np.full_like(k, n_row[r0 + i]), k], 1))
        r0 += H
    return n_row, np.concatenate(both), np.concatenate(nrk)


def pair_fisher(bits, rows, n_samples):
    """The four outputs of dig_pair_fisher over the stacked matrix: n_row i32 [H_total]; n_both i32, pval_cooccur, pval_exclusive f64
    [n_pairs] in pair order, cohort after cohort."""
    n_row, both, nrk = pair_counts(bits, rows, n_samples)
    p = np.array([tails(int(n), int(r), int(k), int(a)) for (n, r, k), a in zip(nrk, both)], np.float64).reshape(-1, 2)
    return n_row, both, p[:, 0].copy(), p[:, 1].copy()


def rows_of_table(n, r, k, a):
    """The table as two bool rows over n samples: row A the first r samples, row B a of them and k - a outside."""
    m = np.zeros((2, n), bool)
    m[0, :r] = True
    m[1, :a] = True
    m[1, r:r + k - a] = True
    return m


def check_pvalues(got, exact, what):
    """The accuracy bound: within 1e-6 relative where the exact value is at least 1e-250, under 1.1e-250 below that.  Prints the worst
    relative error before it asserts; returns it."""
    got, exact = np.asarray(got, np.float64), np.asarray(exact, np.float64)
    assert got.shape == exact.shape and not np.isnan(got).any(), what
    big = exact >= TINY
    rel = np.abs(got[big] - exact[big]) / exact[big]
    worst = float(rel.max()) if rel.size else 0.0
    print("%s: worst relative error %.3g over %d values, %d below 1e-250" % (what, worst, int(big.sum()), int((~big).sum())))
    assert worst <= 1e-6, (what, worst, exact[big][rel.argmax()])
    assert (got[~big] < 1.1e-250).all() and (got[~big] >= 0).all(), what
    return worst
