"""Plain numpy statements of dig_group_sums and of the parts of dig_group_fisher that are exact (include/dig_hip.h): n_used and the
m = 0, 1, 2 clauses -- what tests/test_gpu_group_fisher.py, test_gpu_group_fisher_guarded.py and test_gpu_element_meta.py compare
against bit for bit.  The m >= 3 clause is pinned by the 80-digit table of tests/golden/make_group_fisher_golden.py."""
import numpy as np


def _planes(x, member):
    x, member = np.asarray(x, np.float64), np.asarray(member) != 0
    x = x[None] if x.ndim == 2 else x
    assert x.ndim == 3 and member.ndim == 2 and member.shape[1] == x.shape[1]
    return x, member


def group_sums(x, member, gate=None):
    """out[r, g, e] = x[r, c, e] added up over the members c of g in ascending c from +0.0, one addition each; with a gate only the
    members whose gate[r, c, e] is not NaN.  f64 [R, M, E]."""
    x, member = _planes(x, member)
    gate = None if gate is None else _planes(gate, member)[0]
    R, C, E = x.shape
    out = np.zeros((R, len(member), E))
    with np.errstate(all="ignore"):
        for g, row in enumerate(member):
            for c in np.flatnonzero(row):
                out[:, g] = out[:, g] + (x[:, c] if gate is None else np.where(np.isnan(gate[:, c]), 0.0, x[:, c]))
    return out


def n_used(p, member):
    """i32 [R, M, E]: the members of g whose p[r, c, e] is not NaN."""
    p, member = _planes(p, member)
    return np.stack([(~np.isnan(p[:, row])).sum(axis=1) for row in member], axis=1).astype(np.int32) if len(member) else \
        np.zeros((p.shape[0], 0, p.shape[2]), np.int32)


def small_groups(p, member, pair):
    """The exact clauses: (value f64 [R, M, E], known bool [R, M, E]) -- NaN where m = 0, the member's p where m = 1, pair(p_a, p_b)
    with a < b where m = 2 (pair: the two-member form, nb_model.fisher_combine); known is False where m >= 3 (value NaN there)."""
    p, member = _planes(p, member)
    R, C, E = p.shape
    m = n_used(p, member)
    val = np.full((R, len(member), E), np.nan)
    for g, row in enumerate(member):
        ok = ~np.isnan(p) & row[None, :, None]                                   # [R, C, E]
        first = ok.argmax(axis=1)                                                # the lowest testable member
        last = C - 1 - ok[:, ::-1].argmax(axis=1)
        pa = np.take_along_axis(p, first[:, None], axis=1)[:, 0]
        pb = np.take_along_axis(p, last[:, None], axis=1)[:, 0]
        val[:, g] = np.where(m[:, g] == 1, pa, val[:, g])
        two = m[:, g] == 2
        if two.any():
            val[:, g][two] = np.asarray(pair(pa[two], pb[two]), np.float64)
    return val, m <= 2
