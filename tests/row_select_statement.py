"""Plain numpy statements of dig_row_select_count / dig_row_select_fill / dig_row_scatter (include/dig_hip.h) and of
cohort_batch.plane_qvalues -- what tests/test_gpu_row_select.py, test_gpu_row_select_guarded.py and test_gpu_element_calls.py compare
the kernels with, bit for bit.  K is the chunk of the library (dig_row_select_chunk), passed in by the caller."""
import numpy as np


def selected(score, cut):
    """bool [rows, n]: score[r, e] <= cut[r]; a NaN on either side compares false."""
    score = np.asarray(score, np.float64)
    cut = np.broadcast_to(np.asarray(cut, np.float64).reshape(-1), (score.shape[0],))
    with np.errstate(invalid="ignore"):
        return score <= cut[:, None]


def counts(score, cut, K):
    """i32 [rows * ceil(n / K)]: the selected elements of every chunk of K consecutive elements of every row."""
    sel = selected(score, cut)
    rows, n = sel.shape
    chunks = -(-n // K)
    padded = np.zeros((rows, chunks * K), bool)
    padded[:, :n] = sel
    return padded.reshape(rows, chunks, K).sum(axis=2).astype(np.int32).reshape(-1)


def fill(score, cut):
    """(index i32, score f64 [selected], row_ptr i64 [rows + 1]): the selected elements row-major, ascending in e within a row."""
    score = np.asarray(score, np.float64)
    sel = selected(score, cut)
    r, e = np.nonzero(sel)                                           # row-major
    return e.astype(np.int32), score[r, e], np.concatenate([[0], np.cumsum(sel.sum(axis=1))]).astype(np.int64)


def scatter(score, cut, values, fill_value):
    """f64 [rows, n]: values, in the order of fill's lists, at the selected places and fill_value elsewhere."""
    sel = selected(score, cut)
    out = np.full(sel.shape, fill_value, np.float64)
    out[sel] = np.asarray(values, np.float64)
    return out


def plane_qvalues(p):
    """For every row along the last axis: nb_model.get_q_vals (its host form: statsmodels' operations, pinned by the golden files)
    of the row's non-NaN values, put back at their places; NaN where p is NaN."""
    from digdriver_amd.sequence_model import nb_model
    p = np.asarray(p, np.float64)
    flat = p.reshape(-1, p.shape[-1])
    out = np.full(flat.shape, np.nan)
    for r in range(flat.shape[0]):
        ok = ~np.isnan(flat[r])
        out[r, ok] = nb_model.get_q_vals(flat[r][ok])
    return out.reshape(p.shape)
