"""The rows of many cohorts as one stack: what every many-cohort route does before it calls the engine.

A cohort record is the dict an encoder returns (tabulate_gpu.encode_mutation_file / encode_gene_rows, sites.encode_site_rows,
objectives.encode_objective_rows, sequence_tools.encode_sequence_rows): row columns of one length, numpy arrays or -- uploaded by
the parser threads already -- device tensors, and, where samples matter, a `sample_names` list.  Written on the backend pair of
_marshal.py, so it serves both; torch is imported only when arrays are placed on a device.
"""
import numpy as np

from .. import _lib
from .._marshal import backend_of, resolve_device


def sample_offsets(records):
    """A cohort's first GLOBAL sample: int64 [C + 1], 0 first (the sample_offsets of the engine's counting routes)."""
    return np.concatenate([[0], np.cumsum([len(r["sample_names"]) for r in records])]).astype(np.int64)


def id_offsets(records, key):
    """A cohort's first id once the dense ids of column `key` (uid, gene) are made distinct over the cohorts: int64 [C + 1]; a
    cohort holds max + 1 ids, one without rows none."""
    return np.concatenate([[0], np.cumsum([int(r[key].max()) + 1 if len(r[key]) else 0 for r in records])]).astype(np.int64)


def column(records, key, dtype=None, shift=None, subset=None):
    """Column `key` of the cohorts (of those in `subset`, in its order) one after the other, as `dtype` ("i64", "i32", "u8", ...;
    None: the column's own).  shift: an integer per cohort added to its rows first (sample_offsets: the global sample; id_offsets:
    distinct ids).  Arrays in -> an array, device tensors in -> a tensor; an empty array of `dtype` when nothing is left."""
    which = range(len(records)) if subset is None else list(subset)
    cols = [records[c][key] for c in which]
    be = backend_of(*cols)
    if shift is not None:
        cols = [be.arr(x, dtype) + int(shift[c]) for c, x in zip(which, cols)]
    return be.cat(cols, dtype)


def cohort_column(records, key, subset=None):
    """The cohort of every row of column(records, key, subset=subset): int32, from the cohorts' row counts."""
    which = range(len(records)) if subset is None else list(subset)
    return np.repeat(np.asarray(which, np.int32), [len(records[c][key]) for c in which])


def place(arrays, on_device=None, device=0):
    """Host arrays where a route wants them: C-contiguous as they are (on_device False) or as tensors on `device` (True); None:
    the device unless the process is torch-free."""
    arrays = [np.ascontiguousarray(a) for a in arrays]
    if not ((not _lib.TORCH_FREE) if on_device is None else on_device):
        return arrays
    import torch
    dev = resolve_device(device)
    return [torch.as_tensor(a, device=dev) for a in arrays]
