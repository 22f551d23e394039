"""Per-element / per-gene / per-tile pretraining: accumulate region parameters and Pi for every element.

Host mirror of DIGDriver/sequence_model/genic_driver_tools.py.  The reference walks the elements in a
pure-Python loop inside a multiprocessing pool (three h5 reads per element); here the whole element set
-- and any number of cohorts -- is one dig_accumulate_elements launch.

Element data container (f_nonc_data / f_genic), mirror layout (see digdriver_amd/io/mapfile.py):
    window_{w}/full_window_si_values   int  [N, 64]   64 context counts per genome bin
    window_{w}/full_window_si_index    int  [N, 3]    (chrom, start, end) of those bins
    window_{w}/{save_key}/names, chrom, strand, blk_ptr, blk_start, blk_end, L [E, n_class, 192]
(the reference's per-element HDF5 groups window_{w}/{save_key}/{elt}/{L_counts,region_counts}+overlaps,
sequence_tools.py:639-641, hold the same information one element at a time; region_counts and overlaps are
recomputed here from the bin table, which is how preprocess_nonc produced them, sequence_tools.py:628-634).
"""
import numpy as np
import pandas as pd

from .. import engine
from ..io import mapfile


# ---------------------------------------------------------------------------------------------
# small reference helpers
# ---------------------------------------------------------------------------------------------
def trip_to_str(trip):
    """genic_driver_tools.py:286-287"""
    return 'chr{}:{}-{}'.format(trip[0], trip[1], trip[2])


def _index_transform(s):
    """genic_driver_tools.py:721-725"""
    chrom = int(s.split(":")[0].lstrip("chr"))
    start = int(s.split(":")[-1].split('-')[0])
    end = int(s.split(":")[-1].split('-')[1])
    return "region_{}_{}_{}".format(chrom, start, end)


def get_ideal_overlaps(chrom, intervals, window):
    """genic_driver_tools.py:275-283: the bins touched by the blocks of one element, as (chrom, start, end)
    triples.  The reference returns them in set order; here they are sorted by start."""
    intervals = np.asarray(intervals)
    starts, ends = intervals[0].astype(np.int64), intervals[1].astype(np.int64)
    hi = int(max(ends.max(), starts.max()) // window + 2) if len(starts) else 1
    bin_start = np.arange(0, hi * window, window, dtype=np.int64)
    _, idx = engine.ideal_overlaps([0], [0, len(starts)], starts, ends, window, np.zeros(len(bin_start), np.int32), bin_start)
    return [(chrom, int(bin_start[i]), int(bin_start[i]) + int(window)) for i in idx]


def get_elt_ideal_overlaps(chrom, start, end, window):
    """genic_driver_tools.py:289-297"""
    return [(int(c), s, e) for c, s, e in get_ideal_overlaps(chrom, np.array([[start], [end]]), window)]


# ---------------------------------------------------------------------------------------------
# cohort tables
# ---------------------------------------------------------------------------------------------
def _columns_to_table(cols, dtype, block=2048):
    """C columns of N values -> a contiguous [N, C] table.  np.stack(axis=1) writes every column with a stride of C values (0.22 s
    for 288 000 x 37 doubles); rows are taken in blocks that stay in cache instead (0.06 s)."""
    a = cols if isinstance(cols, np.ndarray) and cols.ndim == 2 and cols.dtype == dtype else np.array(cols, dtype=dtype)   # [C, N]
    C, N = a.shape if a.ndim == 2 else (len(cols), 0)
    out = np.empty((N, C), dtype)
    for r0 in range(0, N, block):
        out[r0:r0 + block] = a[:, r0:r0 + block].T
    return out


class RegionTables:
    """region_params of one or more cohorts on a common, (chrom, start)-sorted bin grid.  `frames`: per cohort a DataFrame or a
    dict of column arrays (mapfile.read_columns) with CHROM, START, END, Y_PRED, STD, Y_TRUE, FLAG.
    The tables are kept COHORT-MAJOR ([C, N]: a cohort's column as it was read is one contiguous row -- `mu_cm`, `std_cm`,
    `y_cm`, `flag_cm`); the [N, C] layout of the kernels (`mu`, `std`, `y`, `flag`) is formed on first use on the host, or by
    `on_device(dev)`: the cohort-major tables uploaded and transposed on the device (a blocked host transpose of four 288 000 x
    37 tables was 0.15 s of a 37-cohort run, the device does it in under a millisecond)."""

    def __init__(self, frames):
        col = lambda f, k: np.asarray(f[k].values if hasattr(f[k], "values") else f[k])
        # one ordering for all cohorts: the (CHROM, START) order of the first map -- nothing to do when the map is stored in that
        # order (the usual case: 1 ms to check where a 288 000-row sort_values took 25 ms per cohort); a cohort whose raw
        # columns equal the first one's shares its ordering, any other is sorted on its own and must land on the same grid
        chrom0, start0 = col(frames[0], 'CHROM'), col(frames[0], 'START')
        in_order = len(chrom0) < 2 or bool(np.all((chrom0[1:] > chrom0[:-1]) | ((chrom0[1:] == chrom0[:-1]) & (start0[1:] >= start0[:-1]))))
        order0 = None if in_order else np.lexsort((start0, chrom0))
        take = (lambda a, o: a) if in_order else (lambda a, o: a[o])
        g_chrom, g_start = take(chrom0, order0), take(start0, order0)
        self.chrom = g_chrom.astype(np.int32)
        self.start = g_start.astype(np.int64)
        end0 = col(frames[0], 'END')
        self.window = int(take(end0, order0)[0] - g_start[0])                # genic_driver_tools.py:308
        cols = {k: [] for k in ('Y_PRED', 'STD', 'Y_TRUE', 'FLAG')}
        for f in frames:
            fc, fs = col(f, 'CHROM'), col(f, 'START')
            if fc is chrom0 or (np.array_equal(fc, chrom0) and np.array_equal(fs, start0)):
                order = order0
            else:
                order = np.lexsort((fs, fc))
                if not (np.array_equal(fc[order], g_chrom) and np.array_equal(fs[order], g_start)):
                    raise ValueError("all cohorts must share one bin grid")
            for k in cols:
                v = col(f, k)
                cols[k].append(v if order is None else v[order])
        C, N = len(frames), len(self.chrom)
        stack = lambda vs, dt: np.array(vs, dtype=dt).reshape(C, N)          # [C, N]: contiguous row copies
        self.mu_cm, self.std_cm = stack(cols['Y_PRED'], np.float64), stack(cols['STD'], np.float64)
        self.y_cm = stack(cols['Y_TRUE'], np.int32)
        self.flag_cm = stack([np.asarray(v).astype(bool) for v in cols['FLAG']], np.uint8)
        self._nc = {}

    def _table(self, name):
        if name not in self._nc:
            cm = getattr(self, name + "_cm")
            self._nc[name] = _columns_to_table(cm, cm.dtype)
        return self._nc[name]

    mu = property(lambda self: self._table("mu"))
    std = property(lambda self: self._table("std"))
    y = property(lambda self: self._table("y"))
    flag = property(lambda self: self._table("flag"))

    def on_device(self, device):
        """(mu, std, y, flag) as [N, C] device tensors: the cohort-major tables uploaded, transposed there."""
        import torch
        up = lambda a: torch.as_tensor(a, device=device).t().contiguous()
        return up(self.mu_cm), up(self.std_cm), up(self.y_cm), up(self.flag_cm)

    def aligned_context(self, si_index, si_values):
        """Rows of full_window_si_values re-ordered to this bin grid (a bin without context row is an error)."""
        si_index = np.asarray(si_index)
        key = (si_index[:, 0].astype(np.int64) << 40) | si_index[:, 1].astype(np.int64)
        want = (self.chrom.astype(np.int64) << 40) | self.start
        if len(key) == len(want) and np.array_equal(key, want):           # the usual case: the container lists the map's own bins
            return np.ascontiguousarray(si_values, np.int32)
        order = np.argsort(key, kind="stable")
        pos = np.searchsorted(key[order], want)
        pos = np.minimum(pos, max(len(key) - 1, 0))
        ok = key[order][pos] == want if len(key) else np.zeros(len(want), bool)
        if not ok.all():
            bad = int(np.flatnonzero(~ok)[0])
            raise KeyError("bin chr%s:%s of region_params has no context counts" % (int(self.chrom[bad]), int(self.start[bad])))
        return np.ascontiguousarray(np.asarray(si_values)[order[pos]], np.int32)


def sorted_d_pr(df_seq):
    """FREQ re-indexed by the sorted 'XYZ>XaZ' string (genic_driver_tools.py:321-325)."""
    names = [c + '>' + c[0] + m[2] + c[2] for m, c in zip(df_seq.MUT_TYPE, df_seq.CONTEXT)]
    order = np.argsort(np.array(names), kind="stable")
    return np.asarray(df_seq.FREQ.values, np.float64)[order]


def _read_cohort_frames(args):
    f, key = args
    # only what RegionTables takes, as column arrays straight from the stored blocks (no DataFrame: see mapfile.read_columns)
    return mapfile.read_columns(f, key, ['CHROM', 'START', 'END', 'Y_PRED', 'STD', 'Y_TRUE', 'FLAG']), mapfile.read_frame(f, 'sequence_model_192')


def _usable_cores():
    """The cores this process may run on: the length of its affinity mask where the platform has one (a process confined to a few
    cores of a large machine sizes its pools by those), else the machine's count."""
    import os
    return len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)


def _load_cohorts(f_pretrained, key='region_params', workers=1):
    """The maps' region_params as RegionTables + the [C, 192] sequence models.  workers > 1: the C maps are read side by
    side by spawned processes (37 whole-genome maps: 37 x 288 000 rows of HDF5)."""
    files = [f_pretrained] if isinstance(f_pretrained, (str, bytes)) or hasattr(f_pretrained, "__fspath__") else list(f_pretrained)
    workers = min(len(files), _usable_cores()) if workers is None else int(workers)
    if workers > 1 and len(files) > 1:
        from concurrent.futures import ThreadPoolExecutor          # (zlib and numpy release the interpreter lock)
        with ThreadPoolExecutor(max_workers=workers) as pool:
            got = list(pool.map(_read_cohort_frames, [(f, key) for f in files]))
    else:
        got = [_read_cohort_frames((f, key)) for f in files]
    tables = RegionTables([g[0] for g in got])
    d_pr = np.stack([sorted_d_pr(g[1]) for g in got])
    return files, tables, d_pr


def _minus_strand_order():
    """Order in which preprocess_nonc lists the 192 region counts of a '-' element (sequence_tools.py:633-634): positions
    sorted by the reverse complement of their substitution string."""
    from . import sequence_tools
    keys = sorted(sequence_tools.mk_trans_idx(n_up=1, n_down=1, collapse=False))
    rc = [sequence_tools.reverse_complement(k.split('>')[0]) + '>' + sequence_tools.reverse_complement(k.split('>')[1]) for k in keys]
    return np.array(sorted(range(192), key=lambda i: rc[i]), dtype=np.int64)


def _element_set_reference_layout(f_data, window, save_key, names=None):
    """The element container the REFERENCE writes (preprocess_nonc / preprocess_sites, sequence_tools.py:605-641,655-700):
    one HDF5 group per element, window_{w}/{key}/{elt}/{L_counts, region_counts} + attribute `overlaps` [(chrom, start,
    end)].  The overlapped bins come straight from the attribute; the strand is not stored, but region_counts is (the
    window contexts summed, listed in reverse-complement order for '-' elements), which is enough to recover it."""
    base = 'window_{}/{}'.format(window, save_key)
    all_names = mapfile.list_keys(f_data, base)
    use = list(names) if names is not None else all_names
    missing = [n for n in use if n not in set(all_names)]
    if missing:
        raise KeyError("elements %r are not in %s:%s" % (missing[:5], f_data, base))
    L = np.zeros((len(use), 1, 192), np.int32)
    rc = np.zeros((len(use), 192), np.int64)
    ov = []
    for j, n in enumerate(use):
        L[j, 0] = np.asarray(mapfile.read_array(f_data, '{}/{}/L_counts'.format(base, n))).astype(np.int32)
        rc[j] = np.asarray(mapfile.read_array(f_data, '{}/{}/region_counts'.format(base, n))).astype(np.int64)
        o = np.asarray(mapfile.read_attrs(f_data, '{}/{}'.format(base, n))['overlaps'])
        ov.append(np.array([[int(str(r[0]).replace('chr', '')), int(r[1])] for r in o.reshape(-1, 3)], dtype=np.int64).reshape(-1, 2))
    return dict(names=np.array(use, dtype=str), L=L, region_counts=rc, overlaps=ov)


def _element_set(f_data, window, save_key, names=None):
    base = 'window_{}/{}/'.format(window, save_key)
    if not mapfile.has_key(f_data, base + 'names') and mapfile._is_h5(f_data) and mapfile.has_key(f_data, base.rstrip('/')):
        return _element_set_reference_layout(f_data, window, save_key, names)
    all_names = mapfile.read_array(f_data, base + 'names').astype(str)
    blk_ptr = mapfile.read_array(f_data, base + 'blk_ptr').astype(np.int64)
    bs = mapfile.read_array(f_data, base + 'blk_start').astype(np.int64)
    be = mapfile.read_array(f_data, base + 'blk_end').astype(np.int64)
    strand = mapfile.read_array(f_data, base + 'strand')
    chrom = mapfile.read_array(f_data, base + 'chrom')
    L = mapfile.read_array(f_data, base + 'L')
    if names is not None:                                    # a subset, in the caller's order (no Python loop over the elements)
        pos = {n: i for i, n in enumerate(all_names)}
        sel = np.array([pos[n] for n in names], dtype=np.int64)
        cnt = (blk_ptr[1:] - blk_ptr[:-1])[sel]
        new_ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        take = np.repeat(blk_ptr[sel] - new_ptr[:-1], cnt) + np.arange(int(new_ptr[-1]), dtype=np.int64)
        all_names, strand, chrom, L, bs, be, blk_ptr = all_names[sel], strand[sel], chrom[sel], L[sel], bs[take], be[take], new_ptr
    if L.ndim == 2:
        L = L[:, None, :]
    strand = strand.astype(str)
    return dict(names=all_names, chrom=chrom.astype(np.int32), strand_minus=((strand == '-') | (strand == '-1')).astype(np.uint8),
                blk_ptr=blk_ptr, blk_start=bs, blk_end=be, L=np.ascontiguousarray(L, np.int32))


def _accumulate(tables, d_pr, f_data, elts, gene_length=None):
    w = tables.window
    si_index = mapfile.read_array(f_data, 'window_{}/full_window_si_index'.format(w))
    si_values = mapfile.read_array(f_data, 'window_{}/full_window_si_values'.format(w))
    ctx = tables.aligned_context(si_index, si_values)
    if 'overlaps' in elts:                                   # reference-layout container: bins from the stored attribute
        row = {(int(c), int(s)): i for i, (c, s) in enumerate(zip(tables.chrom, tables.start))}
        try:
            idx = [np.sort(np.array([row[(int(c), int(s))] for c, s in o], dtype=np.int32)) for o in elts['overlaps']]
        except KeyError as exc:
            raise KeyError("an element overlaps bin chr%s:%s, which region_params does not have" % exc.args[0]) from exc
        ov_ptr = np.concatenate([[0], np.cumsum([len(i) for i in idx])]).astype(np.int64)
        ov_idx = np.concatenate(idx).astype(np.int32) if idx else np.zeros(0, np.int32)
        plus = np.repeat(np.add.reduceat(ctx[ov_idx].astype(np.int64), ov_ptr[:-1], axis=0), 3, axis=1) if len(ov_idx) else \
            np.zeros((len(idx), 192), np.int64)
        plus[np.diff(ov_ptr) == 0] = 0
        minus = plus[:, _minus_strand_order()]
        is_plus = (plus == elts['region_counts']).all(axis=1)
        is_minus = (minus == elts['region_counts']).all(axis=1)
        if not (is_plus | is_minus).all():
            bad = elts['names'][~(is_plus | is_minus)][:5]
            raise ValueError("region_counts of elements %r do not match the window contexts of their overlapped bins "
                             "(was the element data built on another genome-counts file?)" % (list(bad),))
        elts = dict(elts, strand_minus=(~is_plus).astype(np.uint8))
    else:
        ov_ptr, ov_idx = engine.ideal_overlaps(elts['chrom'], elts['blk_ptr'], elts['blk_start'], elts['blk_end'], w,
                                               tables.chrom, tables.start)
    return engine.accumulate_elements(tables.mu, tables.std, tables.y, tables.flag, ctx, ov_ptr, ov_idx, elts['L'],
                                      elts['strand_minus'], d_pr, gene_length=gene_length)


def _nonc_frame(names, acc, c, acc_indel=None):
    ind = acc if acc_indel is None else acc_indel
    return pd.DataFrame({
        'ELT': names, 'ELT_SIZE': acc['ELT_SIZE'], 'FLAG': acc['FLAG'][:, c].astype(bool), 'R_SIZE': acc['R_SIZE'],
        'R_OBS': acc['R_OBS'][:, c], 'R_INDEL': ind['R_OBS'][:, c], 'MU': acc['MU'][:, c], 'SIGMA': acc['SIGMA'][:, c],
        'MU_INDEL': ind['MU'][:, c], 'SIGMA_INDEL': ind['SIGMA'][:, c], 'P_SUM': acc['P'][:, 0, c],
        'P_INDEL': acc['P_INDEL']})


# ---------------------------------------------------------------------------------------------
# nonc / tiled / genic models
# ---------------------------------------------------------------------------------------------
def nonc_model(elt_lst, f_pretrained, f_nonc_data, save_key, indels_direct):
    """genic_driver_tools.py:300-431.  `f_pretrained` may be one map or a list of maps (cohorts): one frame is
    returned for a single map, a list of frames (one per cohort, one launch for all of them) for a list."""
    files, tables, d_pr = _load_cohorts(f_pretrained)
    elts = _element_set(f_nonc_data, tables.window, save_key, names=list(elt_lst))
    acc = _accumulate(tables, d_pr, f_nonc_data, elts)
    acc_ind = None
    if indels_direct:
        _, t_ind, _ = _load_cohorts(f_pretrained, key='region_params_indels')
        acc_ind = _accumulate(t_ind, d_pr, f_nonc_data, elts)
    frames = [_nonc_frame(elts['names'], acc, c, acc_ind) for c in range(len(files))]
    return frames[0] if isinstance(f_pretrained, (str, bytes)) or hasattr(f_pretrained, "__fspath__") else frames


def nonc_model_parallel(f_pretrained, f_nonc_data, nonc_L_key, N_procs, indels_direct=False):
    """genic_driver_tools.py:434-463.  N_procs is accepted for interface compatibility; the GPU needs no pool."""
    first = f_pretrained if isinstance(f_pretrained, (str, bytes)) else list(f_pretrained)[0]
    idx = mapfile.read_array(first, 'idx')
    window = int(idx[0, 2] - idx[0, 1])
    base = 'window_{}/{}'.format(window, nonc_L_key)
    if mapfile.has_key(f_nonc_data, base + '/names'):
        names = mapfile.read_array(f_nonc_data, base + '/names').astype(str)
    else:                                                   # the reference's per-element groups (genic_driver_tools.py:443)
        names = mapfile.list_keys(f_nonc_data, base)
    return nonc_model(list(names), f_pretrained, f_nonc_data, nonc_L_key, indels_direct)


def tiled_nonc_model(elt_lst, f_pretrained, f_nonc_data, save_key):
    """genic_driver_tools.py:599-690: one-bin-per-element tiles named 'chr{c}:{s}-{e}'; L comes from the table
    '{save_key}/L_counts' (rows = tiles).  Returned ELT names are 'region_{c}_{s}_{e}' (:666)."""
    files, tables, d_pr = _load_cohorts(f_pretrained)
    w = tables.window
    L_table = mapfile.read_frame(f_nonc_data, "{}/L_counts".format(save_key))
    elt_lst = list(elt_lst)
    L = np.ascontiguousarray(L_table.loc[elt_lst].values, np.int32)[:, None, :]
    chrom = np.array([int(e.split(":")[0].lstrip("chr")) for e in elt_lst], np.int32)
    start = np.array([int(e.split(":")[1].split("-")[0]) for e in elt_lst], np.int64)
    region_start = (start // 10000) * 10000                   # hard-coded 10 kb in the reference (:634)
    n = len(elt_lst)
    elts = dict(names=np.array(elt_lst), chrom=chrom, strand_minus=np.zeros(n, np.uint8), blk_ptr=np.arange(n + 1),
                blk_start=region_start, blk_end=region_start + w, L=L)
    acc = _accumulate(tables, d_pr, f_nonc_data, elts)
    out_names = [_index_transform(e) for e in elt_lst]
    frames = [_nonc_frame(out_names, acc, c) for c in range(len(files))]
    return frames[0] if isinstance(f_pretrained, (str, bytes)) else frames


def tiled_model_parallel(f_pretrained, f_nonc_data, save_key, N_procs):
    """genic_driver_tools.py:692-719"""
    elt_table = mapfile.read_frame(f_nonc_data, "{}/L_counts".format(save_key))
    return tiled_nonc_model(list(elt_table.index), f_pretrained, f_nonc_data, save_key)


def genic_model(genes_lst, f_pretrained_str, f_genic_str, counts_key, indels_direct):
    """genic_driver_tools.py:31-203: four mutation classes per gene (L_data rows: silent, missense, nonsense,
    splice).  Genes on X/Y are skipped (:90-92).  The gene container holds, under window_{w}/genes/, the same
    arrays as an element set with L of shape [G, 4, 192]; GENE_LENGTH = sum(end - start + 1) over CDS blocks (:158).
    `counts_key` is accepted for interface compatibility: the per-gene region counts it names in the reference
    are the sum of the overlapped bins' context rows, which is what the kernel recomputes."""
    files, tables, d_pr = _load_cohorts(f_pretrained_str)
    w = tables.window
    base = 'window_{}/genes/'.format(w)
    chrom_str = mapfile.read_array(f_genic_str, base + 'chrom_str').astype(str)
    all_names = mapfile.read_array(f_genic_str, base + 'names').astype(str)
    pos = {n: i for i, n in enumerate(all_names)}
    keep = [g for g in genes_lst if chrom_str[pos[g]] not in ('X', 'Y')]
    elts = _element_set(f_genic_str, w, 'genes', names=keep)
    nblk = np.diff(elts['blk_ptr'])
    owner = np.repeat(np.arange(len(keep)), nblk)
    glen = np.zeros(len(keep), np.int64)
    np.add.at(glen, owner, elts['blk_end'] - elts['blk_start'] + 1)
    acc = _accumulate(tables, d_pr, f_genic_str, elts, gene_length=glen.astype(np.int32))
    acc_ind = None
    if indels_direct:
        _, t_ind, _ = _load_cohorts(f_pretrained_str, key='region_params_indels')
        acc_ind = _accumulate(t_ind, d_pr, f_genic_str, elts, gene_length=glen.astype(np.int32))
    frames = []
    for c in range(len(files)):
        ind = acc if acc_ind is None else acc_ind
        P = acc['P'][:, :, c]
        frames.append(pd.DataFrame({
            'CHROM': [chrom_str[pos[g]] for g in keep], 'GENE': keep, 'GENE_LENGTH': glen, 'R_SIZE': acc['R_SIZE'],
            'R_OBS': acc['R_OBS'][:, c], 'R_INDEL': ind['R_OBS'][:, c], 'MU': acc['MU'][:, c], 'SIGMA': acc['SIGMA'][:, c],
            'MU_INDEL': ind['MU'][:, c], 'SIGMA_INDEL': ind['SIGMA'][:, c], 'FLAG': acc['FLAG'][:, c].astype(bool),
            'P_MIS': P[:, 1], 'P_NONS': P[:, 2], 'P_SILENT': P[:, 0], 'P_SPLICE': P[:, 3], 'P_TRUNC': P[:, 2] + P[:, 3],
            'P_INDEL': acc['P_INDEL']}))
    return frames[0] if isinstance(f_pretrained_str, (str, bytes)) else frames


def genic_model_parallel(f_pretrained_str, f_genic_str, N_procs, counts_key="window_10kb/counts", indels_direct=False):
    """genic_driver_tools.py:206-227"""
    first = f_pretrained_str if isinstance(f_pretrained_str, (str, bytes)) else list(f_pretrained_str)[0]
    idx = mapfile.read_array(first, 'idx')
    window = int(idx[0, 2] - idx[0, 1])
    names = mapfile.read_array(f_genic_str, 'window_{}/genes/names'.format(window)).astype(str)
    return genic_model(list(names), f_pretrained_str, f_genic_str, counts_key, indels_direct)


def get_region_params_direct(df, overlaps, window):
    """genic_driver_tools.py:258-272 for one element on a region_params frame (host convenience; the batched
    path is dig_accumulate_elements)."""
    rows = [trip_to_str(r) for r in overlaps]
    sub = df.loc[rows]
    mu, var, robs, flag = 0, 0, 0, False
    for yp, sd, yt, fl in zip(sub.Y_PRED.values, sub.STD.values, sub.Y_TRUE.values, sub.FLAG.values):
        mu += yp
        var += sd ** 2
        robs += yt
        flag = bool(flag) | bool(fl)
    return mu, np.sqrt(var), robs, flag


def get_region_params(df, chrom, intervals, window):
    """genic_driver_tools.py:235-251"""
    return get_region_params_direct(df, get_ideal_overlaps(chrom, intervals, window), window)
