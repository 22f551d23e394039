"""How good a mutation-rate map is: variance explained across scales and the calibration of its region p-values, for many maps at once.

The numeric helpers of the reference's sequence_model/gp_tools.py -- merge_windows (:125-160: Y_TRUE, Y_PRED and sqrt(sum STD^2) of
the bins whose START falls inside each larger window, three boolean masks over the whole frame per merged window) and
calibration_score_by_pvals (:117-121) -- as one segmented merge with the region test per merged window (dig_map_windows) and one
bit-reproducible score reduction (dig_map_scores) per scale, over all cohorts at once.  include/dig_hip.h states the definitions.
"""
import os

import numpy as np
import pandas as pd

from .. import engine
from ..io import mapfile

DEFAULT_SCALES_BP = (10_000, 50_000, 100_000, 1_000_000)
LEVELS = engine.MAP_LEVELS
REPORT_COLUMNS = ["SCALE_BP", "N_WINDOWS", "N_TESTED", "OBS_TOTAL", "EXP_TOTAL", "R2", "CALIB_SCORE"] + ["FRAC_%g" % a for a in LEVELS]
WINDOW_COLUMNS = ["START", "END", "N_BINS", "Y_TRUE", "Y_PRED", "STD", "PVAL"]
_MAP_COLUMNS = ['CHROM', 'START', 'END', 'Y_PRED', 'STD', 'Y_TRUE', 'FLAG']


def check_options(n_maps, labels=None, tail="upper", outliers_fdr=None, scales_bp=DEFAULT_SCALES_BP):
    """What can be refused before a map is read; ValueError."""
    if n_maps < 1:
        raise ValueError("at least one map")
    if labels is not None and len(labels) != n_maps:
        raise ValueError("labels: one label per map (%d labels, %d maps)" % (len(labels), n_maps))
    if labels is not None and len(set(labels)) != len(labels):
        raise ValueError("labels: every label once")
    if tail not in engine.MAP_TAILS:
        raise ValueError("tail: 'upper' or 'side', not %r" % (tail,))
    if outliers_fdr is not None and not 0.0 < float(outliers_fdr) <= 1.0:
        raise ValueError("outliers_fdr: a level within (0, 1], not %r" % (outliers_fdr,))
    scales = [int(b) for b in scales_bp]
    if not scales or any(b != v or b < 1 for b, v in zip(scales, scales_bp)) or len(set(scales)) != len(scales):
        raise ValueError("scales_bp: one or more different whole numbers of base pairs >= 1, not %r" % (list(scales_bp),))
    return scales


def scales_in_bins(scales_bp, window):
    """Base pairs -> whole numbers of the grid's window; ValueError for a scale that is no multiple of it."""
    bad = [b for b in scales_bp if b % window]
    if bad:
        raise ValueError("scales %r are not multiples of the maps' window of %d bp" % (bad, window))
    return [b // window for b in scales_bp]


def merged_runs(chrom, start, step):
    """The merged windows of a (CHROM, START)-sorted grid at `step` base pairs: the runs of equal (chrom, start // step) in grid order.
    Returns (run_ptr int64 [M + 1], CHROM int32 [M], START int64 [M], END int64 [M]); START = g step, END = (g + 1) step."""
    chrom, g = np.asarray(chrom), np.asarray(start, np.int64) // int(step)
    head = np.ones(len(chrom), bool)
    head[1:] = (chrom[1:] != chrom[:-1]) | (g[1:] != g[:-1])
    first = np.flatnonzero(head)
    return (np.concatenate([first, [len(chrom)]]).astype(np.int64), chrom[first].astype(np.int32), g[first] * int(step),
            (g[first] + 1) * int(step))


def load_maps(f_maps, key='region_params', workers=None):
    """The maps' region_params as genic_driver_tools.RegionTables (no sequence model is needed), and each map's cohort_name
    attribute (None without one).  ValueError for maps on different grids."""
    from ..sequence_model import genic_driver_tools as gdt
    files = [f_maps] if isinstance(f_maps, (str, bytes)) or hasattr(f_maps, "__fspath__") else list(f_maps)

    def read(f):
        name = mapfile.read_attrs(f).get('cohort_name')
        return mapfile.read_columns(f, key, _MAP_COLUMNS), None if name is None else str(name.decode() if isinstance(name, bytes) else name)
    workers = min(len(files), gdt._usable_cores()) if workers is None else int(workers)
    if workers > 1 and len(files) > 1:
        from concurrent.futures import ThreadPoolExecutor          # (zlib and numpy release the interpreter lock)
        with ThreadPoolExecutor(max_workers=workers) as pool:
            got = list(pool.map(read, files))
    else:
        got = [read(f) for f in files]
    return files, gdt.RegionTables([g[0] for g in got]), [g[1] for g in got]


def default_labels(files, names):
    """A map's cohort_name attribute, else its file stem."""
    stem = lambda f: os.path.splitext(os.path.basename(os.path.normpath(str(f))))[0]
    return [n if n else stem(f) for f, n in zip(files, names)]


def report_rows(counts, sums, scale_bp):
    """The report's columns for one scale from dig_map_scores' host arrays counts [C, 7], sums [C, 4]: R2 = Sxy^2 / (Sxx Syy) -- 0 where
    that is NaN (gp_trainer.py:23-25) or with fewer than two windows --, FRAC_a = N_BELOW[a] / N_TESTED and CALIB_SCORE = sum over
    the four levels of (a - FRAC_a)^2 (gp_tools.py:117-121)."""
    counts, sums = np.asarray(counts, np.int64), np.asarray(sums, np.float64)
    with np.errstate(all="ignore"):
        r2 = sums[:, 3] * sums[:, 3] / (sums[:, 1] * sums[:, 2])
        r2 = np.where(np.isnan(r2) | (counts[:, 0] < 2), 0.0, r2)
        frac = counts[:, 3:7] / counts[:, 1:2].astype(np.float64)
        calib = np.zeros(len(counts))
        for j, a in enumerate(LEVELS):                               # (the reference's sum: first level to last)
            calib = calib + (a - frac[:, j]) ** 2
    d = dict(SCALE_BP=np.full(len(counts), int(scale_bp), np.int64), N_WINDOWS=counts[:, 0], N_TESTED=counts[:, 1], OBS_TOTAL=counts[:, 2],
             EXP_TOTAL=sums[:, 0], R2=r2, CALIB_SCORE=calib)
    d.update({"FRAC_%g" % a: frac[:, j] for j, a in enumerate(LEVELS)})
    return d


def _select_outliers(planes, fdr):
    """Per cohort the windows with Benjamini-Hochberg q <= fdr over the cohort's testable windows: (hit_ptr host [C + 1], the hits'
    window index, and the planes' values and QVAL at the hits, as host arrays, grid order within a cohort)."""
    import torch
    from ..driver_model import cohort_batch
    from ..sequence_model import nb_model
    pval = planes["pval"]
    C = int(pval.shape[0])
    Q = cohort_batch.plane_qvalues(pval)
    cuts = np.array([nb_model.bh_cut(pval[c], Q[c], fdr) for c in range(C)])          # {q <= fdr} = {p <= p*}; NaN never passes
    hits = engine.row_select(pval, cuts)
    ptr, idx = hits["row_ptr"], hits["index"].long()
    row = torch.as_tensor(np.repeat(np.arange(C), np.diff(ptr)), device=idx.device)
    got = {k: v[row, idx].cpu().numpy() for k, v in planes.items()}
    got["qval"] = Q[row, idx].cpu().numpy()
    return ptr, idx.cpu().numpy(), got


def window_frame(chrom, start, end, cols, qval=None):
    """One cohort's merged windows as the frame the command writes: index CHROM, columns START END N_BINS Y_TRUE Y_PRED STD PVAL (+ QVAL)."""
    d = dict(START=np.asarray(start, np.int64), END=np.asarray(end, np.int64), N_BINS=np.asarray(cols["n_bins"], np.int64),
             Y_TRUE=np.asarray(cols["y_true"], np.int64), Y_PRED=np.asarray(cols["y_pred"], np.float64),
             STD=np.asarray(cols["std"], np.float64), PVAL=np.asarray(cols["pval"], np.float64))
    if qval is not None:
        d["QVAL"] = np.asarray(qval, np.float64)
    return pd.DataFrame(d, index=pd.Index(np.asarray(chrom, np.int64), name='CHROM'))


def evaluate_maps(f_maps, scales_bp=DEFAULT_SCALES_BP, key='region_params', labels=None, drop_flagged=False, tail='upper',
                  outliers_fdr=None, device=0, read_workers=None):
    """Accuracy and calibration of C maps on one grid at every scale of scales_bp (base pairs, multiples of the maps' window).

    Returns dict(report: a frame with one row per cohort and scale -- index COHORT, columns REPORT_COLUMNS --; labels; scales_bp;
    windows: per scale dict(run_ptr, CHROM, START, END host arrays [M], planes: dict(n_bins, y_true, y_pred, std, pval) device tensors
    [C, M]); outliers (with outliers_fdr, else None): per scale a list of C frames -- window_frame with QVAL -- of the windows whose
    Benjamini-Hochberg q-value over the cohort's testable windows is <= outliers_fdr, in grid order).
    The cohort-major tables are uploaded once; per scale run_ptr is built on the host and the two kernels run; only the scores, and
    the outliers' rows, cross back.  ValueError before a device is touched: a scale that is no multiple of the window, maps on
    different grids, a label count that differs from the map count, outliers_fdr outside (0, 1]."""
    files = [f_maps] if isinstance(f_maps, (str, bytes)) or hasattr(f_maps, "__fspath__") else list(f_maps)
    scales = check_options(len(files), labels, tail, outliers_fdr, scales_bp)
    files, tables, names = load_maps(files, key, read_workers)
    labels = list(labels) if labels is not None else default_labels(files, names)
    if len(set(labels)) != len(labels):
        raise ValueError("two maps share the label %r: pass labels" % [l for l in labels if labels.count(l) > 1][0])
    scales_in_bins(scales, tables.window)
    import torch
    from .._marshal import resolve_device
    dev = resolve_device(device)
    up = lambda a: torch.as_tensor(a, device=dev)
    mu, sd, y, flag = up(tables.mu_cm), up(tables.std_cm), up(tables.y_cm), up(tables.flag_cm) if drop_flagged else None
    rows, windows, outliers = [], {}, {} if outliers_fdr is not None else None
    for bp in scales:
        ptr, w_chrom, w_start, w_end = merged_runs(tables.chrom, tables.start, bp)
        planes = engine.map_windows(mu, sd, y, flag, up(ptr), drop_flagged=drop_flagged, tail=tail)
        sc = engine.map_scores(planes["n_bins"], planes["y_true"], planes["y_pred"], planes["pval"])
        d = report_rows(sc["counts"].cpu().numpy(), sc["sums"].cpu().numpy(), bp)
        rows.append(pd.DataFrame(d, index=pd.Index(labels, name='COHORT'))[REPORT_COLUMNS])
        windows[bp] = dict(run_ptr=ptr, CHROM=w_chrom, START=w_start, END=w_end, planes=planes)
        if outliers_fdr is not None:
            hit_ptr, idx, got = _select_outliers(planes, float(outliers_fdr))
            outliers[bp] = [window_frame(w_chrom[idx[a:b]], w_start[idx[a:b]], w_end[idx[a:b]], {k: v[a:b] for k, v in got.items()},
                                         got["qval"][a:b]) for a, b in zip(hit_ptr[:-1], hit_ptr[1:])]
    return dict(report=pd.concat(rows), labels=labels, scales_bp=scales, windows=windows, outliers=outliers)


def write_report(res, outdir, write_windows=False):
    """The files of `DigPretrain.py evaluateMaps`: outdir/map_report.txt; with write_windows outdir/<label>.windows_<bp>.txt; with
    outliers outdir/<label>.outliers_<bp>.txt.  Returns the paths."""
    os.makedirs(outdir, exist_ok=True)
    paths = [os.path.join(outdir, "map_report.txt")]
    mapfile.write_results_tsv(res["report"], paths[0])
    for bp in res["scales_bp"] if write_windows else ():
        w = res["windows"][bp]
        host = {k: v.cpu().numpy() for k, v in w["planes"].items()}
        for c, label in enumerate(res["labels"]):
            paths.append(os.path.join(outdir, "%s.windows_%d.txt" % (label, bp)))
            mapfile.write_results_tsv(window_frame(w["CHROM"], w["START"], w["END"], {k: v[c] for k, v in host.items()}), paths[-1])
    for bp in res["scales_bp"] if res["outliers"] is not None else ():
        for label, frame in zip(res["labels"], res["outliers"][bp]):
            paths.append(os.path.join(outdir, "%s.outliers_%d.txt" % (label, bp)))
            mapfile.write_results_tsv(frame, paths[-1])
    return paths
