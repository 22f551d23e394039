"""elementDriver for MANY cohorts in one pass over device-resident tables.

The reference runs one cohort per process: `DigPretrain.py elementModel` (genic_driver_tools.nonc_model) writes the
element frame, `DigDriver.py elementDriver` (transfer_tools.run_element_region_model, transfer_tools.py:969-1096) joins
the cohort's observed counts and computes the statistics block.  With C pretrained maps on one bin grid the same
arithmetic is a batch along the cohort axis:

    observed counts   dig_overlap_join_* + tabulate_gpu.tabulate_cohorts   -> OBS_* [E, C]     (mutation_tools.py:155-230)
    scale factors     genome mode, transfer_tools.py:129-159: unique mutations in unflagged bins / sum Y_PRED[~FLAG]
    element pipeline  dig_element_pipeline                                 -> every column of the result frames

and the result is one frame per cohort with the reference's column names, identical to what the per-cohort route
gives (tests/test_gpu_cohort_batch.py).

geneDriver (transfer_tools.run_gene_model, transfer_tools.py:789-874) is batched the same way -- run_gene_cohorts: C gene models
with one gene index, the coding rows of C cohorts counted by engine.gene_counts (dig_gene_row_keys + a key sort +
dig_gene_counts), then ONE dig_gene_stats launch and, when asked for, ONE dig_gene_selection launch over [G, C]
(tests/test_gpu_gene_cohorts.py).

elementDriver --f-sites (transfer_tools.run_sites_region_model, transfer_tools.py:1098-1169) likewise -- run_sites_cohorts: the sites
file encoded once, the rows of C cohorts matched exactly and counted by engine.site_counts (dig_site_match_count / keys + a key sort
+ dig_site_counts), then the statistics element-wise over [E, C] (tests/test_gpu_sites_cohorts.py).

quickDriver (onthefly_tools.DIG_onthefly: ad-hoc elements, no pretrained element model) likewise -- run_quick_cohorts: the elements'
context counts are one engine.element_context_counts launch over the bed12 (dig_element_context_counts), the grid's window contexts
one engine.count_contexts launch, and the rest is run_element_cohorts without its element container (tests/test_gpu_quick_cohorts.py).

targetDriver (transfer_tools.run_target_model, transfer_tools.py:876-967) likewise -- run_target_cohorts: the tested rows go the
gene route's way (engine.gene_counts), the scale factor's rows inside the panel are counted by engine.panel_counts
(dig_panel_row_keys + a key sort + dig_panel_counts), then ONE dig_gene_stats launch over [G, C]; count_cohort_mutations writes the
attributes of `DigPretrain.py countMutations` for C maps from one such call over all installed panels
(tests/test_gpu_target_cohorts.py).

What the routes share, each written once:
    _element_planes   overlaps, tabulation, scale callback, plan, unpack, gamma -> planes()     element_pass (element, calls, meta, power), quick
    _select_hits, _hit_frames, _check_cut   q-values, cut, row_select, gather, hit frames       run_element_calls, run_element_meta_calls
    _gene_row_counts, _gene_frame_columns, _gene_frame_done   rows -> gene_counts -> columns    gene, target
    _run_and_write    files written while the frames behind them are assembled                  the five run_and_write_*_cohorts
    _write_frames     finished frames to files, several at a time                               write_results, the calls', the groups' and the power files
    _writer_threads, _usable_cores   every pool's size, from the cores the process may use      all of the above, _encode_all_mutations
"""
import numpy as np
import pandas as pd

from .. import engine
from .._marshal import resolve_device
from ..data_tools import cohort_rows, mutation_tools, tabulate_gpu
from ..io import mapfile
from ..sequence_model import genic_driver_tools, nb_model
from ..sequence_model.genic_driver_tools import _usable_cores
from . import transfer_tools


def genome_scale_factors(tables, cohorts, device, dev_tables=None):
    """calc_scale_factor_efficient, genome mode (transfer_tools.py:129-159), for all cohorts: (#unique SNVs, #unique
    indels overlapping an unflagged bin) / sum of Y_PRED over unflagged bins.  `cohorts` = encode_mutations() dicts.
    The reference re-reads the intersected rows with read_mutation_file(drop_duplicates=True, unique_indels=True)
    (mutation_tools.py:22-43,45-104): two de-duplications one after the other.  Rows with the same mutation have the same
    coordinates, hence the same bins and the same "an overlapped bin is unflagged" answer, so the de-duplications commute with
    the intersection: they are per-row flags of the FILE (dedup_flags / dig_mutation_file_flags_host, formed where the file
    is parsed), and the device only joins, marks the rows that touch an unflagged bin and counts -- no sort (round 4 ran three
    torch.unique row sorts over the 11 M rows of 37 cohorts here: genome_scale_factors_by_sorting, kept as the cross-check)."""
    import torch
    bins = tabulate_gpu.ElementBlocks(tables.chrom, tables.start, tables.start + tables.window, np.arange(len(tables.start)),
                                      len(tables.start), device)
    mu_d, flag = (dev_tables[0], dev_tables[3]) if dev_tables is not None else \
        (torch.as_tensor(tables.mu, device=device), torch.as_tensor(tables.flag, device=device))
    cat = lambda k: cohort_rows.column(cohorts, k)
    chrom, cohort = cat("chrom"), cat("cohort")
    pm, pb = tabulate_gpu.overlap_pairs(bins, chrom, cat("start"), cat("end"))
    pm = pm.long()
    ok_pair = flag[bins.elt[pb.long()], cohort[pm]] == 0              # the overlapped bin is unflagged in that cohort
    ok = torch.zeros(chrom.numel(), dtype=torch.bool, device=device)
    ok[pm[ok_pair]] = True                                             # the row touches an unflagged bin
    snv = ok & (cat("first_row") != 0) & (cat("indel") == 0)
    ind = ok & (cat("first_indel") != 0)
    # rows are concatenated cohort by cohort: a cohort's count is a difference of two entries of the running sum (an index_add
    # of 11 M flags onto 37 addresses serialises on its atomics: 0.2 s)
    ends = torch.as_tensor(np.cumsum([c["chrom"].numel() for c in cohorts]), device=device)
    def per_cohort(mask):
        run = torch.cat([torch.zeros(1, dtype=torch.int64, device=device), torch.cumsum(mask.to(torch.int64), 0)])
        at = run[ends]
        return (at - torch.cat([at.new_zeros(1), at[:-1]])).double()
    n_snv, n_ind = per_cohort(snv), per_cohort(ind)
    exp_sum = engine.scale_suffstats(mu_d, flag)
    return n_snv / exp_sum, n_ind / exp_sum


def genome_scale_factors_by_sorting(tables, cohorts, device):
    """genome_scale_factors as round 4 formed it: the de-duplications as three torch.unique row sorts over the intersected
    rows (the cross-check of the flag form; tests/test_gpu_host_mirror.py)."""
    import torch
    C = len(cohorts)
    bins = tabulate_gpu.ElementBlocks(tables.chrom, tables.start, tables.start + tables.window, np.arange(len(tables.start)),
                                      len(tables.start), device)
    flag = torch.as_tensor(tables.flag, device=device)
    cat = lambda k, shift=None: cohort_rows.column(cohorts, k, shift=shift)
    pm, pb = tabulate_gpu.overlap_pairs(bins, cat("chrom"), cat("start"), cat("end"))
    pm = pm.long()
    cohort = cat("cohort")
    ok = flag[bins.elt[pb.long()], cohort[pm]] == 0                    # the overlapped bin is unflagged in that cohort
    # the reference re-reads the intersected rows with read_mutation_file(drop_duplicates=True, unique_indels=True)
    # (mutation_tools.py:22-43,45-104), i.e. two de-duplications one after the other:
    uid = cat("uid", cohort_rows.id_offsets(cohorts, "uid"))
    smp = cat("sample", cohort_rows.sample_offsets(cohorts))
    indel = cat("indel")
    gene = cat("gene", cohort_rows.id_offsets(cohorts, "gene"))
    pm_ok = pm[ok]
    # step 1, drop_duplicate_mutations (mutation_tools.py:106-108): first row of every (cohort, uid, sample)
    key, inv = torch.unique(torch.stack([cohort[pm_ok], uid[pm_ok], smp[pm_ok]], dim=1), dim=0, return_inverse=True)
    first = torch.full((key.shape[0],), torch.iinfo(torch.int64).max, dtype=torch.int64, device=device)
    first.scatter_reduce_(0, inv, pm_ok, reduce="amin", include_self=True)      # file order = row index
    is_ind = indel[first] != 0
    n_snv = torch.zeros(C, dtype=torch.float64, device=device).index_add_(0, key[~is_ind, 0], torch.ones(int((~is_ind).sum()), dtype=torch.float64, device=device))
    # step 2, get_unique_indels (mutation_tools.py:110-117): indels recurring in several samples count once per
    # (CHROM, START, END, REF, ALT, GENE) -- GENE is that of the row step 1 kept
    ind_key = torch.unique(torch.stack([key[is_ind, 0], key[is_ind, 1], gene[first[is_ind]]], dim=1), dim=0)
    n_ind = torch.zeros(C, dtype=torch.float64, device=device).index_add_(0, ind_key[:, 0], torch.ones(ind_key.shape[0], dtype=torch.float64, device=device))
    exp_sum = engine.scale_suffstats(torch.as_tensor(tables.mu, device=device), flag)
    return n_snv / exp_sum, n_ind / exp_sum


class _Stages:
    """Wall-clock per stage of run_element_cohorts (tools/e2e_bench.py): the device is drained at every boundary."""

    def __init__(self, sink, dev):
        import time
        self.sink, self.dev, self.clock, self.t = sink, dev, time.perf_counter, time.perf_counter()

    def mark(self, name):
        if self.sink is None:
            return
        import torch
        torch.cuda.synchronize(self.dev)
        now = self.clock()
        self.sink[name] = self.sink.get(name, 0.0) + (now - self.t)
        self.t = now


_PVAL_PLANES = {'PVAL_SNV_BURDEN': 1, 'PVAL_SAMPLE_BURDEN': 2, 'PVAL_INDEL_BURDEN': 5, 'PVAL_MUT_BURDEN': 6}     # in engine.ES_PLANES
_QVAL_COLUMNS = ['QVAL_' + k[5:] for k in _PVAL_PLANES]                 # in the order they stand behind the frame's columns


def element_pass(f_muts, f_pretrained, f_element_data, save_key, scale_factors=None, max_muts_per_sample=3e9,
                 max_muts_per_elt_per_sample=3e9, device=0, timings=None, read_workers=None, output_form="records",
                 keep_sample_keys=False):
    """The front half the four element routes share, and what their `element_pass=` argument takes: the three inputs read side by
    side, then _element_planes (the tabulation, the scale factors, the plan's pass and its unpacking).  Returns (planes, names,
    stages): `planes()` gives every plane a frame is built from as a device tensor, a cohort's column one contiguous row -- ELT_SIZE,
    R_SIZE, P_INDEL [E]; FLAG, R_OBS, MU, SIGMA, ALPHA, THETA (unscaled), P0, OBS_SNV, OBS_SAMPLES, OBS_INDEL [C, E]; S [7, C, E]
    (engine.ES_PLANES); CJ [C] -- `names` the element names and `stages` the _Stages of `timings`, marked up to "kernels".
    The three inputs are independent until the kernels need them, so they are read SIDE BY SIDE (round 5; one after the other
    they were 0.8 of the 1.5 s of a 37-cohort run): the maps (a thread per map), the element container, and the mutation
    files -- each parsed by the library's own parser and uploaded by its own thread as soon as it is parsed.
    keep_sample_keys: the tabulation's (cohort, element, sample) keys stay on the device beside the planes, as `planes.sample_keys`
    (tabulate_gpu.tabulate_cohorts, return_sample_keys), with the elements' blocks as `planes.elements`: what run_element_pairs
    needs.  Without it nothing is kept."""
    import time
    from concurrent.futures import ThreadPoolExecutor
    dev = resolve_device(device)
    assert len(f_muts) == len(f_pretrained) and len(f_muts) > 0
    C = len(f_muts)
    if read_workers is None:
        read_workers = min(C, _usable_cores()) if C >= 8 else 1
    st_ = _Stages(timings, dev)
    first = list(f_pretrained)[0]
    idx0 = mapfile.read_array(first, 'idx')
    w = int(idx0[0, 2] - idx0[0, 1])                        # the grid's window (RegionTables checks that every map has it)
    spans = {}

    def timed(name, fn):
        def run():
            t0 = time.perf_counter()
            out = fn()
            spans[name] = time.perf_counter() - t0
            return out
        return run

    def read_elements():
        elts_ = genic_driver_tools._element_set(f_element_data, w, save_key)
        si_index = mapfile.read_array(f_element_data, 'window_{}/full_window_si_index'.format(w))
        si_values = mapfile.read_array(f_element_data, 'window_{}/full_window_si_values'.format(w))
        return elts_, si_index, si_values

    if read_workers > 1:
        with ThreadPoolExecutor(max_workers=3) as pool:
            fut_maps = pool.submit(timed("read_maps", lambda: genic_driver_tools._load_cohorts(list(f_pretrained), workers=read_workers)))
            fut_elts = pool.submit(timed("read_element_data", read_elements))
            fut_muts = pool.submit(timed("parse_and_upload_mutation_files", lambda: _encode_all_mutations(f_muts, read_workers, device=dev)))
            files, tables, d_pr = fut_maps.result()
            elts, si_index, si_values = fut_elts.result()
            cohorts = fut_muts.result()
    else:
        files, tables, d_pr = timed("read_maps", lambda: genic_driver_tools._load_cohorts(list(f_pretrained), workers=1))()
        elts, si_index, si_values = timed("read_element_data", read_elements)()
        cohorts = timed("parse_and_upload_mutation_files", lambda: _encode_all_mutations(f_muts, 1, device=dev))()
    assert tables.window == w, "the maps' bin grid and the first map's idx disagree"
    ctx = tables.aligned_context(si_index, si_values)
    st_.mark("read_parse_upload")
    if timings is not None:
        timings["inside_read_parse_upload"] = {k: round(v, 4) for k, v in spans.items()}

    def scale(blacklists, dev_tables):
        if scale_factors is not None:
            return scale_factors
        print('Calculating scale factor')
        return genome_scale_factors(tables, cohorts, dev, dev_tables)
    return _element_planes(elts, tables, d_pr, ctx, cohorts, scale, max_muts_per_sample, max_muts_per_elt_per_sample, dev, st_,
                           output_form, keep_sample_keys), elts['names'], st_


_run_element_pass = element_pass                         # (the routes below take an argument of this name)


def _element_planes(elts, tables, d_pr, ctx, cohorts, scale, max_muts_per_sample, max_muts_per_elt_per_sample, dev, st_,
                    output_form="records", keep_sample_keys=False):
    """What the element and the quick route do alike once both hold the elements (elts: chrom, blk_ptr, blk_start, blk_end,
    strand_minus, L -- host arrays or device tensors), the maps' tables and d_pr, the grid's window contexts ctx and the encoded
    cohorts: the bin overlaps, the join and tabulation, the scale factors, the plan's pass, its unpacking and the Gamma parameters.
    scale(blacklists, dev_tables) -> (cj [C], cj_indel [C]) is the route's own rule, called once behind the tabulation (the quick
    route's expectation rule needs the samples the tabulation blacklisted).  Returns `planes`: planes() is the dict of device planes
    element_pass describes.  st_: the _Stages marked from "bin_overlaps" to "kernels"."""
    import torch
    C, E = len(cohorts), len(elts['blk_ptr']) - 1
    ov_ptr, ov_idx = engine.ideal_overlaps(elts['chrom'], elts['blk_ptr'], elts['blk_start'], elts['blk_end'], tables.window,
                                           tables.chrom, tables.start)
    st_.mark("bin_overlaps")
    print('Tabulating mutations')
    owner = np.repeat(np.arange(E), np.diff(elts['blk_ptr']))
    blocks = tabulate_gpu.ElementBlocks(elts['chrom'][owner], elts['blk_start'], elts['blk_end'], owner, E, dev)
    obs_snv, obs_smp, obs_ind, blacklists, *sample_keys = tabulate_gpu.tabulate_cohorts(
        blocks, cohorts, drop_duplicates=True, max_muts_per_sample=max_muts_per_sample,
        max_muts_per_elt_per_sample=max_muts_per_elt_per_sample, **(dict(return_sample_keys=True) if keep_sample_keys else {}))
    st_.mark("join_tabulate")
    dev_tables = tables.on_device(dev)                      # [N, C] on the device (uploaded cohort-major, transposed there)
    cj, cji = (x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, float), device=dev).reshape(C)
               for x in scale(blacklists, dev_tables))
    st_.mark("scale_factors")
    print('Calculating statistics')
    t = lambda a: a if torch.is_tensor(a) else torch.as_tensor(np.ascontiguousarray(a), device=dev)
    args = (*dev_tables, t(ctx), t(ov_ptr), t(ov_idx), t(elts['L']), t(elts['strand_minus']), t(d_pr))
    st_.mark("h2d")
    # The pass.  The statistics stage writes tile-blocked RECORDS (DIG_PIPE_RECORDS: one aligned run per 64-pair tile instead of
    # eleven store streams) and dig_element_records_unpack turns them into what the frames below want -- every plane cohort-major
    # ([C, E]: a cohort's column is one contiguous row; read with a stride of C values, the 24 columns of 37 frames were 0.35 s of
    # cache misses on the host) -- in ONE kernel; the plane form (`output_form="planes"`: eleven [E, C] arrays) needs a transpose per
    # plane behind the pass.  Same bits.  The general (192-substitution) form of the accumulation, as the per-cohort route runs it:
    # the same P to the last bit.
    by_cohort = lambda x: x.transpose(-1, -2).contiguous()
    # (element_rates=False, element_p=False: the plan runs ONCE -- a table of the rate sums, or of P, would be written and read for nothing)
    plan = engine.PipelinePlan(*args, obs_snv, obs_smp, obs_ind, compact=False, pack_bins=True, records_out=(output_form == "records"),
                               element_rates=False, element_p=False)
    if plan.records_out:
        acc, _ = plan.run(cj, cji)
        st_cm = torch.empty((len(engine.ES_PLANES), plan.C, plan.E), dtype=torch.float64, device=dev)
        rates = {k: torch.empty((plan.C, plan.E), dtype=kind, device=dev)
                 for k, kind in (("MU", torch.float64), ("SIGMA", torch.float64), ("R_OBS", torch.int32), ("FLAG", torch.int32))}
        plan.unpack(cohort_major=True, stats=st_cm, rates=rates)
        alpha, theta = nb_model.normal_params_to_gamma(rates["MU"], rates["SIGMA"])
        st_.mark("kernels")

        def planes():
            D = {k: v for k, v in acc.items() if k not in ('P', 'MU', 'SIGMA', 'R_OBS', 'FLAG')}
            D.update(rates, S=st_cm, ALPHA=alpha, THETA=theta)
            return D
    else:
        acc, st = plan.run(cj, cji)
        alpha, theta = nb_model.normal_params_to_gamma(acc["MU"], acc["SIGMA"])
        st_.mark("kernels")

        def planes():
            D = {k: (by_cohort(v) if v.dim() == 2 else v) for k, v in acc.items() if k != 'P'}              # (P [E, 1, C]: its one class below)
            D.update(S=by_cohort(st), ALPHA=by_cohort(alpha), THETA=by_cohort(theta))
            return D

    def all_planes():
        D = planes()
        D.update(P0=acc['P'][:, 0, :].transpose(0, 1).contiguous(), CJ=cj, OBS_SNV=by_cohort(obs_snv), OBS_SAMPLES=by_cohort(obs_smp),
                 OBS_INDEL=by_cohort(obs_ind))
        return D
    if keep_sample_keys:
        host = lambda a: a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        all_planes.sample_keys = sample_keys[0]
        all_planes.elements = {k: host(elts[k]) for k in ('chrom', 'blk_ptr', 'blk_start', 'blk_end')}
    return all_planes


def _element_columns(x, cj, have_indel, q=None):
    """The columns of one cohort's frame, in the frame's order, from host arrays: x maps a plane of element_pass to the cohort's row of
    it (S: [7, rows]) -- every element for run_element_cohorts, the hits for run_element_calls --, cj is the cohort's scale factor,
    q [4, rows] or None the q-values of the four PVAL columns."""
    S = x['S']
    d = {'ELT_SIZE': x['ELT_SIZE'], 'FLAG': x['FLAG'].astype(bool), 'R_SIZE': x['R_SIZE'], 'R_OBS': x['R_OBS'],
         'R_INDEL': x['R_OBS'], 'MU': x['MU'], 'SIGMA': x['SIGMA'], 'ALPHA': x['ALPHA'],
         'THETA': x['THETA'] * cj, 'MU_INDEL': x['MU'], 'SIGMA_INDEL': x['SIGMA'], 'ALPHA_INDEL': x['ALPHA'],
         'THETA_INDEL': S[3] if have_indel else x['THETA'], 'Pi_SUM': x['P0'], 'Pi_INDEL': x['P_INDEL'],
         'OBS_SAMPLES': x['OBS_SAMPLES'].astype(float), 'OBS_SNV': x['OBS_SNV'].astype(float), 'OBS_INDEL': x['OBS_INDEL'].astype(float),
         'EXP_SNV': S[0], 'PVAL_SNV_BURDEN': S[1], 'PVAL_SAMPLE_BURDEN': S[2]}
    if have_indel:                                           # transfer_tools.py:1079-1087
        d.update({'EXP_INDEL': S[4], 'PVAL_INDEL_BURDEN': S[5], 'PVAL_MUT_BURDEN': S[6]})
    if q is not None:
        d.update({k: q[i] for i, k in enumerate(_QVAL_COLUMNS[:4 if have_indel else 2])})
    return d


def _cohort_rows_of(X, c):
    """Cohort c's row of every host plane of element_pass (a per-element plane as it is, CJ left out)."""
    return {k: (v if v.ndim == 1 else v[:, c] if v.ndim == 3 else v[c]) for k, v in X.items() if k != 'CJ'}


def _ragged_qvalues(p):
    """p f64 [rows, n] on the device -> (the non-NaN values of every row as ragged lists: engine.row_select at cut = +inf, index
    left out; their Benjamini-Hochberg q-values within the row, in the lists' order: nb_model.bh_ragged)."""
    lists = engine.row_select(p, float("inf"), index=False)
    q = nb_model.bh_ragged(lists["score"], lists["row_ptr"])[0] if lists["score"].numel() else lists["score"].clone()
    return lists, q


def plane_qvalues(p):
    """Benjamini-Hochberg q-values along the last axis of an f64 device tensor [..., n], over the TESTABLE (non-NaN) values of every
    row: row r of the result holds the bits of nb_model.get_q_vals(p[r][~isnan(p[r])]) where p is a number and NaN where it is NaN.
    engine.row_select at cut = +inf takes the testable values out, nb_model.bh_ragged ranks them (dig_bh_qvalues_ragged),
    engine.row_scatter puts the q-values back; no argsort on the host."""
    import torch
    assert p.is_cuda and p.dtype == torch.float64
    flat = p.contiguous().reshape(-1, p.shape[-1])
    _, q = _ragged_qvalues(flat)
    return engine.row_scatter(flat, float("inf"), q, float("nan")).reshape(p.shape)


def _planes_of(given, *inputs):
    """(the device planes, the element names, the stages) of a route's element_pass= argument, or of element_pass(*inputs) without it."""
    planes, names, st_ = given or element_pass(*inputs)
    return planes(), names, st_


def _check_cut(pval_max, fdr, cut_on, what="cut_on"):
    """A cut's arguments, checked before a file is read: exactly one of pval_max / fdr, `cut_on` one of the four PVAL_*_BURDEN columns;
    returns its place among them (0..3).  what="best_on": the column run_element_meta ranks the members by, which no cut goes with."""
    if what == "cut_on" and (pval_max is None) == (fdr is None):
        raise ValueError("exactly one of pval_max and fdr must be given")
    if cut_on not in _PVAL_PLANES:
        raise ValueError("%s: one of %s" % (what, ", ".join(_PVAL_PLANES)))
    return list(_PVAL_PLANES).index(cut_on)


def _select_hits(P, j, pval_max, fdr):
    """The selection over the p-value planes P f64 [4, R, E] on the device (R rows: cohorts or groups), cut on plane j: the q-values of
    all four planes (_ragged_qvalues, scattered back: NaN where P is), the cut per row -- nb_model.bh_cut over the row's testable
    values of plane j at `fdr`, or `pval_max` for every row -- and engine.row_select at it.  Returns (Q f64 [4, R, E], hit_ptr host
    [R + 1], the hits' row and element as device index tensors, n_testable [R]: the non-NaN values of plane j)."""
    import torch
    _, R, E = P.shape
    pvals = P.reshape(4 * R, E)
    lists, q_lists = _ragged_qvalues(pvals)
    Q = engine.row_scatter(pvals, float("inf"), q_lists, float("nan")).reshape(4, R, E)
    ptr = lists["row_ptr"][j * R:(j + 1) * R + 1]                                     # the lists of plane j
    if fdr is not None:
        cuts = np.array([nb_model.bh_cut(lists["score"][ptr[r]:ptr[r + 1]], q_lists[ptr[r]:ptr[r + 1]], fdr) for r in range(R)])
    else:
        cuts = np.full(R, float(pval_max))
    hits = engine.row_select(pvals[j * R:(j + 1) * R], cuts)
    hit_ptr, elt = hits["row_ptr"], hits["index"].long()
    row = torch.as_tensor(np.repeat(np.arange(R), np.diff(hit_ptr)), device=elt.device)
    return Q, hit_ptr, row, elt, np.diff(ptr)


def _hit_frames(planes, hits, names, st_, columns):
    """One frame per row of _select_hits' `hits` from the device planes ([E], [R, E] or [k, R, E]) gathered at (row, element) -- only
    the hits cross to the host --: columns(r, x, q) gives row r's columns from its slice x of every plane and q [4, hits] of the
    q-values.  Index: the hits' element names; attrs['n_testable']."""
    Q, hit_ptr, row, elt, n_testable = hits
    at = lambda v: v[elt] if v.dim() == 1 else v[:, row, elt] if v.dim() == 3 else v[row, elt]
    X = {k: at(v).cpu().numpy() for k, v in planes.items()}
    q_hits, elt = at(Q).cpu().numpy(), elt.cpu().numpy()
    st_.mark("d2h")
    frames = []
    index = pd.Index(names, name='ELT')
    for r in range(len(hit_ptr) - 1):
        lo, hi = int(hit_ptr[r]), int(hit_ptr[r + 1])
        frames.append(pd.DataFrame(columns(r, {k: v[..., lo:hi] for k, v in X.items()}, q_hits[:, lo:hi]), index=index[elt[lo:hi]]))
        frames[-1].attrs['n_testable'] = int(n_testable[r])
    st_.mark("frames")
    return frames


def run_element_cohorts(f_muts, f_pretrained, f_element_data, save_key, scale_factors=None, max_muts_per_sample=3e9,
                        max_muts_per_elt_per_sample=3e9, device=0, timings=None, read_workers=None, on_frame=None,
                        output_form="records", qvalues=False, element_pass=None):
    """One result frame per cohort (index ELT, the columns of run_element_region_model) for the mutation files
    `f_muts[c]` against the pretrained maps `f_pretrained[c]` (one bin grid) and the element set `save_key` of
    `f_element_data`.  scale_factors: (cj [C], cj_indel [C]) or None for the genome mode.
    timings: dict that receives seconds per stage; read_workers: threads that parse the C mutation files and read the C
    maps side by side (default: min(C, cores) from 8 cohorts on, else 1 = in this process).
    on_frame(c, frame, columns, index): called as soon as cohort c's frame exists -- the frame, the dict of column arrays it was
    built from and its row index (run_and_write_element_cohorts hands them to a writer thread there, so that the result files
    are written while the next frames are assembled).
    output_form: "records" (default) or "planes" -- the layout the statistics stage writes on the device (same frames).
    qvalues: behind the columns of the frame, QVAL_SNV_BURDEN, QVAL_SAMPLE_BURDEN and, where the cohort has indel columns,
    QVAL_INDEL_BURDEN, QVAL_MUT_BURDEN: Benjamini-Hochberg over the column's non-NaN p-values (plane_qvalues; NaN where PVAL is).
    element_pass: what element_pass returned for the same inputs, for a caller that runs several routes behind ONE pass (the
    command line with --groups); the inputs are then not read again."""
    D, names, st_ = _planes_of(element_pass, f_muts, f_pretrained, f_element_data, save_key, scale_factors, max_muts_per_sample,
                               max_muts_per_elt_per_sample, device, timings, read_workers, output_form)
    if qvalues:
        Q = plane_qvalues(D['S'][list(_PVAL_PLANES.values())]).cpu().numpy()             # [4, C, E]
        st_.mark("qvalues")
    X = {k: v.cpu().numpy() for k, v in D.items()}
    st_.mark("d2h")
    frames = []
    index = pd.Index(names, name='ELT')                      # one object for all cohorts
    for c in range(len(f_muts)):
        d = _element_columns(_cohort_rows_of(X, c), X['CJ'][c], X['OBS_INDEL'][c].sum() != 0, Q[:, c] if qvalues else None)
        frames.append(pd.DataFrame(d, index=index))
        if on_frame is not None:
            on_frame(c, frames[-1], d, index)
    st_.mark("frames")
    return frames


def run_element_calls(f_muts, f_pretrained, f_element_data, save_key, pval_max=None, fdr=None, cut_on='PVAL_SNV_BURDEN',
                      scale_factors=None, max_muts_per_sample=3e9, max_muts_per_elt_per_sample=3e9, device=0, timings=None,
                      read_workers=None, output_form="records", element_pass=None):
    """The rows of run_element_cohorts(..., qvalues=True)'s frames that pass a cut, without the frames being built: frame c equals
    that frame restricted to the rows with `cut_on` <= pval_max, or with the q-value of `cut_on` <= fdr -- the same columns, dtypes,
    row order and bits.  Exactly one of pval_max / fdr; cut_on: one of the four PVAL_*_BURDEN columns (an indel column that a cohort
    lacks is a ValueError).  frame.attrs['n_testable']: the non-NaN values of cut_on in the cohort.
    fdr: p* per cohort from nb_model.bh_cut over the cohort's testable p-values ({q <= fdr} = {p <= p*}); the hits are
    engine.row_select at p* (pval_max: at pval_max), every column is gathered at (cohort, element) on the device, and only the hits
    cross to the host.  The other options as run_element_cohorts takes them."""
    j = _check_cut(pval_max, fdr, cut_on)
    D, names, st_ = _planes_of(element_pass, f_muts, f_pretrained, f_element_data, save_key, scale_factors, max_muts_per_sample,
                               max_muts_per_elt_per_sample, device, timings, read_workers, output_form)
    have_indel = (D['OBS_INDEL'].sum(dim=1) != 0).cpu().numpy()
    if j >= 2 and not have_indel.all():
        raise ValueError("cut_on = %s: cohorts %s have no indel columns" % (cut_on, [c for c in range(len(have_indel)) if not have_indel[c]]))
    hits = _select_hits(D['S'][list(_PVAL_PLANES.values())], j, pval_max, fdr)        # row k C + c: PVAL column k of cohort c
    st_.mark("qvalues_select")
    cj = D.pop('CJ').cpu().numpy()
    return _hit_frames(D, hits, names, st_, lambda c, x, q: _element_columns(x, cj[c], have_indel[c], q))


def run_and_write_element_calls(f_muts, f_pretrained, f_element_data, save_key, outdir, prefixes, write_threads=None, **kw):
    """run_element_calls with cohort c's hits written to <outdir>/<prefix>.hits.txt (mapfile.write_results_tsv, the OBS_* columns as
    integers like those of the results files), several files at a time as write_results writes them.  Returns (frames, paths)."""
    import os
    frames = run_element_calls(f_muts, f_pretrained, f_element_data, save_key, **kw)
    assert len(prefixes) == len(frames)
    return frames, _write_frames(frames, [os.path.join(outdir, pfx + '.hits.txt') for pfx in prefixes], write_threads)


# ---------------------------------------------------------------------------------------------
# meta-cohorts of the element route: groups of cohorts combined per element
# ---------------------------------------------------------------------------------------------
def _meta_groups(groups, labels, C):
    """The groups of run_element_meta checked before any file is read: (names, the members of every group as ascending cohort
    indices, labels as a list of str or None).  groups: an ordered dict group name -> list of cohort indices, or of labels from
    `labels` (one per cohort).  ValueError for no group, an empty group, an index outside [0, C), an unknown label or a repeated
    member."""
    if labels is not None:
        labels = [str(v) for v in labels]
        if len(labels) != C or len(set(labels)) != C:
            raise ValueError("labels: one label per cohort (%d), each once" % C)
    if not groups:
        raise ValueError("groups: at least one group")
    names, members = [], []
    for name, listed in groups.items():
        listed = list(listed)
        if not listed:
            raise ValueError("group %r is empty" % (name,))
        idx = []
        for v in listed:
            if isinstance(v, (int, np.integer)) and not isinstance(v, bool):
                if not 0 <= v < C:
                    raise ValueError("group %r: cohort index %d outside [0, %d)" % (name, v, C))
                idx.append(int(v))
            elif labels is None or str(v) not in labels:
                raise ValueError("group %r: unknown cohort label %r" % (name, v))
            else:
                idx.append(labels.index(str(v)))
        if len(set(idx)) != len(idx):
            raise ValueError("group %r names a cohort more than once" % (name,))
        names.append(str(name))
        members.append(sorted(idx))
    return names, members, labels


_N_TESTED_COLUMNS = ['N_TESTED_' + k[5:] for k in _PVAL_PLANES]


def _meta_planes(D, members, best_on):
    """The device half of the meta routes from the planes of element_pass: dict(P f64 [4, M, E] the combined _PVAL_PLANES, N i32
    [4, M, E] the members that tested, OBS f64 [3, M, E] the sums of OBS_SAMPLES, OBS_SNV, OBS_INDEL, EXP f64 [2, M, E] those of EXP_SNV
    and EXP_INDEL over the members that tested the SNV / the indel burden, BEST i64 [M, E] the member with the smallest p-value of
    plane `best_on` (ties: the lowest cohort; -1 where none tested), have_indel bool [C] on the host).  The indel and mut planes of a
    cohort without indel columns (the test of run_element_calls) count as not tested."""
    import torch
    S = D['S']
    C, E = D['MU'].shape
    have_indel = D['OBS_INDEL'].sum(dim=1) != 0
    P = S[list(_PVAL_PLANES.values())].clone()                                        # [4, C, E]
    P[2:, ~have_indel] = float("nan")
    member = torch.zeros((len(members), C), dtype=torch.uint8, device=S.device)
    for g, idx in enumerate(members):
        member[g, idx] = 1
    gf = engine.group_fisher(P, member)
    obs = engine.group_sums(torch.stack([D['OBS_SAMPLES'], D['OBS_SNV'], D['OBS_INDEL']]).double(), member)
    exp = engine.group_sums(torch.stack([S[0], S[4]]), member, gate=torch.stack([P[0], P[2]]))
    # one masked argmin per group, over its member rows only (the first of equal minima: the lowest cohort)
    best = []
    for g, idx in enumerate(members):
        at = torch.as_tensor(idx, device=S.device)
        rows = P[best_on][at]                                                         # [members, E]
        first = torch.where(rows.isnan(), float("inf"), rows).argmin(dim=0)
        best.append(torch.where(gf["n_used"][best_on, g] > 0, at[first], -1))
    return dict(P=gf["pval"], N=gf["n_used"], OBS=obs, EXP=exp, BEST=torch.stack(best), have_indel=have_indel.cpu().numpy())


def _meta_columns(x, n_members, have_indel, q, labels):
    """The columns of one group's frame, in the frame's order, from host arrays: x maps ELT_SIZE [rows], OBS [3, rows], EXP [2, rows],
    P [4, rows], N [4, rows], BEST [rows] of _meta_planes to the group's rows -- every element for run_element_meta, the hits for
    run_element_meta_calls --, have_indel whether a member of the group has indel columns, q [4, rows] or None the q-values."""
    n_p = 4 if have_indel else 2
    d = {'ELT_SIZE': x['ELT_SIZE'], 'N_COHORTS': np.full(len(x['ELT_SIZE']), n_members, np.int64),
         'OBS_SAMPLES': x['OBS'][0], 'OBS_SNV': x['OBS'][1], 'OBS_INDEL': x['OBS'][2], 'EXP_SNV': x['EXP'][0]}
    if have_indel:
        d['EXP_INDEL'] = x['EXP'][1]
    d.update({k: x['P'][i] for i, k in enumerate(list(_PVAL_PLANES)[:n_p])})
    d.update({k: x['N'][i].astype(np.int64) for i, k in enumerate(_N_TESTED_COLUMNS[:n_p])})
    if q is not None:
        d.update({k: q[i] for i, k in enumerate(_QVAL_COLUMNS[:n_p])})
    best = x['BEST'].astype(np.int64)
    d['BEST_COHORT'] = best if labels is None else np.array(labels + [''], dtype=object)[best]
    return d


def run_element_meta(f_muts, f_pretrained, f_element_data, save_key, groups, labels=None, qvalues=True, best_on='PVAL_SNV_BURDEN',
                     scale_factors=None, max_muts_per_sample=3e9, max_muts_per_elt_per_sample=3e9, device=0, timings=None,
                     read_workers=None, output_form="records", element_pass=None):
    """One frame per GROUP of cohorts (index ELT) from one pass of the element route over all cohorts: the cohorts' p-values combined
    per element by Fisher's method over the members that tested it (engine.group_fisher: chi2.sf(-2 sum ln p_c, 2 m); a NaN p did not
    test), and the counts summed (engine.group_sums).  groups: an ordered dict group name -> list of cohort indices, or of labels from
    `labels` (one per cohort); a cohort may be in many groups.  An unknown label, an empty list or a repeated member is a ValueError
    raised before any file is read.  Columns: ELT_SIZE, N_COHORTS (the members), OBS_SAMPLES, OBS_SNV, OBS_INDEL (sums over the
    members), EXP_SNV, EXP_INDEL (sums over the members that tested the SNV / the indel burden), the four PVAL_*_BURDEN combined, the
    four N_TESTED_*_BURDEN (the members behind each), with qvalues the four QVAL_*_BURDEN (Benjamini-Hochberg over the group's testable
    elements, plane_qvalues), and BEST_COHORT: the label (without labels: the index) of the member with the smallest p-value of
    `best_on`, ties to the lowest cohort index, '' (-1) where none tested.  The indel and mut planes of a cohort without indel columns
    count as not tested; a group in which no member has indel columns leaves out EXP_INDEL and its indel and mut columns, as a cohort's
    frame does.  The other options as run_element_cohorts takes them."""
    names_g, members, labels = _meta_groups(groups, labels, len(f_muts))
    j = _check_cut(None, None, best_on, "best_on")
    D, names, st_ = _planes_of(element_pass, f_muts, f_pretrained, f_element_data, save_key, scale_factors, max_muts_per_sample,
                               max_muts_per_elt_per_sample, device, timings, read_workers, output_form)
    T = _meta_planes(D, members, j)
    have_indel = T.pop('have_indel')
    Q = plane_qvalues(T['P']).cpu().numpy() if qvalues else None
    st_.mark("meta")
    X = {k: v.cpu().numpy() for k, v in T.items()}
    elt_size = D['ELT_SIZE'].cpu().numpy()
    st_.mark("d2h")
    frames = []
    index = pd.Index(names, name='ELT')
    for g, idx in enumerate(members):
        x = dict({k: v[:, g] for k, v in X.items() if k != 'BEST'}, BEST=X['BEST'][g], ELT_SIZE=elt_size)
        d = _meta_columns(x, len(idx), bool(have_indel[idx].any()), Q[:, g] if qvalues else None, labels)
        frames.append(pd.DataFrame(d, index=index))
        frames[-1].attrs['group'] = names_g[g]
    st_.mark("frames")
    return frames


def run_element_meta_calls(f_muts, f_pretrained, f_element_data, save_key, groups, labels=None, pval_max=None, fdr=None,
                           cut_on='PVAL_SNV_BURDEN', scale_factors=None, max_muts_per_sample=3e9, max_muts_per_elt_per_sample=3e9,
                           device=0, timings=None, read_workers=None, output_form="records", element_pass=None):
    """The rows of run_element_meta(..., qvalues=True, best_on=cut_on)'s frames that pass a cut, without the frames being built: frame
    g equals that frame restricted to the rows with the group's combined `cut_on` <= pval_max, or with its q-value <= fdr -- the same
    columns, dtypes, row order and bits.  Exactly one of pval_max / fdr; an indel column that a group lacks is a ValueError.  The
    selection is run_element_calls' over the groups' combined planes (nb_model.bh_cut, engine.row_select at p*, a gather at (group,
    element)); only the hits cross to the host.  frame.attrs['n_testable']: the non-NaN values of cut_on in the group."""
    j = _check_cut(pval_max, fdr, cut_on)
    names_g, members, labels = _meta_groups(groups, labels, len(f_muts))
    D, names, st_ = _planes_of(element_pass, f_muts, f_pretrained, f_element_data, save_key, scale_factors, max_muts_per_sample,
                               max_muts_per_elt_per_sample, device, timings, read_workers, output_form)
    T = _meta_planes(D, members, j)
    have_indel = np.array([bool(T['have_indel'][idx].any()) for idx in members])
    del T['have_indel']
    if j >= 2 and not have_indel.all():
        raise ValueError("cut_on = %s: groups %s have no indel columns" % (cut_on, [n for n, h in zip(names_g, have_indel) if not h]))
    hits = _select_hits(T['P'], j, pval_max, fdr)                                     # row k M + g: PVAL column k of group g
    st_.mark("meta_select")
    frames = _hit_frames(dict(T, ELT_SIZE=D['ELT_SIZE']), hits, names, st_,
                         lambda g, x, q: _meta_columns(x, len(members[g]), have_indel[g], q, labels))
    for g, frame in enumerate(frames):
        frame.attrs['group'] = names_g[g]
    return frames


def run_and_write_element_meta(f_muts, f_pretrained, f_element_data, save_key, groups, outdir, labels=None, write_threads=None, **kw):
    """run_element_meta -- with pval_max or fdr among the keywords run_element_meta_calls -- with group g's frame written to
    <outdir>/<group>.meta.results.txt (<group>.meta.hits.txt under a cut) as the cohorts' files are written (_write_one).  Returns
    (frames, paths)."""
    import os
    cut = kw.get('pval_max') is not None or kw.get('fdr') is not None
    run = run_element_meta_calls if cut else run_element_meta
    if not cut:
        kw = {k: v for k, v in kw.items() if k not in ('pval_max', 'fdr', 'cut_on')}
    frames = run(f_muts, f_pretrained, f_element_data, save_key, groups, labels=labels, **kw)
    sfx = '.meta.hits.txt' if cut else '.meta.results.txt'
    return frames, _write_frames(frames, [os.path.join(outdir, f.attrs['group'] + sfx) for f in frames], write_threads)


# ---------------------------------------------------------------------------------------------
# power of the element route: could an element that was not called have been called at all?
# ---------------------------------------------------------------------------------------------
_POWER_CUTS = {'PVAL_SNV_BURDEN': ('EXP_SNV', 0, 'OBS_SNV'), 'PVAL_SAMPLE_BURDEN': ('EXP_SNV', 0, 'OBS_SAMPLES'),
               'PVAL_INDEL_BURDEN': ('EXP_INDEL', 4, 'OBS_INDEL')}      # cut_on -> the EXP column, its plane of S, the OBS plane


def _check_power(pval_max, fdr, bonferroni, cut_on, folds, power_min, labels, C):
    """The arguments of run_element_power, checked before a file is read; returns (the folds as floats, their column labels)."""
    if sum(v is not None for v in (pval_max, fdr, bonferroni)) != 1:
        raise ValueError("exactly one of pval_max, fdr and bonferroni must be given")
    if cut_on == 'PVAL_MUT_BURDEN':
        raise ValueError("cut_on = PVAL_MUT_BURDEN has no critical count (Fisher's method over two tests): one of %s" % ", ".join(_POWER_CUTS))
    if cut_on not in _POWER_CUTS:
        raise ValueError("cut_on: one of %s" % ", ".join(_POWER_CUTS))
    folds = [float(f) for f in folds]
    tags = ['%g' % f for f in folds]
    if not 1 <= len(folds) <= engine.NB_POWER_MAX_FOLDS or not all(0.0 < f < float("inf") for f in folds) or len(set(tags)) != len(tags):
        raise ValueError("folds: one to %d different folds, each finite and > 0" % engine.NB_POWER_MAX_FOLDS)
    if not 0.0 < power_min <= 1.0:
        raise ValueError("power_min: a power within (0, 1]")
    if labels is not None and len(labels) != C:
        raise ValueError("labels: one label per cohort (%d)" % C)
    return folds, tags


def power_levels(P, pval_max=None, fdr=None, bonferroni=None):
    """The level of run_element_power per row of the p-value plane P f64 [C, E] on the device, by the one of the three rules that is
    given: (level f64 [C], n_testable [C]: the row's non-NaN values, n_hits [C]: its values <= the level; under fdr the row's hits at
    that FDR, from nb_model.bh_cut and engine.row_select_counts), host arrays.  A row without a testable value gets a NaN level."""
    C = int(P.shape[0])
    n_testable = (~P.isnan()).sum(dim=1).cpu().numpy()
    with np.errstate(all="ignore"):
        if fdr is not None:
            lists, q = _ragged_qvalues(P)
            ptr = lists["row_ptr"]
            cuts = np.array([nb_model.bh_cut(lists["score"][ptr[c]:ptr[c + 1]], q[ptr[c]:ptr[c + 1]], fdr) for c in range(C)])
            n_hits = engine.row_select_counts(P, cuts).sum(dim=1).cpu().numpy()
            level = float(fdr) * np.maximum(n_hits, 1) / n_testable
        else:
            level = np.full(C, float(pval_max)) if pval_max is not None else float(bonferroni) / n_testable
        level = np.where(n_testable > 0, level, np.nan)
    if fdr is None:
        n_hits = engine.row_select_counts(P, level).sum(dim=1).cpu().numpy()
    return level, n_testable, n_hits


def run_element_power(f_muts, f_pretrained, f_element_data, save_key, pval_max=None, fdr=None, bonferroni=None,
                      cut_on='PVAL_SNV_BURDEN', folds=(2.0, 5.0, 10.0), power_min=0.8, k_max=1 << 20, labels=None, scale_factors=None,
                      max_muts_per_sample=3e9, max_muts_per_elt_per_sample=3e9, device=0, timings=None, read_workers=None,
                      output_form="records", element_pass=None):
    """For every (cohort, element): the CRITICAL COUNT of the burden test `cut_on` at the cohort's level -- the smallest count at which
    the element would pass the cut -- and the POWER at it, the probability of reaching that count were the element under selection of
    fold f (the reference's alternative, selection_coefficient: the same ALPHA, THETA Pi times f); engine.nb_power over the planes of
    element_pass.  Returns (one frame per cohort, the per-element summary frame).
    Exactly one of the three levels; with n_c the non-NaN values of cut_on in cohort c:
        pval_max     the level is pval_max in every cohort
        bonferroni   bonferroni / n_c
        fdr          fdr max(h_c, 1) / n_c, h_c the cohort's hits at that FDR (nb_model.bh_cut, engine.row_select_counts): the
                     Benjamini-Hochberg line at the last rejected rank -- an element whose p-value fell below it would be called; a
                     cohort without hits gets the first step, fdr / n_c
    (n_c = 0: a NaN level, hence K_CRIT = -1 and NaN powers in that cohort).  cut_on: PVAL_SNV_BURDEN, PVAL_SAMPLE_BURDEN or
    PVAL_INDEL_BURDEN (PVAL_MUT_BURDEN has no critical count; an indel column that a cohort lacks is the ValueError of
    run_element_calls).  folds: one to eight different folds, finite and > 0.
    Frame c: index ELT; ELT_SIZE, EXP_<X>, OBS_<X>, the cut_on column, K_CRIT (-1: out of reach within k_max, or not defined),
    POWER_F<fold> per fold (the fold printed with %g; 0.0 where the level is out of reach, NaN where K is not defined), POWERED (bool:
    the power at the LARGEST fold >= power_min); attrs level, n_testable (n_c), n_hits (the elements with cut_on <= the level; h_c
    under fdr).
    Summary frame: index ELT; N_COHORTS_TESTED (the cohorts whose cut_on is a number), N_COHORTS_POWERED_F<fold> per fold (the cohorts
    with that power >= power_min, summed on the device), MIN_K_CRIT (the smallest K_CRIT >= 0 over the cohorts, -1 if none),
    BEST_COHORT (the cohort with the largest power at the largest fold, ties to the lowest cohort: its label from `labels`, without
    labels its index; '' (-1) where no cohort's power is a number).  The other options as run_element_cohorts takes them."""
    import torch
    folds, tags = _check_power(pval_max, fdr, bonferroni, cut_on, folds, power_min, labels, len(f_muts))
    D, names, st_ = _planes_of(element_pass, f_muts, f_pretrained, f_element_data, save_key, scale_factors, max_muts_per_sample,
                               max_muts_per_elt_per_sample, device, timings, read_workers, output_form)
    S = D['S']
    C, E = D['MU'].shape
    exp_name, exp_plane, obs_name = _POWER_CUTS[cut_on]
    indel = cut_on == 'PVAL_INDEL_BURDEN'
    if indel:
        have_indel = (D['OBS_INDEL'].sum(dim=1) != 0).cpu().numpy()
        if not have_indel.all():
            raise ValueError("cut_on = %s: cohorts %s have no indel columns" % (cut_on, [c for c in range(C) if not have_indel[c]]))
    P = S[_PVAL_PLANES[cut_on]]                                                       # [C, E]
    level, n_testable, n_hits = power_levels(P, pval_max, fdr, bonferroni)
    if indel:
        got = engine.nb_power(D['ALPHA'], S[3], D['P_INDEL'].expand(C, E).contiguous(), level, folds=folds, k_max=k_max)
    else:
        got = engine.nb_power(D['ALPHA'], D['THETA'], D['P0'], level, scale=D['CJ'], folds=folds, k_max=k_max)
    K, power = got["k_crit"], got["power"]                                            # [C, E], [F, C, E]
    # the summary over the cohort axis, on the device
    top = int(np.argmax(folds))
    n_powered = (power >= power_min).sum(dim=1)                                       # [F, E] (a NaN power is not >=)
    min_k = torch.where(K >= 0, K, torch.iinfo(torch.int32).max).min(dim=0).values
    min_k = torch.where((K >= 0).any(dim=0), min_k, -1)
    pw = torch.where(power[top].isnan(), float("-inf"), power[top])                   # [C, E]
    cohort = torch.arange(C, device=pw.device)[:, None]
    best = torch.where(pw == pw.max(dim=0).values, cohort, C).min(dim=0).values      # the lowest cohort among the largest powers
    best = torch.where(power[top].isnan().all(dim=0), -1, best)
    n_tested = (~P.isnan()).sum(dim=0)
    st_.mark("power")
    X = {k: v.cpu().numpy() for k, v in dict(ELT_SIZE=D['ELT_SIZE'], EXP=S[exp_plane], OBS=D[obs_name], P=P, K=K, POWER=power,
                                             N_POWERED=n_powered, MIN_K=min_k, BEST=best, N_TESTED=n_tested).items()}
    st_.mark("d2h")
    index = pd.Index(names, name='ELT')
    frames = []
    for c in range(C):
        d = {'ELT_SIZE': X['ELT_SIZE'], exp_name: X['EXP'][c], obs_name: X['OBS'][c].astype(float), cut_on: X['P'][c],
             'K_CRIT': X['K'][c].astype(np.int64)}
        d.update({'POWER_F' + t: X['POWER'][j, c] for j, t in enumerate(tags)})
        d['POWERED'] = X['POWER'][top, c] >= power_min
        frames.append(pd.DataFrame(d, index=index))
        frames[-1].attrs.update(level=float(level[c]), n_testable=int(n_testable[c]), n_hits=int(n_hits[c]))
    d = {'N_COHORTS_TESTED': X['N_TESTED'].astype(np.int64)}
    d.update({'N_COHORTS_POWERED_F' + t: X['N_POWERED'][j].astype(np.int64) for j, t in enumerate(tags)})
    d['MIN_K_CRIT'] = X['MIN_K'].astype(np.int64)
    best = X['BEST'].astype(np.int64)
    d['BEST_COHORT'] = best if labels is None else np.array([str(v) for v in labels] + [''], dtype=object)[best]
    st_.mark("frames")
    return frames, pd.DataFrame(d, index=index)


def run_and_write_element_power(f_muts, f_pretrained, f_element_data, save_key, outdir, prefixes, write_threads=None, **kw):
    """run_element_power (labels: the prefixes, unless given) with cohort c's frame written to <outdir>/<prefix>.power.txt and the
    summary frame to <outdir>/elements.power.txt, as the calls' files are written (_write_frames).  Returns (frames, summary, paths:
    the cohorts' files, then the summary's)."""
    import os
    kw.setdefault('labels', list(prefixes))
    frames, summary = run_element_power(f_muts, f_pretrained, f_element_data, save_key, **kw)
    assert len(prefixes) == len(frames)
    paths = [os.path.join(outdir, pfx + '.power.txt') for pfx in prefixes] + [os.path.join(outdir, 'elements.power.txt')]
    return frames, summary, _write_frames(frames + [summary], paths, write_threads)


# ---------------------------------------------------------------------------------------------
# pairs of the element route: co-occurrence and exclusivity of the called elements across a cohort's samples
# ---------------------------------------------------------------------------------------------
PAIR_COLUMNS = ['ELT_B', 'N_SAMPLES', 'N_A', 'N_B', 'N_BOTH', 'N_A_ONLY', 'N_B_ONLY', 'N_NEITHER', 'LOG2_ODDS', 'PVAL_COOCCUR',
                'PVAL_EXCLUSIVE', 'QVAL_COOCCUR', 'QVAL_EXCLUSIVE', 'TENDENCY']              # behind the index, ELT_A


def _check_pairs(pair_pval_max, pair_fdr, min_samples, n_samples, C):
    """run_element_pairs' own arguments, checked before a file is read."""
    if (pair_pval_max is None) == (pair_fdr is None):
        raise ValueError("exactly one of pair_pval_max and pair_fdr must be given")
    if int(min_samples) != min_samples or min_samples < 1:
        raise ValueError("min_samples: an integer >= 1, not %r" % (min_samples,))
    if n_samples is not None and (len(n_samples) != C or any(int(n) != n or n < 1 for n in n_samples)):
        raise ValueError("n_samples: one integer >= 1 per cohort (%d)" % C)


def overlapping_pairs(chrom, blk_ptr, blk_start, blk_end, elements):
    """The pairs (i < j) of positions in `elements` whose elements share a base: a block of one intersects a block of the other on one
    chromosome (blocks half-open).  A sweep on the host over the blocks of the listed elements in (chromosome, start) order, each
    against the blocks before it that are still open.  int64 [n, 2], ascending, without repeats."""
    elements = np.asarray(elements, np.int64)
    if len(elements) < 2:
        return np.zeros((0, 2), np.int64)
    n_blk = blk_ptr[elements + 1] - blk_ptr[elements]
    pos = np.repeat(np.arange(len(elements)), n_blk)
    blk = np.concatenate([np.arange(blk_ptr[e], blk_ptr[e + 1]) for e in elements]) if len(pos) else np.zeros(0, np.int64)
    ch, lo, hi = np.asarray(chrom)[elements][pos], np.asarray(blk_start)[blk], np.asarray(blk_end)[blk]
    order = np.lexsort((lo, ch))
    found, active = set(), []                                # active: (end, position) of the blocks that may still reach a later start
    last = None
    for b in order:
        if ch[b] != last:
            active, last = [], ch[b]
        active = [(e, q) for e, q in active if e > lo[b]]
        if hi[b] > lo[b]:
            found.update((min(q, pos[b]), max(q, pos[b])) for e, q in active if q != pos[b])
            active.append((hi[b], pos[b]))
    return np.array(sorted(found), np.int64).reshape(-1, 2)


def _pair_rows_of(slot, H):
    """(i, j) of the slots of one cohort's row-major upper triangle (engine.pair_index inverted), int64 arrays."""
    slot = np.asarray(slot, np.int64)
    i = np.floor(((2 * H - 1) - np.sqrt((2.0 * H - 1) ** 2 - 8.0 * slot)) / 2).astype(np.int64)
    i = np.clip(i, 0, max(H - 2, 0))
    for _ in range(2):                                       # (the square root may be off by one either way)
        i = np.where(engine.pair_index(i, i + 1, H) > slot, i - 1, i)
        i = np.where((i + 1 <= H - 2) & (engine.pair_index(i + 1, i + 2, H) <= slot), i + 1, i)
    return i, slot - engine.pair_index(i, i + 1, H) + i + 1


def run_element_pairs(f_muts, f_pretrained, f_element_data, save_key, pval_max=None, fdr=None, cut_on='PVAL_SNV_BURDEN',
                      pair_pval_max=None, pair_fdr=None, min_samples=1, n_samples=None, scale_factors=None, max_muts_per_sample=3e9,
                      max_muts_per_elt_per_sample=3e9, device=0, timings=None, read_workers=None, output_form="records",
                      element_pass=None):
    """How the calls of run_element_calls relate to each other across a cohort's samples: per cohort, for every pair of called elements,
    the samples hit in both and the two one-sided Fisher exact tests -- co-occurrence and exclusivity -- with Benjamini-Hochberg over
    the cohort's pairs (include/dig_hip.h and DESIGN, Pairs of the element route, state the rule; engine.pair_bits / engine.pair_fisher).
    The element cut (pval_max / fdr, cut_on) is run_element_calls'; the hits with OBS_SAMPLES >= min_samples enter, in the order of
    the hits frame (more than 8 192 of them in a cohort: ValueError).  Row h is the set of samples with a kept row in element h: the
    tabulation's own (cohort, element, sample) keys, so its size is OBS_SAMPLES.  The universe is the cohort's samples that the
    tabulation did not blacklist, or n_samples[c] >= that number (samples without a mutation are not in the file).
    Pairs whose elements share a base would co-occur through one mutation: their p-values are NaN (not testable, outside the
    Benjamini-Hochberg family), TENDENCY 'overlap', counts reported.  Exactly one of pair_pval_max / pair_fdr: a pair is reported when
    either p-value (q-value) passes; only the reported pairs and the overlapping ones cross to the host.
    One frame per cohort in pair order, index ELT_A, columns PAIR_COLUMNS; LOG2_ODDS = log2((N_BOTH + 1/2)(N_NEITHER + 1/2) /
    ((N_A_ONLY + 1/2)(N_B_ONLY + 1/2))), TENDENCY 'co-occurrence' where it is above 0, else 'exclusivity'.  attrs: n_elements,
    n_pairs, n_testable.  element_pass: what element_pass(..., keep_sample_keys=True) returned for the same inputs."""
    import torch
    j = _check_cut(pval_max, fdr, cut_on)
    C = len(f_muts)
    _check_pairs(pair_pval_max, pair_fdr, min_samples, n_samples, C)
    given = element_pass or _run_element_pass(f_muts, f_pretrained, f_element_data, save_key, scale_factors, max_muts_per_sample,
                                              max_muts_per_elt_per_sample, device, timings, read_workers, output_form, True)
    planes, names, st_ = given
    if not hasattr(planes, 'sample_keys'):
        raise ValueError("element_pass: made without keep_sample_keys=True")
    D = planes()
    dev = D['S'].device
    E = D['S'].shape[-1]
    have_indel = (D['OBS_INDEL'].sum(dim=1) != 0).cpu().numpy()
    if j >= 2 and not have_indel.all():
        raise ValueError("cut_on = %s: cohorts %s have no indel columns" % (cut_on, [c for c in range(C) if not have_indel[c]]))
    _, hit_ptr, row, elt, _ = _select_hits(D['S'][list(_PVAL_PLANES.values())], j, pval_max, fdr)
    st_.mark("qvalues_select")
    enters = D['OBS_SAMPLES'][row, elt] >= int(min_samples)
    row, elt = row[enters], elt[enters]
    rows = torch.bincount(row, minlength=C).cpu().numpy().astype(np.int64)              # H per cohort
    if rows.max(initial=0) > engine.PAIR_MAX_ROWS:
        raise ValueError("cohorts %s have more than %d entering elements (%s): raise min_samples (%d) or make the cut on %s stricter"
                         % ([c for c in range(C) if rows[c] > engine.PAIR_MAX_ROWS], engine.PAIR_MAX_ROWS, rows.max(), min_samples, cut_on))
    observed = np.asarray(planes.sample_keys['n_samples'], np.int64)
    n = observed if n_samples is None else np.asarray(n_samples, np.int64)
    if (n < observed).any():
        raise ValueError("n_samples: below the samples of the mutation file that were not blacklisted (%s) in cohorts %s"
                         % (observed.tolist(), np.nonzero(n < observed)[0].tolist()))
    H_total = int(rows.sum())
    # the bit matrix: the hit's place in the stacked matrix per (cohort, element), -1 elsewhere; one key per kept sample of an element
    place = torch.full((C * E,), -1, dtype=torch.int32, device=dev)
    place[row * E + elt] = torch.arange(H_total, dtype=torch.int32, device=dev)
    keys = planes.sample_keys['keys']
    bits = engine.pair_bits(place[keys[:, 0] * E + keys[:, 1]], keys[:, 2].to(torch.int32), H_total, engine.pair_words(int(n.max(initial=0))))
    got = engine.pair_fisher(bits, rows, n)
    st_.mark("pair_tests")
    row_ptr, pair_ptr = got['plan']['row_ptr'], got['pair_ptr']
    p = torch.stack([got['pval_cooccur'], got['pval_exclusive']])                      # [2, n_pairs]
    # the pairs that share a base: found on the host among the entering elements' blocks, set to NaN on the device
    elt_host, B = elt.cpu().numpy(), planes.elements
    shared = [overlapping_pairs(B['chrom'], B['blk_ptr'], B['blk_start'], B['blk_end'], elt_host[row_ptr[c]:row_ptr[c + 1]]) for c in range(C)]
    shared_slot = np.concatenate([pair_ptr[c] + engine.pair_index(s[:, 0], s[:, 1], int(rows[c])) for c, s in enumerate(shared)]
                                 or [np.zeros(0, np.int64)]).astype(np.int64)
    overlap = torch.zeros(p.shape[1], dtype=torch.bool, device=dev)
    overlap[torch.as_tensor(shared_slot, device=dev)] = True
    p[:, overlap] = float("nan")
    # Benjamini-Hochberg per cohort and column over the testable pairs: the ragged lists of the non-NaN values
    testable = ~p[0].isnan()
    before = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), testable.cumsum(0)])
    t_ptr = before[torch.as_tensor(pair_ptr, device=dev)].cpu().numpy()
    q = torch.full_like(p, float("nan"))
    if int(t_ptr[-1]):
        for k in range(2):
            q[k, testable] = nb_model.bh_ragged(p[k, testable], t_ptr)[0]
    st_.mark("pair_qvalues")
    level, by = (pair_fdr, q) if pair_fdr is not None else (pair_pval_max, p)
    at = torch.nonzero(((by <= level).any(dim=0)) | overlap)[:, 0]
    X = {k: v[..., at].cpu().numpy() for k, v in dict(P=p, Q=q, BOTH=got['n_both'], OVERLAP=overlap).items()}
    slot, n_row = at.cpu().numpy(), got['n_row'].cpu().numpy().astype(np.int64)
    st_.mark("d2h")
    frames = []
    names = np.asarray(names, dtype=object)
    for c in range(C):
        lo, hi = np.searchsorted(slot, [pair_ptr[c], pair_ptr[c + 1]])
        i, k = _pair_rows_of(slot[lo:hi] - pair_ptr[c], int(rows[c]))
        n_a, n_b, both = n_row[row_ptr[c] + i], n_row[row_ptr[c] + k], X['BOTH'][lo:hi].astype(np.int64)
        a_only, b_only = n_a - both, n_b - both
        neither = int(n[c]) - n_a - n_b + both
        odds = np.log2((both + 0.5) * (neither + 0.5) / ((a_only + 0.5) * (b_only + 0.5)))
        tendency = np.where(X['OVERLAP'][lo:hi], 'overlap', np.where(odds > 0, 'co-occurrence', 'exclusivity')).astype(object)
        d = {'ELT_B': names[elt_host[row_ptr[c] + k]], 'N_SAMPLES': np.full(hi - lo, int(n[c]), np.int64), 'N_A': n_a, 'N_B': n_b,
             'N_BOTH': both, 'N_A_ONLY': a_only, 'N_B_ONLY': b_only, 'N_NEITHER': neither, 'LOG2_ODDS': odds,
             'PVAL_COOCCUR': X['P'][0, lo:hi], 'PVAL_EXCLUSIVE': X['P'][1, lo:hi], 'QVAL_COOCCUR': X['Q'][0, lo:hi],
             'QVAL_EXCLUSIVE': X['Q'][1, lo:hi], 'TENDENCY': tendency}
        frames.append(pd.DataFrame(d, index=pd.Index(names[elt_host[row_ptr[c] + i]], name='ELT_A'), columns=PAIR_COLUMNS))
        frames[-1].attrs.update(n_elements=int(rows[c]), n_pairs=int(pair_ptr[c + 1] - pair_ptr[c]), n_testable=int(t_ptr[c + 1] - t_ptr[c]))
    st_.mark("frames")
    return frames


def run_and_write_element_pairs(f_muts, f_pretrained, f_element_data, save_key, outdir, prefixes, write_threads=None, **kw):
    """run_element_pairs with cohort c's frame written to <outdir>/<prefix>.pairs.txt (mapfile.write_results_tsv: the counts are
    integers), as the calls' files are written (_write_frames).  Returns (frames, paths)."""
    import os
    frames = run_element_pairs(f_muts, f_pretrained, f_element_data, save_key, **kw)
    assert len(prefixes) == len(frames)
    return frames, _write_frames(frames, [os.path.join(outdir, pfx + '.pairs.txt') for pfx in prefixes], write_threads)


def _writer_threads(n, write_threads=None):
    """For n files written side by side: (the worker threads, one per file up to the usable cores; the threads the native writer
    uses per file -- write_threads, or the cores shared out among the files, at most 8: the writer keeps one buffer per thread, so
    files side by side do not contend)."""
    cores = _usable_cores()
    return max(1, min(n, cores)), int(write_threads) if write_threads else max(1, min(8, cores // max(n, 1)))


def _write_frames(frames, paths, write_threads=None, workers=None):
    """Frame k written to paths[k] as _write_one writes it (the directories are made), several files at a time -- the native call
    does not hold the interpreter lock.  workers: the files in flight (default: _writer_threads; 1: one after the other, in this
    thread).  Returns paths."""
    import os
    from concurrent.futures import ThreadPoolExecutor
    jobs = list(zip(frames, paths))
    pool_size, threads = _writer_threads(len(jobs), write_threads)
    workers = pool_size if workers is None else int(workers)
    for d in set(os.path.dirname(p) for _, p in jobs):
        os.makedirs(d or '.', exist_ok=True)
    if workers <= 1 or len(jobs) <= 1:
        for frame, path in jobs:
            _write_one(frame, path, threads)
    else:
        with ThreadPoolExecutor(max_workers=workers) as pool:
            list(pool.map(lambda job: _write_one(job[0], job[1], threads), jobs))
    return list(paths)


def _run_and_write(run, n, outdir, prefixes, write_threads, writer):
    """frames = run(on_frame) with the result files written as the frames arrive: on_frame(c, *made) takes what the route hands over
    for cohort c, writer(path, threads, *made) -- called there, by the thread that assembles the frames -- returns the job a worker
    thread runs (the native writer holds no interpreter lock), and the frames of the cohorts after c are assembled meanwhile.
    Returns (frames, paths); the files are complete when the call returns."""
    import os
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(outdir, exist_ok=True)
    assert len(prefixes) == n
    paths = [os.path.join(outdir, pfx + '.results.txt') for pfx in prefixes]
    pool_size, threads = _writer_threads(n, write_threads)                # (threads: what the writer uses per file)
    pending = []
    with ThreadPoolExecutor(max_workers=pool_size) as pool:
        frames = run(lambda c, *made: pending.append(pool.submit(writer(paths[c], threads, *made))))
        for f in pending:
            f.result()
    return frames, paths


def run_and_write_element_cohorts(f_muts, f_pretrained, f_element_data, save_key, outdir, prefixes, write_threads=None, **kw):
    """run_element_cohorts + write_results with the two overlapped: cohort c's <outdir>/<prefix>.results.txt is written by a
    worker thread while the frames of the cohorts after it are assembled (_run_and_write)."""
    labels = []

    def writer(path, threads, frame, cols, index):
        # the writer takes the frame's COLUMN ARRAYS (the dict the frame was built from, the OBS_* columns as integers:
        # DigDriver.py:108-112) and the row labels encoded once: no pandas object is touched by a writer thread, whose
        # Python part is then a few microseconds (frame.assign + the column extraction of 37 writer threads held the
        # interpreter lock for 0.3 s of the 0.4 s the frames took)
        if not labels:
            labels.append(mapfile.encode_labels(index))
        out_cols = [(k, np.asarray(v).astype(np.int64) if k in ('OBS_SAMPLES', 'OBS_SNV', 'OBS_INDEL') else np.asarray(v)) for k, v in cols.items()]

        def write():
            # (row labels or a column the native writer does not cover -- a quote, a tab or a newline in an element name, an
            #  object column: encode_labels gives None / write_columns_tsv raises ValueError -- go the route write_results takes
            #  for them: pandas.  ADVICE r5: the run used to abort here, behind all the device work.)
            if labels[0] is not None:
                try:
                    return mapfile.write_columns_tsv(path, index.name, labels[0], out_cols, threads)
                except ValueError:
                    pass
            return _write_one(frame, path, threads)
        return write
    return _run_and_write(lambda on_frame: run_element_cohorts(f_muts, f_pretrained, f_element_data, save_key, on_frame=on_frame, **kw),
                          len(f_muts), outdir, prefixes, write_threads, writer)


def _write_one(df, path, threads):
    """One result file as DigDriver.py writes it (DigDriver.py:108-118: the OBS_* columns as integers)."""
    ints = {col: df[col].astype(int) for col in ('OBS_SAMPLES', 'OBS_SNV', 'OBS_INDEL') if col in df.columns}
    mapfile.write_results_tsv(df.assign(**ints), path, threads=threads)
    return path


def _encode_all_mutations(f_muts, workers=None, device=None):
    """The C mutation files as the host arrays of tabulate_gpu.encode_mutation_file, parsed and encoded side by side: a
    cohort's file is 10^5 - 10^6 rows (pandas: 0.45 s per 300 000; C of them one after the other were the largest stage of a
    many-cohort run).  Threads, not processes: pyarrow's reader and numpy's sorts release the interpreter lock, and worker
    processes would have to be spawned -- this process may hold the GPU -- which re-imports the caller's main module."""
    n = len(f_muts)
    workers = min(n, _usable_cores()) if workers is None else int(workers)
    # device: every file's arrays are uploaded by the thread that parsed it, as soon as it is parsed (round 4 uploaded the 37 x 8
    # arrays one after the other behind the last parse: 0.13 s of small pageable copies)
    def job(cf):
        enc = tabulate_gpu.encode_mutation_file(cf[1], cohort_id=cf[0])
        return enc if device is None else tabulate_gpu.to_device(enc, device)
    if workers <= 1 or n == 1:
        return [job(cf) for cf in enumerate(f_muts)]
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=workers) as pool:
        return list(pool.map(job, list(enumerate(f_muts))))


def write_results(frames, outdir, prefixes, workers=None):
    """<outdir>/<prefix>.results.txt per cohort, as DigDriver.py writes it (DigDriver.py:108-118: the OBS_* columns as
    integers, tab-separated, the index column first) -- through the native writer (mapfile.write_results_tsv: the bytes
    of DataFrame.to_csv), several files at a time (the native call does not hold the interpreter lock)."""
    import os
    os.makedirs(outdir, exist_ok=True)
    frames = list(frames)
    paths = [os.path.join(outdir, pfx + '.results.txt') for pfx in prefixes]
    workers = _writer_threads(min(len(frames), len(paths)))[0] if workers is None else int(workers)
    threads = _writer_threads(workers)[1]
    _write_frames(frames[:1], paths[:1], threads)            # (fills the label cache)
    _write_frames(frames[1:], paths[1:], threads, workers)
    return paths


# ---------------------------------------------------------------------------------------------
# geneDriver for many cohorts
# ---------------------------------------------------------------------------------------------
def _read_models(files, key, index_col, rename, differs, stacked, columns):
    """Frame `key` of the C maps as load_pretrained_model leaves it, without its per-map device calls: the frames are read, indexed
    by `index_col`, renamed and checked first (one index: ValueError `differs`, formatted with f = the first map that differs, first =
    the first map and key), then the `stacked` columns become f64 [n, C] planes and the Gamma parameters of every (MU, SIGMA) pair
    among them are ONE element-wise call over [n, C] (the same bits).  Returns (the frames with `columns`, dict name -> f64 [n, C])."""
    raw = []
    for f in files:
        m = mapfile.read_frame(f, key)
        m = m.set_index(m[index_col]).rename(columns=rename)
        if 'Pi_NONSYN' in columns:                                          # (the gene model's one derived column)
            m['Pi_NONSYN'] = m.Pi_MIS + m.Pi_TRUNC
        if raw and not m.index.equals(raw[0].index):
            raise ValueError(differs.format(f=f, first=list(files)[0], key=key))
        raw.append(m)
    planes = {col: np.ascontiguousarray(np.stack([m[col].values for m in raw], axis=1), dtype=np.float64) for col in stacked}
    pairs = [sfx for sfx in ('', '_INDEL') if 'MU' + sfx in planes]
    for sfx in pairs:
        planes['ALPHA' + sfx], planes['THETA' + sfx] = nb_model.normal_params_to_gamma(planes['MU' + sfx], planes['SIGMA' + sfx])
    frames = []
    for c, m in enumerate(raw):
        for sfx in pairs:
            m['ALPHA' + sfx], m['THETA' + sfx] = planes['ALPHA' + sfx][:, c], planes['THETA' + sfx][:, c]
        frames.append(m[columns])
    return frames, planes


def _read_gene_models(f_genemodels):
    """The C gene models (_read_models): the frames with _GENE_COLS_LEFT columns and the rate, Gamma and Pi_* planes f64 [G, C]."""
    tt = transfer_tools
    return _read_models(f_genemodels, 'genic_model', 'GENE', tt._GENE_RENAME,
                        "{f}: its gene model's gene index differs from that of {first} (run_gene_cohorts needs one gene index for all maps)",
                        ['MU', 'SIGMA', 'MU_INDEL', 'SIGMA_INDEL', 'Pi_INDEL'] + ['Pi_' + c for c in tt.GENE_CLASSES], tt._GENE_COLS_LEFT)


def _expected_syn_scale(genes, n_syn):
    """The scale factor of a cohort from its gene model (index GENE, renamed) and its synonymous row count: observed over expected
    synonymous mutations outside TP53 (transfer_tools.py:809-823,1116-1119: the serial routes' own pandas expression, the same bits)."""
    background = genes.loc[genes.index != 'TP53']
    return n_syn / (background.MU * background.Pi_SYN).sum()


_OBS_NAMES = ('OBS_SYN', 'OBS_MIS', 'OBS_NONS', 'OBS_SPL', 'OBS_INDEL')


def _restrict_gene_models(models, planes, keep):
    """The rows of the C gene models (and of their planes) whose gene is in the set `keep` (cgc_genes, a panel)."""
    inside = models[0].index.isin(keep)
    return [m.loc[inside] for m in models], {k: np.ascontiguousarray(v[inside]) for k, v in planes.items()}


def _gene_counts_on_host(counts):
    """engine.gene_counts' planes cohort-major on the host: obs i64 [C, 5, G], n_samp i64 [C, 6, G], n_samp_indel i64 [C, G],
    n_pairs [C, G]."""
    by_cohort = lambda x: x.transpose(-1, -2).contiguous().cpu().numpy()                     # [..., G, C] -> [..., C, G]
    obs_h = counts["obs"].permute(2, 1, 0).contiguous().cpu().numpy().astype(np.int64)       # [C, 5, G]
    n_samp_h = counts["n_samp"].permute(2, 1, 0).contiguous().cpu().numpy().astype(np.int64)
    return obs_h, n_samp_h, by_cohort(counts["n_samp_indel"]).astype(np.int64), by_cohort(counts["n_pairs"])


def _gene_burden_planes(planes, counts, cj, t_indel, dev):
    """ONE engine.gene_stats launch over [G, C] for the models' planes, the counts of engine.gene_counts, cj [C] and t_indel [C] (None:
    no indel block).  Returns (pi as a tensor [G, 6, C], dict plane name -> host array [C, G])."""
    import torch
    tt = transfer_tools
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    pi = t(np.stack([planes['Pi_' + c] for c in tt.GENE_CLASSES], axis=1))                    # [G, 6, C]
    st = engine.gene_stats(t(planes['MU']), t(planes['SIGMA']), pi, t(planes['Pi_INDEL']), counts["obs"], counts["n_samp"], t(cj),
                           None if t_indel is None else t(t_indel), mu_indel=t(planes['MU_INDEL']), sigma_indel=t(planes['SIGMA_INDEL']))
    return pi, {k: v.transpose(-1, -2).contiguous().cpu().numpy() for k, v in st.items()}


def _gene_count_columns(m, theta, obs, n_samp, n_samp_indel, n_pairs):
    """The columns of transfer_gene_model for one cohort: the model's (m), THETA as scaled, OBS_* (obs i64 [5, G]) and N_SAMP_* (n_samp
    i64 [6, G], n_samp_indel [G]); n_pairs [G]: the (gene, sample) pairs with a row of any class."""
    tt = transfer_tools
    d = {col: m[col].values for col in tt._GENE_COLS_LEFT}
    d['THETA'] = np.ascontiguousarray(theta)
    # a model gene without a row in the cohort's count table makes the serial route's left join fill with NaN: float columns
    kind = np.int64 if (n_pairs > 0).all() else np.float64
    for q, name in enumerate(_OBS_NAMES):
        d[name] = obs[q].astype(kind)
    d['OBS_TRUNC'] = d['OBS_NONS'] + d['OBS_SPL']
    d['OBS_NONSYN'] = d['OBS_MIS'] + d['OBS_TRUNC']
    for q, cls in enumerate(tt.GENE_CLASSES):
        d['N_SAMP_' + cls] = n_samp[q]
    d['N_SAMP_INDEL'] = n_samp_indel
    return d


def _burden_columns(d, S, c):
    """The twelve burden p-value columns of cohort c from the planes of _gene_burden_planes."""
    for pattern in ('PVAL_%s_BURDEN', 'PVAL_%s_BURDEN_SAMPLE'):
        for cls in transfer_tools.GENE_CLASSES:
            d[pattern % cls] = S[pattern % cls][c]
    return d


def _gene_row_counts(f_muts, index, keep, drop_synonymous, dev, max_muts_per_sample, max_muts_per_gene_per_sample):
    """The front half of the gene and the target route: the coding rows of every cohort encoded against the gene `index` (keep: the
    set of genes whose rows count, or None; drop_synonymous: without the Synonymous rows), stacked and counted by engine.gene_counts
    (TP53 apart, the hypermutator filter, the per-gene cap).  Returns (rows, their sample offsets, the device counts, the planes of
    _gene_counts_on_host)."""
    rows = [tabulate_gpu.encode_gene_rows(f, index, c, keep=keep) for c, f in enumerate(f_muts)]
    if drop_synonymous:
        for r in rows:
            kept = r["annot"] != 0
            for k in ("gene", "sample", "annot", "cohort"):
                r[k] = r[k][kept]
    G = len(index)
    tp53 = int(index.get_loc('TP53')) if 'TP53' in index else G + 1
    offsets = cohort_rows.sample_offsets(rows)
    stack = cohort_rows.place([cohort_rows.column(rows, k) for k in ("gene", "sample", "annot", "cohort")], True, dev)
    counts = engine.gene_counts(*stack, offsets, G, len(rows), tp53, max_muts_per_sample=max_muts_per_sample,
                                max_muts_per_gene_per_sample=max_muts_per_gene_per_sample)
    return rows, offsets, counts, _gene_counts_on_host(counts)


def _gene_frame_columns(m, theta, host, c):
    """The columns both gene-shaped frames start with: _gene_count_columns of cohort c from the planes of _gene_counts_on_host, then
    EXP_<class> = ALPHA THETA Pi_<class> (gene_expected_muts_nb: the serial route's own products)."""
    d = _gene_count_columns(m, theta, *(plane[c] for plane in host))
    rate = m.ALPHA.values * d['THETA']
    for cls in transfer_tools.GENE_CLASSES:
        d['EXP_' + cls] = rate * m['Pi_' + cls].values
    return d


def _gene_frame_done(frames, d, index, cj, on_frame):
    """The tail of both gene-shaped routes for the next cohort: its scale factor printed, its frame made, appended and handed on."""
    print("\tScaling factor of cohort {} is: {}".format(len(frames), cj))
    frames.append(pd.DataFrame(d, index=index))
    if on_frame is not None:
        on_frame(len(frames) - 1, frames[-1])


def run_gene_cohorts(f_muts, f_genemodels, scale_by_sample=False, pval_burden_nb=True, pval_burden_dnds=True, pval_sel=True,
                     max_muts_per_sample=3e9, max_muts_per_gene_per_sample=3e9, scale_factors=None, scale_by_expectation=True,
                     cgc_genes=False, all_cosmic=None, selection=False, device=0, on_frame=None):
    """geneDriver for C cohorts in one pass: one frame per cohort, with the columns, the column order and the dtypes of
    transfer_tools.run_gene_model(f_muts[c], f_genemodels[c], fused=True, ...) and the same keywords (scale_factors: an array [C]
    in place of scale_factor).  The gene models must share one gene index.  The sample and exome ratios (scale_by_sample, or
    neither scale_by_expectation nor scale_factors) need the maps' N_MUT_CDS bookkeeping and are not batched: NotImplementedError,
    before any device work.
    The observed counts, N_SAMP_*, the hypermutator filter and the synonymous row count come from engine.gene_counts over the
    rows of tabulate_gpu.encode_gene_rows; the scale factor's and the indel rate's denominators are the serial route's own pandas
    expressions over a cohort's model (G values each: the same bits); the statistics are one engine.gene_stats launch and, with
    selection=True, one engine.gene_selection launch over [G, C].
    on_frame(c, frame): called as soon as cohort c's frame exists."""
    import torch
    tt = transfer_tools
    C = len(f_muts)
    assert C > 0 and len(f_genemodels) == C
    if scale_by_sample or not (scale_by_expectation or scale_factors is not None):
        raise NotImplementedError("run_gene_cohorts scales by the expected synonymous count (scale_by_expectation) or by given "
                                  "scale_factors; the sample and exome ratios are run_gene_model's")
    if scale_factors is not None and not scale_by_expectation:
        scale_factors = np.asarray(scale_factors, float).reshape(C)
    models, planes = _read_gene_models(f_genemodels)
    keep = None
    if cgc_genes:
        keep = set(tt.gene_panel(cgc_genes))
        models, planes = _restrict_gene_models(models, planes, keep)
    index = models[0].index
    dev = resolve_device(device)
    _, _, counts, host = _gene_row_counts(f_muts, index, keep, False, dev, max_muts_per_sample, max_muts_per_gene_per_sample)
    by_cohort = lambda x: x.transpose(-1, -2).contiguous().cpu().numpy()                     # [..., G, C] -> [..., C, G]
    obs_h = host[0]
    n_syn = counts["n_syn"].cpu().numpy()

    # scale factors (transfer_tools.py:809-823) and the uniform indel rate (:709-721), a cohort at a time over G values
    if scale_by_expectation:
        print('scaling by expected synonymous mutations (excluding TP53)')
        cj = np.array([_expected_syn_scale(m, int(n_syn[c])) for c, m in enumerate(models)])
    else:
        cj = scale_factors
    theta = planes['THETA'] * 1.0 * cj[None, :]                          # (_attach_counts scales by 1.0, transfer_gene_model by cj)
    has_indel = obs_h[:, 4, :].sum(axis=1) != 0
    if not pval_burden_nb and has_indel.any():
        raise KeyError('PVAL_TRUNC_BURDEN')                              # (what the serial route's Fisher step says without the burden tests)
    t_indel = np.ones(C)
    if has_indel.any():
        null = ~index.isin(tt.cosmic_null_set(all_cosmic))
        for c in np.flatnonzero(has_indel):
            m = models[c].loc[null]
            t_indel[c] = pd.Series(obs_h[c, 4][null]).sum() / (m.Pi_INDEL * m.ALPHA_INDEL * m.THETA_INDEL).sum()

    print('Calculating statistics')
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    S = {}
    if pval_burden_nb:
        pi, S = _gene_burden_planes(planes, counts, cj, t_indel, dev)
    else:
        pi = t(np.stack([planes['Pi_' + c] for c in tt.GENE_CLASSES], axis=1))                # [G, 6, C]
    if selection:
        sel = engine.gene_selection(t(planes['ALPHA']), t(theta), pi, counts["obs"])
        S.update({k: by_cohort(v) for k, v in sel.items()})

    frames = []
    for c, m in enumerate(models):
        d = _gene_frame_columns(m, theta[:, c], host, c)
        if pval_burden_nb:
            if not selection:                                              # (EXP_<class> as the statistics kernel formed them)
                d.update({'EXP_' + cls: S['EXP_' + cls][c] for cls in tt.GENE_CLASSES})
            _burden_columns(d, S, c)
        if selection:
            names = ['T_SYN', 'MRFOLD'] + ['EXP_%s_ML' % cls for cls in tt.GENE_CLASSES]
            if pval_burden_dnds:
                names += ['PVAL_%s_BURDEN_DNDS' % cls for cls in tt.GENE_CLASSES]
            if pval_sel:
                names += ['PVAL_%s_SEL_NB' % cls for cls in tt._SEL_NB_CLASSES]
            for name in names:
                d[name] = S[name][c]
        if has_indel[c]:                                                   # (pval_burden_nb holds here)
            for name in ('THETA_INDEL', 'EXP_INDEL', 'PVAL_INDEL_BURDEN', 'PVAL_MUT_BURDEN'):
                d[name] = S[name][c]
        _gene_frame_done(frames, d, index, cj[c], on_frame)
    return frames


def run_and_write_gene_cohorts(f_muts, f_genemodels, outdir, prefixes, write_threads=None, **kw):
    """run_gene_cohorts + <outdir>/<prefix>.results.txt per cohort through the native writer, as `DigDriver.py geneDriver` writes
    it (mapfile.write_results_tsv of the frame as it is: the bytes of frame.to_csv), each file by a worker thread while the frames
    of the cohorts after it are assembled (_run_and_write)."""
    return _run_and_write(lambda on_frame: run_gene_cohorts(f_muts, f_genemodels, on_frame=on_frame, **kw), len(f_muts), outdir, prefixes,
                          write_threads, lambda path, threads, frame: lambda: mapfile.write_results_tsv(frame, path, threads))


# ---------------------------------------------------------------------------------------------
# targetDriver and countMutations for many cohorts
# ---------------------------------------------------------------------------------------------
def _panel_table(panels):
    """The label table of engine.panel_counts for the panels {name: genes} (at most 32): (labels: the union of their genes in order of
    first appearance, label_mask u32 [L]: bit p set for a gene of the p-th panel)."""
    if len(panels) > 32:
        raise ValueError("{} panels: a panel is a bit of a 32-bit mask".format(len(panels)))
    place, bits = {}, []
    for p, genes in enumerate(panels.values()):
        for gene in genes:
            if gene not in place:
                place[gene] = len(bits)
                bits.append(0)
            bits[place[gene]] |= 1 << p
    return list(place), np.array(bits, np.uint64).astype(np.uint32)


def _panel_counts_on_host(rows, label_mask, P, skip, device):
    """engine.panel_counts over the stacked rows of encode_panel_rows (device None: host arrays through the `_host` twins), its
    counts as host arrays."""
    if len(label_mask) == 0:                      # no panel at all: one label without a panel (every row carries it; n_cds still counts)
        label_mask = np.zeros(1, np.uint32)
    stack =cohort_rows.place([cohort_rows.column(rows, k) for k in ("label", "sample", "annot", "cohort")], device is not None, device)
    counts = engine.panel_counts(*stack, cohort_rows.sample_offsets(rows), label_mask, P, skip=skip, device=device or 0)
    return {k: (v.cpu().numpy() if engine.is_cuda(v) else np.asarray(v)) for k, v in counts.items()}


def run_target_cohorts(f_muts, f_genemodels, panel="MSK_341", scale_by_sample=False, max_muts_per_sample=3e9,
                       max_muts_per_gene_per_sample=3e9, drop_synonymous=True, cgc_genes=False, scale_factors=None, device=0,
                       on_frame=None):
    """targetDriver for C cohorts in one pass: one frame per cohort, with the columns, the column order, the dtypes and the values of
    transfer_tools.run_target_model(f_muts[c], f_genemodels[c], ...) and the same keywords (scale_factors: an array [C] in place of
    scale_factor; as there, a zero stands for "not given").  The gene models must share one gene index (ValueError); a map without the
    N_MUT_<panel> (scale_by_sample: N_SAMPLE_<panel>) attribute its scale factor needs: KeyError naming the map, before any device
    work.
    The tested rows (the panel's genes, or those of cgc_genes; without Synonymous rows when drop_synonymous) are counted by
    engine.gene_counts, which also gives the blacklist of max_muts_per_sample; the blacklist is carried by sample name onto the rows
    of tabulate_gpu.encode_panel_rows -- read_mutation_file(drop_duplicates=True) -- which engine.panel_counts counts inside the
    PANEL's genes: rows (or, scale_by_sample, distinct samples) whose ANNOT is none of Noncoding, Synonymous, Essential_Splice.  The
    scale factor is the serial route's own division by the map's attribute (the same bits); the statistics are one engine.gene_stats
    launch over [G, C], without the indel block (run_target_model has none).
    on_frame(c, frame): called as soon as cohort c's frame exists."""
    tt = transfer_tools
    f_muts, f_genemodels = list(f_muts), list(f_genemodels)
    C = len(f_muts)
    if C == 0 or len(f_genemodels) != C:
        raise ValueError("run_target_cohorts: {} mutation files for {} maps (one map per cohort, at least one cohort)".format(C, len(f_genemodels)))
    given = np.zeros(C) if scale_factors is None else np.asarray(scale_factors, float).reshape(-1)
    if len(given) != C:
        raise ValueError("run_target_cohorts: scale_factors must hold one value per cohort ({})".format(C))
    print(panel)
    panel_genes = tt.gene_panel(panel)
    tested = set(tt.gene_panel(cgc_genes)) if cgc_genes else set(panel_genes)
    attr = 'N_SAMPLE_{}'.format(panel) if scale_by_sample else 'N_MUT_{}'.format(panel)
    denom = {}
    for c in np.flatnonzero(given == 0):
        attrs = mapfile.read_attrs(f_genemodels[c])
        if attr not in attrs:
            raise KeyError("{}: no attribute {} (DigPretrain.py countMutations writes it; or pass scale_factors)".format(f_genemodels[c], attr))
        denom[c] = attrs[attr]
    models, planes = _read_gene_models(f_genemodels)
    models, planes = _restrict_gene_models(models, planes, tested)
    index = models[0].index
    dev = resolve_device(device)
    # row set A: the tested rows -> observed counts, N_SAMP_*, the blacklist
    rows, offsets, counts, host = _gene_row_counts(f_muts, index, tested, drop_synonymous, dev, max_muts_per_sample,
                                                   max_muts_per_gene_per_sample)

    # row set B: the scale factor's rows inside the panel, without the samples row set A blacklisted (carried over by name)
    cj = given.copy()
    if denom:
        black = counts["blacklisted"].cpu().numpy()
        labels, label_mask = _panel_table({panel: panel_genes})
        rows_b = [tabulate_gpu.encode_panel_rows(f, labels, c) for c, f in enumerate(f_muts)]
        off_b = cohort_rows.sample_offsets(rows_b)
        skip = np.zeros(int(off_b[-1]), np.uint8)
        for c in range(C):
            listed = set(name for j, name in enumerate(rows[c]["sample_names"]) if black[offsets[c] + j])
            if listed:
                skip[off_b[c]:off_b[c + 1]] = [name in listed for name in rows_b[c]["sample_names"]]
        inside = _panel_counts_on_host(rows_b, label_mask, 1, skip, dev)
        counted = inside["n_sample"] if scale_by_sample else inside["n_mut"]
        for c, d in denom.items():
            cj[c] = int(counted[c, 0]) / d                                # (CohortRun.panel_scale's own division)

    print('Calculating statistics')
    theta = planes['THETA'] * 1.0 * cj[None, :]                           # (_attach_counts scales by 1.0, transfer_gene_model by cj)
    _, S = _gene_burden_planes(planes, counts, cj, None, dev)
    frames = []
    for c, m in enumerate(models):
        d = _burden_columns(_gene_frame_columns(m, theta[:, c], host, c), S, c)
        _gene_frame_done(frames, d, index, cj[c], on_frame)
    return frames


def run_and_write_target_cohorts(f_muts, f_genemodels, outdir, prefixes, write_threads=None, **kw):
    """run_target_cohorts + <outdir>/<prefix>.results.txt per cohort through the native writer, as `DigDriver.py targetDriver` writes
    it (mapfile.write_results_tsv of the frame as it is), each file by a worker thread while the frames of the cohorts after it are
    assembled (_run_and_write)."""
    return _run_and_write(lambda on_frame: run_target_cohorts(f_muts, f_genemodels, on_frame=on_frame, **kw), len(f_muts), outdir,
                          prefixes, write_threads, lambda path, threads, frame: lambda: mapfile.write_results_tsv(frame, path, threads))


COUNT_PANELS = ('MSK_230', 'MSK_341', 'MSK_410', 'MSK_468', 'metabric_173', 'ucla_1202')     # DigPretrain.py:163-176


def count_cohort_mutations(f_muts, f_maps, write=True, device=0):
    """DigPretrain.py countMutations for C maps in one pass: the attribute dicts of count_training_mutations(f_muts[c] -> f_maps[c]),
    keys and values, from ONE engine.panel_counts call over the rows of all cohorts and all installed panels (a panel whose
    genes_<name>.txt is not found is skipped, as the serial function skips it).  N_SAMPLES is the length of the encoder's sample
    table, N_MUT_CDS (stored as N_MUT_SAMPLE_CDS too: the reference's slip, kept) the rows that are not Noncoding, N_MUT_TOTAL /
    N_MUT_TRAIN come from each map's region_params.  write=True stores every dict with mapfile.write_attrs.
    device: the card whose memory holds the rows while they are counted; None: host arrays through the `_host` twins."""
    f_muts, f_maps = list(f_muts), list(f_maps)
    C = len(f_muts)
    if C == 0 or len(f_maps) != C:
        raise ValueError("count_cohort_mutations: {} mutation files for {} maps (one map per cohort, at least one cohort)".format(C, len(f_maps)))
    panels = {}
    for name in COUNT_PANELS:
        try:
            panels[name] = transfer_tools.gene_panel(name)
        except FileNotFoundError:
            continue                               # panel list not installed
    labels, label_mask = _panel_table(panels)
    rows = [tabulate_gpu.encode_panel_rows(f, labels, c) for c, f in enumerate(f_muts)]
    counts = _panel_counts_on_host(rows, label_mask, max(len(panels), 1), None, device)
    out = []
    for c, f_map in enumerate(f_maps):
        df = mapfile.read_frame(f_map, 'region_params')
        flag = df.FLAG.values.astype(bool)
        attrs = {'N_MUT_TOTAL': int(df.Y_TRUE.sum()), 'N_MUT_TRAIN': int(df.Y_TRUE.values[~flag].sum()),
                 'N_SAMPLES': len(rows[c]["sample_names"]), 'N_MUT_CDS': int(counts["n_cds"][c]), 'N_MUT_SAMPLE_CDS': int(counts["n_cds"][c])}
        for p, name in enumerate(panels):
            attrs['N_MUT_' + name] = int(counts["n_mut"][c, p])
            attrs['N_MUT_SAMPLE_' + name] = int(counts["n_pairs"][c, p])
            if name == 'MSK_230':
                attrs['N_SAMPLE_MSK_230'] = int(counts["n_sample"][c, p])
        if write:
            mapfile.write_attrs(f_map, **attrs)
        out.append(attrs)
    return out


# ---------------------------------------------------------------------------------------------
# elementDriver --f-sites for many cohorts
# ---------------------------------------------------------------------------------------------
_SITE_MODEL_COLS = ['R_OBS'] + transfer_tools._RATE_COLS + ['Pi_SUM']         # transfer_element_model's left side


def _read_site_models(f_pretrained, pretrain_key):
    """The C element models of the sites route (_read_models): the frames with transfer_element_model's columns and the MU, SIGMA,
    Pi_SUM, ALPHA, THETA planes f64 [E, C]."""
    return _read_models(f_pretrained, pretrain_key, 'ELT', {'P_SUM': 'Pi_SUM', 'P_INDEL': 'Pi_INDEL'},
                        "{f}: the element index of its '{key}' model differs from that of {first} (run_sites_cohorts needs one element "
                        "index for all maps)", ('MU', 'SIGMA', 'Pi_SUM'), _SITE_MODEL_COLS)


def _empty_site_table():
    """mutation_tools.tabulate_sites_in_element for a cohort without a hit: its group-by over an empty merge."""
    none = pd.DataFrame({'ELT': pd.Series([], dtype=object), 'SAMPLE': pd.Series([], dtype=object), 'CHROM': pd.Series([], dtype=np.int64)})
    table = none.groupby('ELT').agg(OBS_SAMPLES=('SAMPLE', lambda x: len(set(x))), OBS_SNV=('CHROM', len)).reset_index()
    return table.set_index('ELT')[['OBS_SAMPLES', 'OBS_SNV']]


def run_sites_cohorts(f_muts, f_sites, f_pretrained, pretrain_key, scale_factors=None, scale_by_expectation=True, scale_type=None,
                      device=0, on_frame=None):
    """elementDriver --f-sites for C cohorts in one pass: one frame per cohort, with the columns, the column order, the row order
    (the model's index) and the dtypes of transfer_tools.run_sites_region_model(f_muts[c], f_sites, f_pretrained[c], pretrain_key,
    ...).  The `pretrain_key` models must share one element index.  Scale factors: the expected synonymous count outside TP53 over
    a cohort's own gene model (scale_by_expectation, the serial route's own pandas expression per cohort), or given scale_factors
    [C]; the MSK_230 and genome rules need the maps' bookkeeping and are not batched: NotImplementedError, before any device work.
    The sites file is read and encoded once (data_tools/sites.py), the rows of all cohorts are matched and counted by
    engine.site_counts (dig_site_match_count / keys + a key sort + dig_site_counts), the Gamma parameters of all maps are one
    element-wise call over [E, C] and the two mid-p columns one nb_pvalue_greater_midp call over the stacked [2, E, C] planes.
    device: the card whose memory holds the rows while they are counted; None: host arrays through the `_host` twins.
    on_frame(c, frame): called as soon as cohort c's frame exists."""
    from ..data_tools import sites
    C = len(f_muts)
    assert C > 0 and len(f_pretrained) == C
    given = None if scale_factors is None else np.asarray(scale_factors, float).reshape(C)
    if not scale_by_expectation and (given is None or not given.all()):
        raise NotImplementedError("run_sites_cohorts scales by the expected synonymous count (scale_by_expectation) or by given "
                                  "non-zero scale_factors; the {} rule is run_sites_region_model's".format(
                                      'MSK_230' if scale_type == 'MSK_230' else 'genome'))
    table = sites.encode_sites_file(f_sites)
    rows = [sites.encode_site_rows(f, table["dicts"], c) for c, f in enumerate(f_muts)]
    models, planes = _read_site_models(f_pretrained, pretrain_key)
    index = models[0].index
    offsets = cohort_rows.sample_offsets(rows)
    if offsets[-1] >= 2 ** 31:
        raise ValueError("{} samples: the global sample is 32-bit; pass fewer cohorts per call".format(int(offsets[-1])))
    E_sites = len(table["elt_names"])
    stack = [table[k] for k in ("site_pos", "site_end", "site_attr", "site_elt")] + [cohort_rows.column(rows, k) for k in ("pos", "end", "attr")] + \
        [cohort_rows.column(rows, "sample", shift=offsets), cohort_rows.column(rows, "cohort")]
    counts = engine.site_counts(*cohort_rows.place(stack, device is not None, device), offsets, E_sites, C)
    # site elements -> model rows: an element the model lacks is dropped, a model element no site names counts nothing
    place = pd.Index(table["elt_names"]).get_indexer(index) if E_sites else np.full(len(index), -1)
    host = lambda x: x.cpu().numpy() if engine.is_cuda(x) else np.asarray(x)
    take = lambda x: np.where(place[:, None] >= 0, host(x).astype(np.int64)[np.maximum(place, 0)], 0) if E_sites \
        else np.zeros((len(index), C), np.int64)
    obs_snv, obs_samples = take(counts["obs_snv"]), take(counts["obs_samples"])                # [E, C]
    counts_any = host(counts["obs_snv"]).any(axis=0) if E_sites else np.zeros(C, bool)         # (elements the model lacks included)

    if scale_by_expectation:
        print('scaling by expected synonymous mutations (excluding TP53)')
        cj = np.empty(C)
        for c, f in enumerate(f_pretrained):                               # (transfer_tools.py:1116-1119)
            genes = mapfile.read_frame(f, 'genic_model')
            cj[c] = _expected_syn_scale(genes.set_index(genes.GENE).rename(columns=transfer_tools._GENE_RENAME), rows[c]["n_syn"])
    else:
        cj = given
    print('Calculating statistics')
    theta = planes['THETA'] * cj[None, :]
    exp_snv = planes['ALPHA'] * theta * planes['Pi_SUM']
    with np.errstate(all="ignore"):
        prob = 1 / (theta * planes['Pi_SUM'] + 1)
    k = np.stack([obs_snv, obs_samples]).astype(np.float64)                                    # [2, E, C]
    pv = np.asarray(nb_model.nb_pvalue_greater_midp(k, np.broadcast_to(planes['ALPHA'], k.shape), np.broadcast_to(prob, k.shape)))

    frames = []
    for c, m in enumerate(models):
        d = {col: m[col].values for col in _SITE_MODEL_COLS}
        d['THETA'] = np.ascontiguousarray(theta[:, c])
        # a model element without a row in the cohort's count table makes the serial route's left join fill with NaN: float columns
        kind = np.int64 if len(index) and (obs_snv[:, c] > 0).all() else np.float64
        kinds = dict(OBS_SAMPLES=kind, OBS_SNV=kind)
        if not counts_any[c]:
            # no hit at all: the serial route's EMPTY count table has an object column, and what its join and fillna make of that is
            # pandas' choice, so its own expressions are asked (an empty table against the model: nothing is counted here)
            kinds = dict(transfer_tools.transfer_element_model(_empty_site_table(), m, 1.0)[['OBS_SAMPLES', 'OBS_SNV']].dtypes)
        d['OBS_SAMPLES'], d['OBS_SNV'] = obs_samples[:, c].astype(kinds['OBS_SAMPLES']), obs_snv[:, c].astype(kinds['OBS_SNV'])
        d['EXP_SNV'] = np.ascontiguousarray(exp_snv[:, c])
        d['PVAL_SNV_BURDEN'], d['PVAL_SAMPLE_BURDEN'] = np.ascontiguousarray(pv[0, :, c]), np.ascontiguousarray(pv[1, :, c])
        print("\tScale factor of cohort {} is: {}".format(c, cj[c]))
        frames.append(pd.DataFrame(d, index=index))
        if on_frame is not None:
            on_frame(c, frames[-1])
    return frames


def run_and_write_sites_cohorts(f_muts, f_sites, f_pretrained, pretrain_key, outdir, prefixes, write_threads=None, **kw):
    """run_sites_cohorts + <outdir>/<prefix>.results.txt per cohort through the native writer, as `DigDriver.py elementDriver
    --f-sites` writes it (DigDriver.py cmd_element: the OBS_* columns as integers), each file by a worker thread while the frames of
    the cohorts after it are assembled (_run_and_write)."""
    return _run_and_write(lambda on_frame: run_sites_cohorts(f_muts, f_sites, f_pretrained, pretrain_key, on_frame=on_frame, **kw),
                          len(f_muts), outdir, prefixes, write_threads, lambda path, threads, frame: lambda: _write_one(frame, path, threads))


# ---------------------------------------------------------------------------------------------
# quickDriver for many cohorts
# ---------------------------------------------------------------------------------------------
_QUICK_SCALE_TYPES = (None, 'genome')


def _quick_elements(f_elts_bed):
    """The elements of a bed12 as the single route reads them (mutation_tools.bed12_boundaries: autosomes only, bed order):
    (names, chrom i32, minus u8, blk_ptr, blk_start, blk_end i64) and the number of rows the bed file lists."""
    df = mutation_tools.bed12_boundaries(f_elts_bed)
    names = df.ELT.values
    if len(set(names.tolist())) != len(names):
        raise ValueError("{}: an element name occurs more than once (run_quick_cohorts needs one row per element)".format(f_elts_bed))
    blk_ptr = np.concatenate([[0], np.cumsum([len(b) for b in df.BLOCK_STARTS])]).astype(np.int64)
    blk_start = np.array([s for b in df.BLOCK_STARTS for s in b], np.int64)
    blk_end = np.array([e for b in df.BLOCK_ENDS for e in b], np.int64)
    minus = np.array([(s == '-1' or s == '-') for s in df.STRAND.astype(str)], np.uint8)     # onthefly_tools.py:126
    n_listed = len(pd.read_csv(f_elts_bed, sep="\t", header=None, usecols=[3]))
    return names, df.CHROM.values.astype(np.int32), minus, blk_ptr, blk_start, blk_end, n_listed


def opposite_strand_pair(names, chrom, minus, blk_ptr, blk_start, blk_end):
    """The first block (chrom, start, end) that elements of OPPOSITE strands share, as (element, other element, chrom, start, end),
    or None.  The single route counts such a block once, on the strand of its first occurrence, for both elements (the reference
    de-duplicates its frame of block counts by 'chr{}:{}-{}': sequence_tools.py:481-525); the element kernel counts every block on
    its own element's strand."""
    owner = np.repeat(np.arange(len(names)), np.diff(blk_ptr))
    if not len(owner):
        return None
    rows = np.stack([chrom[owner].astype(np.int64), blk_start, blk_end, minus[owner].astype(np.int64)], axis=1)
    uniq, first = np.unique(rows, axis=0, return_index=True)               # (sorted: the two strands of a block are neighbours)
    same = (uniq[1:, :3] == uniq[:-1, :3]).all(axis=1)
    if not same.any():
        return None
    hits = np.flatnonzero(same)
    k = hits[np.argmin(np.minimum(first[hits], first[hits + 1]))]          # the pair that appears first in the bed file
    a, b = sorted((int(first[k]), int(first[k + 1])))
    return names[owner[a]], names[owner[b]], int(uniq[k, 0]), int(uniq[k, 1]), int(uniq[k, 2])


def _quick_obs_sample_kinds(index, o_smp, n_listed):
    """The dtype of OBS_SAMPLES in tabulate_mutations_in_element(all_elements=True) (mutation_tools.py:155-189): the integer
    counts are left-joined onto the bed's rows, so they stay integers only when every listed row has a count."""
    return np.int64 if len(index) and n_listed == len(index) and (o_smp > 0).all() else np.float64


def run_quick_cohorts(f_muts, f_pretrained, f_fasta, f_elts_bed=None, region_str=None, scale_factors=None, scale_type=None,
                      scale_by_expectation=True, max_muts_per_sample=3e9, max_muts_per_elt_per_sample=3e9, skip_pvals=False,
                      all_cosmic=None, strict_reference=True, device=0, on_frame=None):
    """quickDriver for C cohorts in one pass: one frame per cohort with the columns, the column order, the dtypes, the row order
    and the index of onthefly_tools.DIG_onthefly(f_pretrained[c], f_muts[c], f_fasta, ...) with the same options -- burden tests
    for ad-hoc elements (a bed12 file, or a region string: the one-block '+' element UserELT) without a pretrained element model.
    The maps must share one bin grid.  What the single route takes from the FASTA one block row at a time -- L, through a frame
    keyed by strings and np.add.at -- is ONE engine.element_context_counts launch over the bed12 ([E, 64], expanded to the 192
    sorted substitution columns by a gather on the device); the window contexts of the grid are one engine.count_contexts launch
    over all N windows; then the bin overlaps, the join and tabulation and one engine.PipelinePlan run (the general form of the
    accumulation, as the single route runs it) as in run_element_cohorts.
    Scale factors, by the single route's own rules: scale_by_expectation (default; CohortRun.synonymous_scale and
    uniform_indel_scale over a cohort's coding rows without the samples the tabulation blacklisted: host work per cohort), else
    scale_factors = (cj [C], cj_indel [C]) as given, else scale_type 'genome' (genome_scale_factors); the other scale types need a
    map's bookkeeping and are not batched: NotImplementedError before any device work.
    strict_reference=True keeps the reference's double application of cj_indel to THETA_INDEL (DIG_onthefly) -- and refuses a bed
    file in which a block occurs in elements of opposite strands (ValueError naming the first pair: opposite_strand_pair);
    False counts such blocks per strand and applies cj_indel once.
    Only the bed's autosome rows are elements (bed12_boundaries); with other rows in the file OBS_SAMPLES is a float column.
    on_frame(c, frame): called as soon as cohort c's frame exists."""
    f_muts, f_pretrained = list(f_muts), list(f_pretrained)
    C = len(f_muts)
    if C == 0 or len(f_pretrained) != C:
        raise ValueError("run_quick_cohorts: {} mutation files for {} maps (one map per cohort, at least one cohort)".format(C, len(f_pretrained)))
    if not (f_elts_bed or region_str):
        raise ValueError("run_quick_cohorts: you must provide f_elts_bed or region_str")
    given = None
    if not scale_by_expectation:
        if scale_factors is not None:
            if len(scale_factors) != 2:
                raise ValueError("run_quick_cohorts: scale_factors is the pair (cj [C], cj_indel [C])")
            given = [np.asarray(x, float).reshape(-1) for x in scale_factors]
            if not all(len(x) == C for x in given):
                raise ValueError("run_quick_cohorts: scale_factors must hold one value per cohort ({})".format(C))
        elif scale_type not in _QUICK_SCALE_TYPES:
            raise NotImplementedError("run_quick_cohorts scales by the expected number of mutations (scale_by_expectation), by given "
                                      "scale_factors or by the genome rule; the {} rule is DIG_onthefly's".format(scale_type))
    temp_name = None
    if region_str and not f_elts_bed:                      # onthefly_tools.py:33-38
        import os
        import tempfile
        from .onthefly_tools import region_str_to_params
        ch, lo, hi = region_str_to_params(region_str)
        handle, temp_name = tempfile.mkstemp()
        with os.fdopen(handle, "w") as bed:
            bed.write("\t".join(str(x) for x in (ch, lo, hi, "UserELT", 0, "+", 0, 0, ".", 1, "%d," % (hi - lo), "0,")))
        f_elts_bed = temp_name
    try:
        names, chrom, minus, blk_ptr, blk_start, blk_end, n_listed = _quick_elements(f_elts_bed)
    finally:
        if temp_name:
            import os
            os.remove(temp_name)
    if strict_reference:
        pair = opposite_strand_pair(names, chrom, minus, blk_ptr, blk_start, blk_end)
        if pair is not None:
            raise ValueError("elements {} and {} lie on opposite strands and share the block chr{}:{}-{}: the reference counts such a "
                             "block once, on the strand of its first occurrence, for both elements; pass strict_reference=False to "
                             "count it on each element's own strand".format(*pair))
    # the arguments are checked: the device work
    import torch
    from ..sequence_model import sequence_tools
    dev = resolve_device(device)
    files, tables, d_pr = genic_driver_tools._load_cohorts(f_pretrained, workers=None if C >= 8 else 1)
    w = tables.window
    cohorts = _encode_all_mutations(f_muts, None if C >= 8 else 1, device=dev)
    genome = sequence_tools.load_genome(f_fasta)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    # L: the elements' strand-aware context counts from the 2-bit genome, every sorted substitution column its context's count
    # (sequence_tools._context_columns: the rule of nonc_elt_context_count)
    print('Counting element contexts')
    L64 = engine.element_context_counts(genome, ['chr' + str(c) for c in chrom], minus, blk_ptr, blk_start, blk_end, device=dev,
                                        on_device=True)
    _, cols = sequence_tools._context_columns(sequence_tools.mk_trans_idx(n_up=1, n_down=1, collapse=False))
    L = L64[:, t(cols)].contiguous()
    # the window contexts of the whole grid (onthefly_tools.py:118-120 counts the touched windows; DESIGN.md section 8.3: all of them
    # cost under a millisecond)
    ctx = engine.count_contexts(genome, ['chr' + str(c) for c in tables.chrom], tables.start, tables.start + w, device=dev)
    cji_h = []

    def scale(blacklists, dev_tables):
        if scale_by_expectation:                           # onthefly_tools.py:44-63, a cohort at a time on the host
            print('scaling by expected number of mutations')
            cj, cji = np.empty(C), np.empty(C)
            null = transfer_tools.cosmic_null_set(all_cosmic)
            for c in range(C):
                run = transfer_tools.CohortRun(f_muts[c], files[c])
                coding = run.coding_rows()
                coding = coding.loc[~coding.SAMPLE.astype(str).isin(set(str(s) for s in blacklists[c]))]
                cj[c] = run.synonymous_scale(run.gene_model(), coding, dedup=True)
                cji[c] = run.uniform_indel_scale(run.gene_model(), coding, null)
        elif given is not None:
            cj, cji = given
        else:
            print('Calculating scale factor')
            cj, cji = (x.cpu().numpy() for x in genome_scale_factors(tables, cohorts, dev, dev_tables))
        cji_h.append(cji)
        # THETA_INDEL: the reference scales it by cj_indel where the frame is made and again in element_pvalue_indel
        # (onthefly_tools.py:151,181); once without strict_reference
        return cj, cji * cji if strict_reference else cji
    elts = dict(chrom=chrom, blk_ptr=blk_ptr, blk_start=blk_start, blk_end=blk_end, strand_minus=minus, L=L)
    planes = _element_planes(elts, tables, d_pr, ctx, cohorts, scale, max_muts_per_sample, max_muts_per_elt_per_sample, dev,
                             _Stages(None, dev))
    X = {k: v.cpu().numpy() for k, v in planes().items()}
    frames = []
    index = pd.Index(np.asarray(names, dtype=object), name='ELT')
    for c in range(C):
        d = _quick_columns(_cohort_rows_of(X, c), X['CJ'][c], cji_h[0][c], index, n_listed, skip_pvals, strict_reference)
        frames.append(pd.DataFrame(d, index=index))
        if on_frame is not None:
            on_frame(c, frames[-1])
    return frames


def _quick_columns(x, cj, cji, index, n_listed, skip_pvals, strict_reference):
    """The columns of one cohort's quick frame from the rows _cohort_rows_of gives _element_columns -- a builder of its own because the
    frame is DIG_onthefly's, not run_element_region_model's: the columns of df_mut_tab.merge(pretrain_df) (onthefly_tools.py:104-112:
    the OBS_* first), then the statistics in the order they are added; FLAG stays the int32 of the merge; OBS_SAMPLES has the dtype
    rule of the left join (_quick_obs_sample_kinds); skip_pvals leaves THETA_INDEL the frame's own product with cji (once more
    under strict_reference) and drops the tests; and the indel columns are there whether or not the cohort has an indel."""
    S, th = x['S'], x['THETA']
    d = {'OBS_SAMPLES': x['OBS_SAMPLES'].astype(_quick_obs_sample_kinds(index, x['OBS_SAMPLES'], n_listed)),
         'OBS_SNV': x['OBS_SNV'].astype(float), 'OBS_INDEL': x['OBS_INDEL'].astype(float), 'ELT_SIZE': x['ELT_SIZE'], 'FLAG': x['FLAG'],
         'R_SIZE': x['R_SIZE'], 'R_OBS': x['R_OBS'], 'R_INDEL': x['R_OBS'], 'MU': x['MU'], 'SIGMA': x['SIGMA'], 'ALPHA': x['ALPHA'],
         'THETA': th * cj, 'MU_INDEL': x['MU'], 'SIGMA_INDEL': x['SIGMA'], 'ALPHA_INDEL': x['ALPHA'],
         'THETA_INDEL': (th * cji if strict_reference else th) if skip_pvals else S[3],
         'Pi_SUM': x['P0'], 'Pi_INDEL': x['P_INDEL'], 'EXP_SNV': S[0]}
    if not skip_pvals:
        d.update({'PVAL_SNV_BURDEN': S[1], 'PVAL_SAMPLE_BURDEN': S[2], 'EXP_INDEL': S[4], 'PVAL_INDEL_BURDEN': S[5],
                  'PVAL_MUT_BURDEN': S[6]})
    return d


def run_and_write_quick_cohorts(f_muts, f_pretrained, f_fasta, outdir, prefixes, write_threads=None, **kw):
    """run_quick_cohorts + <outdir>/<prefix>.results.txt per cohort through the native writer, as `DigDriver.py quickDriver` writes
    it (the OBS_* columns as integers), each file by a worker thread while the frames of the cohorts after it are assembled
    (_run_and_write)."""
    return _run_and_write(lambda on_frame: run_quick_cohorts(f_muts, f_pretrained, f_fasta, on_frame=on_frame, **kw), len(f_muts), outdir,
                          prefixes, write_threads, lambda path, threads, frame: lambda: _write_one(frame, path, threads))
