#!/usr/bin/env python
"""DigDriver.py -- command line of the burden tests on MI355X.

Drop-in for the reference's scripts/DigDriver.py: the same four sub-commands with the same positional
arguments and option names (DigDriver.py:160-275), and the same output, a tab-separated
``<outdir>/<outpfx>.results.txt`` with header and index column (DigDriver.py:38-43,115-118); and `tileDriver`, which the
reference does not have: the per-base scan of many cohorts, written as ``<outdir>/<outpfx>.hits.txt``; and `quickCohorts`,
`quickDriver` for many cohorts in one pass, one ``<outdir>/<outpfx>.results.txt`` per cohort; and `targetCohorts` and
`geneCohorts`, the same for `targetDriver` and `geneDriver`; and `elementCohorts`, the same for `elementDriver`, with q-values and,
at a cut, only the hits (``<outdir>/<outpfx>.hits.txt``).  The statistics
run through libdig_hip.so; `model` may be the reference's HDF5 map (`*.h5`, read by io/h5lite.py +
io/pandas_fixed.py: no h5py or PyTables needed) or the directory mirror described in digdriver_amd/io/mapfile.py.
"""
import argparse
import functools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from digdriver_amd.driver_model import transfer_tools  # noqa: E402
from digdriver_amd.io import mapfile  # noqa: E402

PANELS = ['MSK_230', 'MSK_341', 'MSK_410', 'MSK_468', 'metabric_173', 'ucla_1202']
CGC_SETS = ['CGC_ALL', 'CGC_ONC', 'CGC_TSG']
SCALE_TYPES = ['genome', 'exome', 'sample', 'MSK_230', 'PCAWG_cds']


def _use_panel_dir(args):
    if getattr(args, 'panel_dir', None):
        transfer_tools.set_panel_dir(args.panel_dir)


def write_results(frame, args):
    os.makedirs(args.outdir, exist_ok=True)
    target = os.path.join(args.outdir, args.outpfx + '.results.txt')
    print('\tSaving results to {}'.format(target))
    mapfile.write_results_tsv(frame, target)               # the bytes of frame.to_csv(target, header=True, index=True, sep="\t")


def cmd_gene(args):
    _use_panel_dir(args)
    print('Running gene driver detection')
    res = transfer_tools.run_gene_model(
        args.fmut, args.model, scale_by_sample=args.scale_by_samples, pval_burden_nb=args.pval_burden,
        max_muts_per_sample=args.max_muts_per_sample, max_muts_per_gene_per_sample=args.max_muts_per_gene_per_sample,
        scale_factor=args.scale_factor_manual, scale_by_expectation=args.scale_by_expectation, cgc_genes=args.cgc_genes,
        fused=True, selection=args.selection, pval_burden_dnds=args.pval_burden_dnds, pval_sel=args.pval_sel)
    write_results(res, args)


def cmd_target(args):
    _use_panel_dir(args)
    print('Running MSK-IMPACT driver detection')
    res = transfer_tools.run_target_model(
        args.fmut, args.model, scale_by_sample=args.scale_by_samples, panel=args.panel,
        max_muts_per_sample=args.max_muts_per_sample, max_muts_per_gene_per_sample=args.max_muts_per_gene_per_sample,
        cgc_genes=args.cgc_genes, scale_factor=args.scale_factor_manual, drop_synonymous=False)
    write_results(res, args)


def _scale_mode(args):
    """Expectation scaling is the default; naming a scale type or a manual factor switches it off, and manual
    factors must come as a pair (DigDriver.py:74-80)."""
    args.scale_by_expectation = not (args.scale_type or args.scale_factor_manual)
    if args.scale_factor_manual or args.scale_factor_indel_manual:
        if not (args.scale_factor_manual and args.scale_factor_indel_manual):
            raise SystemExit("ERROR: must specify both --scale-factor-manual and --scale-factor-indel-manual.")


def cmd_element(args):
    _use_panel_dir(args)
    if not (args.f_bed or args.f_sites):
        raise SystemExit("ERROR: you must provide --f-bed or --f-sites.")
    print('Running user-defined element driver detection')
    _scale_mode(args)
    if args.f_sites:
        res = transfer_tools.run_sites_region_model(
            args.fmut, args.f_sites, args.model, args.pretrain_key, scale_factor=args.scale_factor_manual,
            scale_type=args.scale_type, scale_by_expectation=args.scale_by_expectation)
    else:
        res = transfer_tools.run_element_region_model(
            args.fmut, args.f_bed, args.model, args.pretrain_key, scale_type=args.scale_type,
            scale_factor=args.scale_factor_manual, scale_factor_indel=args.scale_factor_indel_manual,
            max_muts_per_sample=args.max_muts_per_sample, max_muts_per_elt_per_sample=args.max_muts_per_elt_per_sample,
            scale_by_expectation=args.scale_by_expectation, skip_pvals=args.skip_pvals, fused=True)
    for col in ('OBS_SAMPLES', 'OBS_SNV', 'OBS_INDEL'):       # integer columns in the TSV (DigDriver.py:108-112)
        if col in res.columns:
            res[col] = res[col].astype(int)
    write_results(res, args)


def cmd_quick(args):
    _use_panel_dir(args)
    if not (args.f_elts_bed or args.region_str):
        raise SystemExit("ERROR: you must provide --f_elts_bed or --region_str.")
    from digdriver_amd.driver_model import onthefly_tools
    print('Running user-defined element driver detection')
    _scale_mode(args)
    res = onthefly_tools.DIG_onthefly(
        args.model, args.fmut, args.f_fasta, f_elts_bed=args.f_elts_bed, region_str=args.region_str,
        scale_factor=args.scale_factor_manual, scale_factor_indel=args.scale_factor_indel_manual,
        scale_type=args.scale_type, max_muts_per_sample=args.max_muts_per_sample,
        max_muts_per_elt_per_sample=args.max_muts_per_elt_per_sample, scale_by_expectation=args.scale_by_expectation,
        skip_pvals=args.skip_pvals)
    for col in ('OBS_SAMPLES', 'OBS_SNV', 'OBS_INDEL'):
        if col in res.columns:
            res[col] = res[col].astype(int)
    write_results(res, args)


def cmd_quick_cohorts(args):
    """quickCohorts: quickDriver for many cohorts on one bin grid in one pass; per cohort <outdir>/<outpfx>.results.txt."""
    _use_panel_dir(args)
    n = _cohort_lists(args, manual=False)
    if not (args.f_elts_bed or args.region_str):
        raise SystemExit("ERROR: you must provide --f_elts_bed or --region_str.")
    _scale_mode(args)
    factors = None
    if args.scale_factor_manual:
        if not len(args.scale_factor_manual) == len(args.scale_factor_indel_manual) == n:
            raise SystemExit("ERROR: --scale-factor-manual and --scale-factor-indel-manual take one value per cohort.")
        factors = (args.scale_factor_manual, args.scale_factor_indel_manual)
    from digdriver_amd.driver_model import cohort_batch
    print('Running user-defined element driver detection for {} cohorts'.format(n))
    _, paths = cohort_batch.run_and_write_quick_cohorts(
        args.mutation_files, args.maps, args.f_fasta, args.outdir, args.outpfx, f_elts_bed=args.f_elts_bed,
        region_str=args.region_str, scale_factors=factors, scale_type=args.scale_type, scale_by_expectation=args.scale_by_expectation,
        max_muts_per_sample=args.max_muts_per_sample, max_muts_per_elt_per_sample=args.max_muts_per_elt_per_sample,
        skip_pvals=args.skip_pvals)
    for path in paths:
        print('\tSaved results to {}'.format(path))


def cmd_element_cohorts(args):
    """elementCohorts: elementDriver for many cohorts on one bin grid in one pass.  Without a cut, per cohort
    <outdir>/<outpfx>.results.txt (--qvalues: with the QVAL_* columns behind the others); with --fdr or --pval-max (on --cut-on,
    default PVAL_SNV_BURDEN) only the elements that pass, as <outdir>/<outpfx>.hits.txt, QVAL_* columns included.  With --groups FILE
    also per group of cohorts <outdir>/<group>.meta.results.txt, or under the cut <outdir>/<group>.meta.hits.txt: the members'
    p-values combined per element by Fisher's method (cohort_batch.run_element_meta / run_element_meta_calls).  With --power also,
    behind the same pass, per cohort <outdir>/<outpfx>.power.txt and <outdir>/elements.power.txt: the critical count of --cut-on at the
    level of the run's own cut (--pval-max, --fdr, or --bonferroni, which cuts nothing itself) and the power at it under --power-folds
    (cohort_batch.run_element_power).  With --pairs (and --fdr or --pval-max: the pairs are pairs of calls) also per cohort
    <outdir>/<outpfx>.pairs.txt: for every pair of called elements the samples hit in both and the one-sided Fisher exact tests of
    co-occurrence and exclusivity, the pairs that pass --pairs-fdr (default 0.1) or --pairs-pval-max (cohort_batch.run_element_pairs)."""
    n = _cohort_lists(args, manual=False)
    factors = None
    if args.scale_factor_manual or args.scale_factor_indel_manual:
        if not (args.scale_factor_manual and args.scale_factor_indel_manual):
            raise SystemExit("ERROR: must specify both --scale-factor-manual and --scale-factor-indel-manual.")
        if not len(args.scale_factor_manual) == len(args.scale_factor_indel_manual) == n:
            raise SystemExit("ERROR: --scale-factor-manual and --scale-factor-indel-manual take one value per cohort.")
        factors = (args.scale_factor_manual, args.scale_factor_indel_manual)
    if args.fdr is not None and args.pval_max is not None:
        raise SystemExit("ERROR: you must provide at most one of --pval-max and --fdr.")
    cut = args.fdr if args.fdr is not None else args.pval_max
    if cut is None and args.cut_on is not None and not args.power:
        raise SystemExit("ERROR: --cut-on needs --fdr or --pval-max.")
    if cut is not None and not 0.0 < cut <= 1.0:
        raise SystemExit("ERROR: --fdr and --pval-max take a level within (0, 1].")
    power_kw = _power_options(args)
    pairs_kw = _pairs_options(args, n)
    groups = _read_groups(args.groups, args.outpfx) if args.groups else None
    from digdriver_amd.driver_model import cohort_batch
    print('Running user-defined element driver detection for {} cohorts'.format(n))
    common = dict(scale_factors=factors, max_muts_per_sample=args.max_muts_per_sample,
                  max_muts_per_elt_per_sample=args.max_muts_per_elt_per_sample)
    if groups is not None or power_kw is not None or pairs_kw is not None:      # every route's files behind ONE pass over the inputs
        keep = dict(keep_sample_keys=True) if pairs_kw is not None else {}
        common['element_pass'] = cohort_batch.element_pass(args.mutation_files, args.maps, args.f_element_data, args.save_key, **common,
                                                           **keep)

    def meta(**cut_kw):
        # (the groups' files beside the cohorts': <group>.meta.results.txt, or <group>.meta.hits.txt under the same cut)
        if groups is None:
            return
        frames, paths = cohort_batch.run_and_write_element_meta(args.mutation_files, args.maps, args.f_element_data, args.save_key,
                                                                groups, args.outdir, labels=args.outpfx, **cut_kw, **common)
        for frame, path in zip(frames, paths):
            if cut_kw:
                print('\t{}: {} hits of {} testable elements; saved to {}'.format(frame.attrs['group'], len(frame),
                                                                                 frame.attrs['n_testable'], path))
            else:
                print('\tSaved results to {}'.format(path))

    def power():
        if power_kw is None:
            return
        frames, summary, paths = _without_indel_columns_exit(cohort_batch.run_and_write_element_power, args.mutation_files, args.maps,
                                                             args.f_element_data, args.save_key, args.outdir, args.outpfx, **power_kw,
                                                             **common)
        for pfx, frame, path in zip(args.outpfx, frames, paths):
            print('\t{}: level {:g}, {} of {} testable elements powered at fold {:g}; saved to {}'.format(
                pfx, frame.attrs['level'], int(frame['POWERED'].sum()), frame.attrs['n_testable'], max(power_kw['folds']), path))
        print('\tSaved the per-element summary to {}'.format(paths[-1]))

    def pairs():
        if pairs_kw is None:
            return
        try:
            frames, paths = _without_indel_columns_exit(cohort_batch.run_and_write_element_pairs, args.mutation_files, args.maps,
                                                        args.f_element_data, args.save_key, args.outdir, args.outpfx, **cut_kw,
                                                        **pairs_kw, **common)
        except ValueError as exc:                        # (too many called elements for the pair matrix, --pairs-n-samples too small)
            if 'entering elements' not in str(exc) and 'n_samples' not in str(exc):
                raise
            raise SystemExit("ERROR: --pairs: {}".format(exc))
        for pfx, frame, path in zip(args.outpfx, frames, paths):
            print('\t{}: {} pairs reported of {} testable among {} elements; saved to {}'.format(
                pfx, len(frame), frame.attrs['n_testable'], frame.attrs['n_elements'], path))

    if cut is None:
        _, paths = cohort_batch.run_and_write_element_cohorts(args.mutation_files, args.maps, args.f_element_data, args.save_key,
                                                              args.outdir, args.outpfx, qvalues=args.qvalues, **common)
        for path in paths:
            print('\tSaved results to {}'.format(path))
        meta()
        power()
        return
    cut_kw = dict(pval_max=args.pval_max, fdr=args.fdr, cut_on=args.cut_on or 'PVAL_SNV_BURDEN')
    frames, paths = _without_indel_columns_exit(cohort_batch.run_and_write_element_calls, args.mutation_files, args.maps,
                                                args.f_element_data, args.save_key, args.outdir, args.outpfx, **cut_kw, **common)
    for pfx, frame, path in zip(args.outpfx, frames, paths):
        print('\t{}: {} hits of {} testable elements; saved to {}'.format(pfx, len(frame), frame.attrs['n_testable'], path))
    _without_indel_columns_exit(meta, **cut_kw)
    power()
    pairs()


def _power_options(args):
    """--power of elementCohorts and what goes with it, checked before a file is read: None without --power, else the keywords of
    cohort_batch.run_element_power (the level of the run's own cut, --cut-on, the folds, --power-min)."""
    if not args.power:
        if args.bonferroni is not None or args.power_folds is not None or args.power_min is not None:
            raise SystemExit("ERROR: --bonferroni, --power-folds and --power-min need --power.")
        return None
    if sum(v is not None for v in (args.pval_max, args.fdr, args.bonferroni)) != 1:
        raise SystemExit("ERROR: --power needs exactly one of --pval-max, --fdr and --bonferroni: the level of the critical counts.")
    if args.bonferroni is not None and not 0.0 < args.bonferroni <= 1.0:
        raise SystemExit("ERROR: --bonferroni takes a level within (0, 1].")
    if args.cut_on == 'PVAL_MUT_BURDEN':
        raise SystemExit("ERROR: --power has no critical count for --cut-on PVAL_MUT_BURDEN (Fisher's method over two tests).")
    folds = args.power_folds if args.power_folds is not None else [2.0, 5.0, 10.0]
    if not 1 <= len(folds) <= 8 or not all(0.0 < f < float('inf') for f in folds) or len(set('%g' % f for f in folds)) != len(folds):
        raise SystemExit("ERROR: --power-folds takes one to eight different folds, each finite and > 0.")
    power_min = 0.8 if args.power_min is None else args.power_min
    if not 0.0 < power_min <= 1.0:
        raise SystemExit("ERROR: --power-min takes a power within (0, 1].")
    return dict(pval_max=args.pval_max, fdr=args.fdr, bonferroni=args.bonferroni, cut_on=args.cut_on or 'PVAL_SNV_BURDEN',
                folds=tuple(folds), power_min=power_min)


def _pairs_options(args, n):
    """--pairs of elementCohorts and what goes with it, checked before a file is read: None without --pairs, else the keywords of
    cohort_batch.run_element_pairs that are its own (the level of the pairs, --pairs-min-samples, --pairs-n-samples)."""
    own = (args.pairs_fdr, args.pairs_pval_max, args.pairs_min_samples, args.pairs_n_samples)
    if not args.pairs:
        if any(v is not None for v in own):
            raise SystemExit("ERROR: --pairs-fdr, --pairs-pval-max, --pairs-min-samples and --pairs-n-samples need --pairs.")
        return None
    if (args.fdr is None) == (args.pval_max is None):
        raise SystemExit("ERROR: --pairs needs exactly one of --fdr and --pval-max: the pairs are pairs of called elements.")
    if args.pairs_fdr is not None and args.pairs_pval_max is not None:
        raise SystemExit("ERROR: you must provide at most one of --pairs-fdr and --pairs-pval-max.")
    level = args.pairs_pval_max if args.pairs_pval_max is not None else 0.1 if args.pairs_fdr is None else args.pairs_fdr
    if not 0.0 < level <= 1.0:
        raise SystemExit("ERROR: --pairs-fdr and --pairs-pval-max take a level within (0, 1].")
    min_samples = 1 if args.pairs_min_samples is None else args.pairs_min_samples
    if min_samples < 1:
        raise SystemExit("ERROR: --pairs-min-samples takes a count of at least 1.")
    if args.pairs_n_samples is not None and (len(args.pairs_n_samples) != n or min(args.pairs_n_samples) < 1):
        raise SystemExit("ERROR: --pairs-n-samples takes one sample count >= 1 per cohort.")
    return dict(pair_pval_max=args.pairs_pval_max, pair_fdr=None if args.pairs_pval_max is not None else level, min_samples=min_samples,
                n_samples=args.pairs_n_samples)


def _without_indel_columns_exit(run, *args, **kw):
    """run(*args, **kw); a cut on an indel column that a cohort or a group lacks ends the command with the route's own words."""
    try:
        return run(*args, **kw)
    except ValueError as exc:
        if 'no indel columns' not in str(exc):
            raise
        raise SystemExit("ERROR: {}".format(exc))


def _read_groups(path, prefixes):
    """--groups FILE of elementCohorts: two tab-separated columns, group name and cohort prefix (one of --outpfx; a cohort may be in
    many groups) -> an ordered dict group name -> prefixes.  An empty file, an unknown prefix, a repeated pair and a group name that
    repeats a cohort prefix (its files would be confused with the cohort's) end the command before a cohort's file is read."""
    if len(set(prefixes)) != len(prefixes):
        raise SystemExit("ERROR: --groups names cohorts by their --outpfx, which must then differ from each other.")
    groups = {}
    with open(path) as fh:
        for n, line in enumerate(fh, 1):
            line = line.rstrip('\r\n')
            if not line.strip() or line.startswith('#'):
                continue
            cols = line.split('\t')
            if len(cols) != 2 or not cols[0].strip() or not cols[1].strip():
                raise SystemExit("ERROR: --groups {}, line {}: two tab-separated columns, group name and cohort prefix.".format(path, n))
            name, pfx = cols[0].strip(), cols[1].strip()
            if pfx not in prefixes:
                raise SystemExit("ERROR: --groups {}, line {}: {} is not one of --outpfx.".format(path, n, pfx))
            if name in prefixes:
                raise SystemExit("ERROR: --groups {}, line {}: the group name {} repeats a cohort prefix.".format(path, n, name))
            if pfx in groups.setdefault(name, []):
                raise SystemExit("ERROR: --groups {}, line {}: {} is in group {} already.".format(path, n, pfx, name))
            groups[name].append(pfx)
    if not groups:
        raise SystemExit("ERROR: --groups {} names no group.".format(path))
    return groups


def _cohort_lists(args, manual=True):
    """The number of cohorts, the lists checked: one map and one prefix per mutation file and (manual) one --scale-factor-manual."""
    n = len(args.mutation_files)
    if not len(args.maps) == len(args.outpfx) == n:
        raise SystemExit("ERROR: --mutation-files, --maps and --outpfx must name the same number of cohorts.")
    if manual and args.scale_factor_manual and len(args.scale_factor_manual) != n:
        raise SystemExit("ERROR: --scale-factor-manual takes one value per cohort.")
    return n


def cmd_target_cohorts(args):
    """targetCohorts: targetDriver for many cohorts in one pass; per cohort <outdir>/<outpfx>.results.txt."""
    _use_panel_dir(args)
    n = _cohort_lists(args)
    from digdriver_amd.driver_model import cohort_batch
    print('Running MSK-IMPACT driver detection for {} cohorts'.format(n))
    _, paths = cohort_batch.run_and_write_target_cohorts(
        args.mutation_files, args.maps, args.outdir, args.outpfx, scale_by_sample=args.scale_by_samples, panel=args.panel,
        max_muts_per_sample=args.max_muts_per_sample, max_muts_per_gene_per_sample=args.max_muts_per_gene_per_sample,
        cgc_genes=args.cgc_genes, scale_factors=args.scale_factor_manual, drop_synonymous=False)
    for path in paths:
        print('\tSaved results to {}'.format(path))


def cmd_gene_cohorts(args):
    """geneCohorts: geneDriver for many cohorts in one pass; per cohort <outdir>/<outpfx>.results.txt.  Scale rules: the expected
    synonymous count (the default) or manual factors, as cohort_batch.run_gene_cohorts takes them."""
    _use_panel_dir(args)
    n = _cohort_lists(args)
    if args.scale_by_samples or not (args.scale_by_expectation or args.scale_factor_manual):
        raise SystemExit("ERROR: geneCohorts scales by expected synonymous mutations or by --scale-factor-manual; the sample and "
                         "mutation-count ratios are geneDriver's.")
    from digdriver_amd.driver_model import cohort_batch
    print('Running gene driver detection for {} cohorts'.format(n))
    _, paths = cohort_batch.run_and_write_gene_cohorts(
        args.mutation_files, args.maps, args.outdir, args.outpfx, pval_burden_nb=args.pval_burden,
        max_muts_per_sample=args.max_muts_per_sample, max_muts_per_gene_per_sample=args.max_muts_per_gene_per_sample,
        scale_factors=args.scale_factor_manual, scale_by_expectation=args.scale_by_expectation, cgc_genes=args.cgc_genes,
        selection=args.selection, pval_burden_dnds=args.pval_burden_dnds, pval_sel=args.pval_sel)
    for path in paths:
        print('\tSaved results to {}'.format(path))


TILE_MODELS = {(1, 1): 'sequence_model_64', (2, 2): 'sequence_model_1024'}


def cmd_tile(args):
    """tileDriver: the per-base scan of many cohorts on one bin grid; per cohort the tiles that pass the cut, as
    <outdir>/<outpfx>.hits.txt (the rows of nb_model's frame, numbered as in it; with --fdr a QVAL column as well).  --sparse tests
    the mutated tiles only (nb_model_hits_sparse; --bonferroni is its third cut, the sample options are not part of it).  The sample
    options (--max-muts-per-sample, --max-muts-per-tile-per-sample, --by-sample, --cut-on) read the sample label from column 6 of
    the mutation files; --by-sample adds OBS_SAMPLES and PVAL_SAMPLE behind REGION.  --window-tiles M [M ...] tests every window of M
    consecutive tiles instead (nb_model_window_hits: WIDTH and PEAK behind REGION; not with --sparse, --by-sample, --cut-on PVAL_SAMPLE).
    --window-samples (with --window-tiles) counts the distinct samples of every window: OBS_SAMPLES and PVAL_SAMPLE behind REGION, and
    --cut-on PVAL_SAMPLE selects on them.  --sparse --sparse-windows M [M ...] tests the windows of M consecutive tiles that hold a
    mutation row, and no other (nb_model_window_hits_sparse: the frames of --window-tiles, the three cuts of --sparse, a zero-window
    floor per cohort and width; not with --window-tiles, --window-samples or the sample options)."""
    n = _cohort_lists(args, manual=False)
    if args.sparse_windows is not None:
        if not args.sparse:
            raise SystemExit("ERROR: --sparse-windows needs --sparse (every window of the dense planes: --window-tiles).")
        if args.window_tiles is not None:
            raise SystemExit("ERROR: --sparse-windows does not go with --window-tiles (the windows of the sparse scan or those of the dense planes).")
        if args.window_samples:
            raise SystemExit("ERROR: --sparse-windows does not take --window-samples (the sparse scan counts rows, not samples).")
        if args.max_muts_per_sample is not None or args.max_muts_per_tile_per_sample is not None or args.by_sample or args.cut_on != 'PVAL':
            raise SystemExit("ERROR: --sparse-windows does not take the sample options (--max-muts-per-sample, --max-muts-per-tile-per-sample, "
                             "--by-sample, --cut-on).")
        if min(args.sparse_windows) < 1 or len(set(args.sparse_windows)) != len(args.sparse_windows):
            raise SystemExit("ERROR: --sparse-windows takes distinct integers >= 1.")
    if args.window_samples and args.window_tiles is None:
        raise SystemExit("ERROR: --window-samples needs --window-tiles (the tiles' own samples: --by-sample).")
    if args.window_tiles is not None:
        if args.sparse:
            raise SystemExit("ERROR: --window-tiles is not part of --sparse (the sparse scan tests single tiles); "
                             "--sparse --sparse-windows M tests the windows that hold a mutation row.")
        if args.by_sample:
            raise SystemExit("ERROR: --window-tiles does not take --by-sample (the samples of a window are not the sum of its tiles' samples); "
                             "--window-samples counts a window's distinct samples.")
        if args.cut_on != 'PVAL' and not args.window_samples:
            raise SystemExit("ERROR: --window-tiles selects on PVAL only (--cut-on PVAL_SAMPLE needs --by-sample, which it does not take); "
                             "with --window-samples it selects on the windows' PVAL_SAMPLE.")
        if min(args.window_tiles) < 1 or len(set(args.window_tiles)) != len(args.window_tiles):
            raise SystemExit("ERROR: --window-tiles takes distinct integers >= 1.")
    if args.bonferroni is not None and not args.sparse:
        raise SystemExit("ERROR: --bonferroni is valid only with --sparse.")
    if args.sparse:
        if sum(x is not None for x in (args.pval_max, args.fdr, args.bonferroni)) != 1:
            raise SystemExit("ERROR: you must provide exactly one of --pval-max, --fdr and --bonferroni.")
        if args.bonferroni is not None and not 0.0 < args.bonferroni <= 1.0:
            raise SystemExit("ERROR: --bonferroni takes a level within (0, 1].")
        if args.max_muts_per_sample is not None or args.max_muts_per_tile_per_sample is not None or args.by_sample or args.cut_on != 'PVAL':
            raise SystemExit("ERROR: --sparse does not take the sample options (--max-muts-per-sample, --max-muts-per-tile-per-sample, "
                             "--by-sample, --cut-on).")
    elif (args.pval_max is None) == (args.fdr is None):
        raise SystemExit("ERROR: you must provide exactly one of --pval-max and --fdr.")
    if args.cut_on == 'PVAL_SAMPLE' and not (args.by_sample or args.window_samples):
        raise SystemExit("ERROR: --cut-on PVAL_SAMPLE requires --by-sample.")
    if args.max_muts_per_tile_per_sample is not None and args.max_muts_per_tile_per_sample < 1:
        raise SystemExit("ERROR: --max-muts-per-tile-per-sample takes an integer >= 1.")
    if args.max_muts_per_sample is not None and args.max_muts_per_sample < 0:
        raise SystemExit("ERROR: --max-muts-per-sample takes an integer >= 0.")
    key = TILE_MODELS.get((args.up, args.down))
    if key is None:
        raise NotImplementedError("the tile kernels take n_up = n_down = 1 or 2")
    import numpy as np
    from digdriver_amd.sequence_model import nb_model
    print('Running per-base tile driver detection for {} cohorts'.format(n))
    cols = ['CHROM', 'START', 'END', 'Y_PRED', 'STD']
    idx, mu, sigma, d_prs = None, [], [], []
    for f_map in args.maps:
        reg = mapfile.read_columns(f_map, 'region_params', cols)
        grid = np.stack([np.asarray(reg[k]).astype(np.int64) for k in cols[:3]], axis=1)
        if idx is None:
            idx = grid
        elif not np.array_equal(grid, idx):
            raise ValueError("{}: the rows of region_params (CHROM, START, END) differ from those of {}".format(f_map, args.maps[0]))
        mu.append(np.asarray(reg['Y_PRED'], float))
        sigma.append(np.asarray(reg['STD'], float))
        try:
            seq = mapfile.read_frame(f_map, key)
        except KeyError:
            raise SystemExit("ERROR: {} has no frame {} (--up {} --down {} needs it).".format(f_map, key, args.up, args.down))
        d_prs.append(seq.set_index('CONTEXT').FREQ if 'CONTEXT' in seq.columns else seq.FREQ)
    keep = np.ones(len(idx), bool) if not args.chroms else np.isin(idx[:, 0].astype(str), [c.replace('chr', '') for c in args.chroms])
    if not keep.any():
        raise SystemExit("ERROR: no region of region_params is left to scan.")
    # (the sample options are passed only when one is set: without them the call is the one of before)
    sample_opts = {} if (args.max_muts_per_sample is None and args.max_muts_per_tile_per_sample is None and not args.by_sample
                         and not args.window_samples) else dict(
        max_muts_per_sample=args.max_muts_per_sample, max_muts_per_tile_per_sample=args.max_muts_per_tile_per_sample,
        by_sample=args.by_sample, cut_on=args.cut_on)
    if args.window_samples:
        sample_opts['window_samples'] = True
    if args.sparse and args.sparse_windows is not None:
        try:
            frames = nb_model.nb_model_window_hits_sparse(d_prs, idx[keep], np.array(mu)[:, keep], np.array(sigma)[:, keep], args.mutation_files,
                                                          args.f_fasta, n_up=args.up, n_down=args.down, binsize=args.binsize,
                                                          widths=args.sparse_windows, pval_max=args.pval_max, fdr=args.fdr,
                                                          bonferroni=args.bonferroni)
        except ValueError as exc:
            if 'no certificate' not in str(exc):
                raise
            raise SystemExit("ERROR: {}".format(exc))
        os.makedirs(args.outdir, exist_ok=True)
        for pfx, frame in zip(args.outpfx, frames):
            target = os.path.join(args.outdir, pfx + '.hits.txt')
            floors = ', '.join('{:.3g}{}'.format(f, '' if done else ' (mutated windows only)')
                               for f, done in zip(frame.attrs['zero_floor'], frame.attrs['complete']))
            print('\t{}: {} hits of {} testable windows (widths {}), zero-window floors {}; saving to {}'.format(
                pfx, len(frame), frame.attrs['n_testable'], args.sparse_windows, floors, target))
            mapfile.write_results_tsv(frame, target)
        return
    if args.sparse:
        try:
            frames = nb_model.nb_model_hits_sparse(d_prs, idx[keep], np.array(mu)[:, keep], np.array(sigma)[:, keep], args.mutation_files,
                                                   args.f_fasta, n_up=args.up, n_down=args.down, binsize=args.binsize,
                                                   pval_max=args.pval_max, fdr=args.fdr, bonferroni=args.bonferroni)
        except ValueError as exc:
            if 'no certificate' not in str(exc):
                raise
            raise SystemExit("ERROR: {}".format(exc))
        os.makedirs(args.outdir, exist_ok=True)
        for pfx, frame in zip(args.outpfx, frames):
            target = os.path.join(args.outdir, pfx + '.hits.txt')
            print('\t{}: {} hits of {} testable tiles, zero-tile floor {:.3g}{}; saving to {}'.format(
                pfx, len(frame), frame.attrs['n_testable'], frame.attrs['zero_floor'],
                '' if frame.attrs['complete'] else ' (mutated tiles only)', target))
            mapfile.write_results_tsv(frame, target)
        return
    # (--window-tiles alone picks the other function: without it the call is the one of before)
    scan = nb_model.nb_model_hits if args.window_tiles is None else functools.partial(nb_model.nb_model_window_hits, widths=args.window_tiles)
    try:
        frames = scan(d_prs, idx[keep], np.array(mu)[:, keep], np.array(sigma)[:, keep], args.mutation_files,
                      args.f_fasta, n_up=args.up, n_down=args.down, binsize=args.binsize, pval_max=args.pval_max,
                      fdr=args.fdr, **sample_opts)
    except ValueError as exc:
        if not sample_opts or 'column 6' not in str(exc):
            raise
        raise SystemExit("ERROR: {}".format(exc))           # (a mutation file without sample labels)
    os.makedirs(args.outdir, exist_ok=True)
    for pfx, frame in zip(args.outpfx, frames):
        target = os.path.join(args.outdir, pfx + '.hits.txt')
        if args.window_tiles is None:
            print('\t{}: {} hits of {} testable tiles; saving to {}'.format(pfx, len(frame), frame.attrs['n_testable'], target))
        else:
            print('\t{}: {} hits of {} testable windows (widths {}); saving to {}'.format(
                pfx, len(frame), frame.attrs['n_testable'], args.window_tiles, target))
        mapfile.write_results_tsv(frame, target)


def _common(p, element_caps):
    p.add_argument('fmut', type=str, help='annotated mutation file (DigPreprocess.py annotMutationFile format)')
    p.add_argument('model', type=str, help='pretrained mutation map')
    # not a reference option: the reference finds its gene panels (genes_CGC_ALL.txt, genes_MSK_341.txt, ...) inside its
    # installed package; here they are looked up in this directory, then $DIG_DATA_DIR, digdriver_amd/data/ and an
    # installed DIGDriver package
    p.add_argument('--panel-dir', type=str, default=None, help='directory holding the gene panel files genes_<NAME>.txt')
    return p


def _output(p):
    p.add_argument('--outpfx', type=str, required=True, help='prefix of the results file')
    p.add_argument('--outdir', type=str, required=True, help='directory for the results file')


def parse_args(text=None):
    parser = argparse.ArgumentParser(description='Burden tests for cancer driver elements (MI355X build).')
    sub = parser.add_subparsers()

    g = _common(sub.add_parser('geneDriver', help='test every gene of a cohort'), False)
    _output(g)
    g.add_argument('--max-muts-per-sample', type=int, default=3e9, help='drop samples with more mutations than this')
    g.add_argument('--max-muts-per-gene-per-sample', type=int, default=3e9, help='cap of mutations one sample adds to a gene')
    g.add_argument('--scale-by-mutations', action='store_false', default=True, dest="scale_by_expectation",
                   help='scale by mutation counts instead of expected synonymous mutations')
    g.add_argument('--scale-by-samples', action='store_true', default=False, help='scale by the number of samples')
    g.add_argument('--scale-factor-manual', default=None, type=float, help='use this scale factor')
    g.add_argument('--cgc-genes', choices=CGC_SETS, default=False, help='restrict to a Cancer Gene Census set')
    g.add_argument('--no-pval-burden', dest='pval_burden', action='store_false', default=True,
                   help='skip the burden p-values')
    g.add_argument('--selection', action='store_true', default=False,
                   help='add the dN/dS-corrected expectations, their burden p-values and the selection p-values')
    g.add_argument('--no-pval-burden-dnds', dest='pval_burden_dnds', action='store_false', default=True,
                   help='with --selection: skip the dN/dS-corrected burden p-values')
    g.add_argument('--no-pval-sel', dest='pval_sel', action='store_false', default=True,
                   help='with --selection: skip the selection p-values')
    g.set_defaults(func=cmd_gene)

    t = _common(sub.add_parser('targetDriver', help='test the genes of a targeted sequencing panel'), False)
    _output(t)
    t.add_argument('--panel', type=str, choices=PANELS, help='gene panel')
    t.add_argument('--max-muts-per-sample', type=int, default=3e9, help='drop samples with more mutations than this')
    t.add_argument('--max-muts-per-gene-per-sample', type=int, default=3e9, help='cap of mutations one sample adds to a gene')
    t.add_argument('--scale-by-samples', action='store_true', default=False, help='scale by the number of samples')
    t.add_argument('--scale-factor-manual', default=None, type=float, help='use this scale factor')
    t.add_argument('--cgc-genes', choices=CGC_SETS, default=False, help='restrict to a Cancer Gene Census set')
    t.set_defaults(func=cmd_target)

    for name, func, extra in (('elementDriver', cmd_element, 'element'), ('quickDriver', cmd_quick, 'quick')):
        e = _common(sub.add_parser(name, help='test user-defined elements' if extra == 'element'
                                   else 'test ad-hoc elements or a region string (no pretrained element model)'), True)
        if extra == 'element':
            e.add_argument('pretrain_key', type=str, help='key of the pretrained element model inside the map')
            e.add_argument('--f-bed', type=str, default="", help='bed12 file the element model was pretrained on')
            e.add_argument('--f-sites', type=str, default="", help='sites file the element model was pretrained on (SNVs only)')
        else:
            e.add_argument('f_fasta', type=str, help='reference genome FASTA (hg19)')
            e.add_argument('--f_elts_bed', type=str, default="", help='bed12 file of elements')
            e.add_argument('--region_str', type=str, default="", help='region as chr{}:start-end')
        _output(e)
        e.add_argument('--max-muts-per-sample', type=int, default=3e9, help='drop samples with more mutations in elements than this')
        e.add_argument('--max-muts-per-elt-per-sample', type=int, default=3e9, help='cap of mutations one sample adds to an element')
        e.add_argument('--scale-type', default=None, choices=SCALE_TYPES, help='how to derive the cohort scale factor')
        e.add_argument('--scale-factor-manual', default=None, type=float, help='use this SNV scale factor')
        e.add_argument('--skip_pvals', default=False, action='store_true', help='expected counts only')
        e.add_argument('--scale-factor-indel-manual', default=None, type=float, help='use this indel scale factor')
        e.set_defaults(func=func)

    # not a reference sub-command: the reference's per-base route (nb_model.py:188-234) has no command line
    d = sub.add_parser('tileDriver', help='per-base scan of many cohorts on one bin grid: the tiles that pass a cut')
    d.add_argument('f_fasta', type=str, help='reference genome FASTA')
    d.add_argument('--mutation-files', type=str, nargs='+', required=True, help='one bed-like mutation file per cohort')
    d.add_argument('--maps', type=str, nargs='+', required=True, help='one pretrained mutation map per cohort, all on one bin grid')
    d.add_argument('--outdir', type=str, required=True, help='directory for the hit files')
    d.add_argument('--outpfx', type=str, nargs='+', required=True, help='one prefix per cohort: <outpfx>.hits.txt')
    d.add_argument('--binsize', type=int, default=50, help='positions per tile')
    d.add_argument('--up', type=int, default=1, help='context bases in front of a position (1 or 2)')
    d.add_argument('--down', type=int, default=1, help='context bases behind a position (equal to --up)')
    d.add_argument('--pval-max', type=float, default=None, help='keep the tiles with PVAL <= this')
    d.add_argument('--fdr', type=float, default=None, help="keep the tiles with Benjamini-Hochberg q <= this over the cohort's testable tiles")
    d.add_argument('--chroms', type=str, nargs='+', default=None, help='scan only the regions of these chromosomes')
    # the scan over the mutated tiles only: memory follows the rows, not the genome (DESIGN.md "Sparse per-base scan")
    d.add_argument('--sparse', action='store_true', default=False,
                   help='test only the tiles that hold a mutation row; an empty tile is ruled out by a bound on its p-value')
    d.add_argument('--bonferroni', type=float, default=None,
                   help="with --sparse: keep the tiles with PVAL <= this / the cohort's testable tiles")
    # the sample guards of the other routes, for tiles; any of them makes column 6 of the mutation files the sample label
    d.add_argument('--max-muts-per-sample', type=int, default=None, help='drop samples with more rows in their file than this')
    d.add_argument('--max-muts-per-tile-per-sample', type=int, default=None, help='cap of rows one sample adds to a tile (>= 1)')
    d.add_argument('--by-sample', action='store_true', default=False,
                   help='add OBS_SAMPLES (samples with a row in the tile) and PVAL_SAMPLE (the test on it)')
    d.add_argument('--cut-on', choices=['PVAL', 'PVAL_SAMPLE'], default='PVAL',
                   help='the score --pval-max / --fdr select on (PVAL_SAMPLE requires --by-sample)')
    # every run of M consecutive tiles instead of the tiles of one grid (DESIGN.md "Sliding windows in the per-base route")
    d.add_argument('--window-tiles', type=int, nargs='+', default=None, metavar='M',
                   help='test every window of M consecutive tiles, for each M given (adds WIDTH and PEAK; not with --sparse, --by-sample)')
    d.add_argument('--window-samples', action='store_true', default=False,
                   help="with --window-tiles: count every window's distinct samples (adds OBS_SAMPLES and PVAL_SAMPLE; --cut-on PVAL_SAMPLE "
                        "then selects on them)")
    # the windows of --window-tiles that hold a mutation row, without the dense planes (DESIGN.md "Sparse sliding windows")
    d.add_argument('--sparse-windows', type=int, nargs='+', default=None, metavar='M',
                   help='with --sparse: test the windows of M consecutive tiles that hold a mutation row, for each M given (adds WIDTH and '
                        'PEAK; not with --window-tiles, --window-samples or the sample options)')
    d.set_defaults(func=cmd_tile)

    # not a reference sub-command: quickDriver for many cohorts at once (driver_model/cohort_batch.py run_quick_cohorts)
    q = sub.add_parser('quickCohorts', help='quickDriver for many cohorts on one bin grid: ad-hoc elements or a region string')
    q.add_argument('f_fasta', type=str, help='reference genome FASTA (hg19)')
    q.add_argument('--mutation-files', type=str, nargs='+', required=True, help='one annotated mutation file per cohort')
    q.add_argument('--maps', type=str, nargs='+', required=True, help='one pretrained mutation map per cohort, all on one bin grid')
    q.add_argument('--outdir', type=str, required=True, help='directory for the results files')
    q.add_argument('--outpfx', type=str, nargs='+', required=True, help='one prefix per cohort: <outpfx>.results.txt')
    q.add_argument('--f_elts_bed', type=str, default="", help='bed12 file of elements')
    q.add_argument('--region_str', type=str, default="", help='region as chr{}:start-end')
    q.add_argument('--max-muts-per-sample', type=int, default=3e9, help='drop samples with more mutations in elements than this')
    q.add_argument('--max-muts-per-elt-per-sample', type=int, default=3e9, help='cap of mutations one sample adds to an element')
    q.add_argument('--scale-type', default=None, choices=SCALE_TYPES, help='how to derive the cohort scale factors')
    q.add_argument('--scale-factor-manual', default=None, type=float, nargs='+', help='use these SNV scale factors, one per cohort')
    q.add_argument('--scale-factor-indel-manual', default=None, type=float, nargs='+', help='use these indel scale factors, one per cohort')
    q.add_argument('--skip_pvals', default=False, action='store_true', help='expected counts only')
    q.add_argument('--panel-dir', type=str, default=None, help='directory holding the gene panel files genes_<NAME>.txt')
    q.set_defaults(func=cmd_quick_cohorts)

    # not a reference sub-command: elementDriver for many cohorts at once, with q-values and calls (driver_model/cohort_batch.py
    # run_element_cohorts / run_element_calls)
    ec = sub.add_parser('elementCohorts', help='elementDriver for many cohorts on one bin grid: results, or only the elements that pass a cut')
    ec.add_argument('f_element_data', type=str, help='element data container (DigPreprocess.py)')
    ec.add_argument('save_key', type=str, help='key of the element set inside the container')
    ec.add_argument('--mutation-files', type=str, nargs='+', required=True, help='one annotated mutation file per cohort')
    ec.add_argument('--maps', type=str, nargs='+', required=True, help='one pretrained mutation map per cohort, all on one bin grid')
    ec.add_argument('--outdir', type=str, required=True, help='directory for the results or hit files')
    ec.add_argument('--outpfx', type=str, nargs='+', required=True, help='one prefix per cohort: <outpfx>.results.txt or <outpfx>.hits.txt')
    ec.add_argument('--max-muts-per-sample', type=int, default=3e9, help='drop samples with more mutations in elements than this')
    ec.add_argument('--max-muts-per-elt-per-sample', type=int, default=3e9, help='cap of mutations one sample adds to an element')
    ec.add_argument('--scale-factor-manual', default=None, type=float, nargs='+', help='use these SNV scale factors, one per cohort')
    ec.add_argument('--scale-factor-indel-manual', default=None, type=float, nargs='+', help='use these indel scale factors, one per cohort')
    ec.add_argument('--qvalues', action='store_true', default=False,
                    help="add a Benjamini-Hochberg QVAL_* column per PVAL_* column, over the cohort's testable elements")
    ec.add_argument('--fdr', type=float, default=None, help='write only the elements with q <= this, as <outpfx>.hits.txt')
    ec.add_argument('--pval-max', type=float, default=None, help='write only the elements with p <= this, as <outpfx>.hits.txt')
    ec.add_argument('--cut-on', default=None, choices=['PVAL_SNV_BURDEN', 'PVAL_SAMPLE_BURDEN', 'PVAL_INDEL_BURDEN', 'PVAL_MUT_BURDEN'],
                    help='the column --fdr / --pval-max select on (default PVAL_SNV_BURDEN)')
    ec.add_argument('--power', action='store_true', default=False,
                    help="also write <outpfx>.power.txt and elements.power.txt: per element the critical count of --cut-on at the level "
                         "of the run's cut and the power at it under a fold of selection")
    ec.add_argument('--bonferroni', type=float, default=None,
                    help="with --power: the level is this over the cohort's testable elements (cuts nothing itself)")
    ec.add_argument('--power-folds', type=float, nargs='+', default=None, help='with --power: the folds of selection (default 2 5 10; at most 8)')
    ec.add_argument('--power-min', type=float, default=None,
                    help='with --power: POWERED is the power at the largest fold >= this (default 0.8)')
    ec.add_argument('--pairs', action='store_true', default=False,
                    help='with --fdr or --pval-max, also write <outpfx>.pairs.txt: co-occurrence and exclusivity of the called elements '
                         "across the cohort's samples (one-sided Fisher exact tests per pair, Benjamini-Hochberg over the pairs)")
    ec.add_argument('--pairs-fdr', type=float, default=None, help='with --pairs: report the pairs with a q-value <= this (default 0.1)')
    ec.add_argument('--pairs-pval-max', type=float, default=None, help='with --pairs: report the pairs with a p-value <= this instead')
    ec.add_argument('--pairs-min-samples', type=int, default=None,
                    help='with --pairs: only the called elements hit in at least this many samples enter (default 1)')
    ec.add_argument('--pairs-n-samples', type=int, nargs='+', default=None,
                    help="with --pairs: the cohorts' sample counts, one per cohort (default: the samples of the mutation file; samples "
                         'without a mutation are not in it)')
    ec.add_argument('--groups', type=str, default=None,
                    help='file of two tab-separated columns, group name and cohort prefix (one of --outpfx): per group the cohorts\' '
                         'p-values combined by Fisher\'s method, as <group>.meta.results.txt (under a cut: <group>.meta.hits.txt)')
    ec.set_defaults(func=cmd_element_cohorts)

    def cohort_lists(p):
        p.add_argument('--mutation-files', type=str, nargs='+', required=True, help='one annotated mutation file per cohort')
        p.add_argument('--maps', type=str, nargs='+', required=True, help='one pretrained mutation map per cohort, all with one gene index')
        p.add_argument('--outdir', type=str, required=True, help='directory for the results files')
        p.add_argument('--outpfx', type=str, nargs='+', required=True, help='one prefix per cohort: <outpfx>.results.txt')
        p.add_argument('--max-muts-per-sample', type=int, default=3e9, help='drop samples with more mutations than this')
        p.add_argument('--max-muts-per-gene-per-sample', type=int, default=3e9, help='cap of mutations one sample adds to a gene')
        p.add_argument('--scale-by-samples', action='store_true', default=False, help='scale by the number of samples')
        p.add_argument('--scale-factor-manual', default=None, type=float, nargs='+', help='use these scale factors, one per cohort')
        p.add_argument('--cgc-genes', choices=CGC_SETS, default=False, help='restrict to a Cancer Gene Census set')
        p.add_argument('--panel-dir', type=str, default=None, help='directory holding the gene panel files genes_<NAME>.txt')

    # not a reference sub-command: targetDriver for many cohorts at once (driver_model/cohort_batch.py run_target_cohorts)
    tc = sub.add_parser('targetCohorts', help='targetDriver for many cohorts: the genes of a targeted sequencing panel')
    cohort_lists(tc)
    tc.add_argument('--panel', type=str, choices=PANELS, help='gene panel')
    tc.set_defaults(func=cmd_target_cohorts)

    # not a reference sub-command: geneDriver for many cohorts at once (driver_model/cohort_batch.py run_gene_cohorts)
    gc = sub.add_parser('geneCohorts', help='geneDriver for many cohorts: every gene of every cohort')
    cohort_lists(gc)
    gc.add_argument('--scale-by-mutations', action='store_false', default=True, dest="scale_by_expectation",
                    help='with --scale-factor-manual: use the manual factors instead of expected synonymous mutations')
    gc.add_argument('--no-pval-burden', dest='pval_burden', action='store_false', default=True, help='skip the burden p-values')
    gc.add_argument('--selection', action='store_true', default=False,
                    help='add the dN/dS-corrected expectations, their burden p-values and the selection p-values')
    gc.add_argument('--no-pval-burden-dnds', dest='pval_burden_dnds', action='store_false', default=True,
                    help='with --selection: skip the dN/dS-corrected burden p-values')
    gc.add_argument('--no-pval-sel', dest='pval_sel', action='store_false', default=True,
                    help='with --selection: skip the selection p-values')
    gc.set_defaults(func=cmd_gene_cohorts)

    return parser.parse_args(text.split()) if text else parser.parse_args()


def main(text=None):
    cli = parse_args(text)
    if cli.func in (cmd_gene, cmd_target, cmd_element):
        # these three read frames, hand numpy arrays to the library's `_host` entry points and write a frame: no tensor is ever made,
        # so PyTorch (1.5 s of import and device-layer start for milliseconds of GPU work) is not loaded at all
        from digdriver_amd import _lib
        _lib.TORCH_FREE = True
        _lib.prewarm_in_background()            # (the HIP runtime starts while pandas is imported and the files are parsed)
    cli.func(cli)
    if os.environ.get("DIG_CLI_ASSERT_NO_TORCH") == "1" and cli.func in (cmd_gene, cmd_target, cmd_element):
        assert "torch" not in sys.modules, "a torch-free sub-command imported torch"         # (tests: the claim above)


if __name__ == "__main__":
    main()
