#!/usr/bin/env python
"""DigPreprocess.py -- sequence-context preprocessing on MI355X.

The sub-commands of the reference's scripts/DigPreprocess.py that feed the burden-test path with context counts and
annotated mutation files.  The reference's addMutationFunction shells out to an R script that needs Bioconductor and dNdScv's
refcds_hg19.rda; here the gene table comes from a bed12 file of coding exons (--cds-bed) and the CDS letters from the FASTA:

    countGenomeContext        window context counts of a genome, --up/--down 1 or 2 (DigPreprocess.py:19-73)
    addMutationFunction       GENE and ANNOT columns of a raw call file (:102-109, scripts/mutationFunction.R)
    addMutationContext        MUT_TYPE and CONTEXT columns of a mutation file (:75-100)
    annotMutationFile         addMutationFunction, then addMutationContext (:111-117)
    initialize_f_data         start an element-data container            (:147-153)
    preprocess_genic_model    the gene container from bed12 + FASTA (--cds-bed) and the genes' window counts (:119-127)
    preprocess_element_model  per-element L counts from bed12 + FASTA    (:129-145)
    preprocess_tiled          L counts of a tiled genome                 (:155-164)

Same positional arguments and option names.  Sequence is read once into a 4-bit packed array (cached next to the
FASTA) and counted by dig_count_contexts2 / dig_count_contexts5 instead of per-region pysam fetches; the mutation contexts come from
dig_mutation_contexts and the genic function from dig_mutation_function over the same genome.  preprocess_genic_model --cds-bed
builds what the reference takes from refcds_hg19.rda and has no code for: the gene container (window_{w}/genes/ with L, the
possible substitutions of every gene by class and type, from dig_gene_site_counts) that DigPretrain.py genicModel reads.
"""
import argparse
import os
import sys

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from digdriver_amd.io import mapfile                                       # noqa: E402
from digdriver_amd.sequence_model import sequence_tools                    # noqa: E402


def count_genome_context(args):
    if bool(args.h5) == bool(args.bed):
        raise SystemExit("Exactly one of --h5 or --bed must be supplied.")
    if (args.up, args.down) not in ((1, 1), (2, 2)):
        raise SystemExit("This build counts trinucleotide (--up 1 --down 1) or penta-nucleotide (--up 2 --down 2) contexts.")
    if args.map_file:
        raise SystemExit("--map-file needs the bigWig reader of the reference's preprocessing stack (out of scope).")
    if args.h5:
        df_bed = pd.DataFrame(mapfile.read_array(args.h5, 'idx'))
    else:
        df_bed = pd.read_table(args.bed, header=None, low_memory=False)
        df_bed[0] = df_bed[0].astype(str)
        df_bed = df_bed[df_bed[0].isin([str(i) for i in range(1, 23)])].copy()      # autosomes (:37-39)
        df_bed[0] = df_bed[0].astype(int)
    df_bed = df_bed.sort_values(by=[0, 1])
    print('Counting nucleotide contexts in {} regions'.format(len(df_bed)))
    df = sequence_tools.count_contexts_in_bed(args.fasta, df_bed, n_up=args.up, n_down=args.down)
    idx = df_bed.iloc[:, 0:3].values
    print('Saving context counts to {}'.format(args.fout))
    with mapfile.batch(args.fout):
        mapfile.write_frame(args.fout, 'genome_counts', df.sum(axis=0).to_frame('COUNT'))
        mapfile.write_frame(args.fout, 'all_window_genome_counts', df)
        mapfile.write_array(args.fout, 'idx', idx.astype(np.int32))
        mapfile.write_attrs(args.fout, n_up=args.up, n_down=args.down, collapse=0)


def add_mutation_context(args):
    # torch-free: the `_host` twin path, as the single-cohort DigDriver commands
    from digdriver_amd import _lib
    _lib.TORCH_FREE = True
    if args.up < 0 or args.down < 0 or args.up + args.down + 1 > 16:
        raise SystemExit("--up and --down must be >= 0 with up + down + 1 <= 16.")
    print('Reading in mutation file')
    fout = args.fout[:-3] if args.fout.endswith('.gz') else args.fout
    try:
        sequence_tools.write_mutation_contexts(args.fmut, args.fasta, fout, n_up=args.up, n_down=args.down, on_device=False)
    except ValueError as exc:
        raise SystemExit("addMutationContext: %s" % exc)
    print('Saved annotated mutation file: {}'.format(fout))


def _mutation_function(args, fout):
    from digdriver_amd.data_tools import mutation_tools
    try:
        counts = mutation_tools.annotate_mutation_function(args.fmut, fout, args.cds_bed, args.fasta, on_device=False)
    except (ValueError, KeyError) as exc:
        raise SystemExit("addMutationFunction: %s" % exc)
    print("\t{coding_snv}\tcoding SNVs\n\t{noncoding_snv}\tnoncoding SNVs\n\t{coding_other}\tcoding INDELs\n"
          "\t{noncoding_other}\tnoncoding INDELs".format(**counts))


def add_mutation_function(args):
    # torch-free, as addMutationContext
    from digdriver_amd import _lib
    _lib.TORCH_FREE = True
    fout = args.fout[:-3] if args.fout.endswith('.gz') else args.fout
    _mutation_function(args, fout)
    print('Saved annotated mutation file: {}'.format(fout))


def annot_mutation_file(args):
    from digdriver_amd import _lib
    _lib.TORCH_FREE = True
    if args.up < 0 or args.down < 0 or args.up + args.down + 1 > 16:
        raise SystemExit("--up and --down must be >= 0 with up + down + 1 <= 16.")
    fout = args.fout[:-3] if args.fout.endswith('.gz') else args.fout
    print('Adding mutation function')
    _mutation_function(args, fout)
    print('Adding mutation context')
    try:                                               # (load_genome keeps the packed genome of `fasta`: one pack for both steps)
        sequence_tools.write_mutation_contexts(fout, args.fasta, fout, n_up=args.up, n_down=args.down, on_device=False)
    except ValueError as exc:
        raise SystemExit("annotMutationFile: %s" % exc)
    print('Saved annotated mutation file: {}'.format(fout))


def initialize_data(args):
    idx = mapfile.read_array(args.f_genome_counts, 'idx')
    if not mapfile.has_key(args.f_genome_counts, 'all_window_genome_counts'):
        raise SystemExit("f_genome_counts does not hold 'all_window_genome_counts'.")
    sequence_tools.initialize_nonc_data(args.f_annot_data, args.f_genome_counts, int(idx[0, 2] - idx[0, 1]))


def preprocess_cds_contexts(args):
    # torch-free, as addMutationFunction
    from digdriver_amd import _lib
    _lib.TORCH_FREE = True
    key = 'window_{}'.format(args.window)
    if args.cds_bed:
        print('Building the gene container from {}'.format(args.cds_bed))
        try:
            genes = sequence_tools.preprocess_genic(args.cds_bed, args.f_fasta, args.f_genic, args.window, on_device=False)
        except (ValueError, KeyError) as exc:
            raise SystemExit("preprocess_genic_model: %s" % exc)
        print('Saved {} genes under {}/genes of {}'.format(len(genes), key, args.f_genic))
    elif not mapfile.has_key(args.f_genic, key + '/genes/names'):
        raise SystemExit("f_genic does not hold {}/genes: pass --cds-bed (a bed12 file of coding exons) to build it.".format(key))
    if not (mapfile.has_key(args.f_genic, key + '/full_window_si_index') and mapfile.has_key(args.f_genic, key + '/full_window_si_values')):
        print("Note: {} does not hold {}/full_window_si_index and full_window_si_values, which genicModel reads: start the "
              "container with initialize_f_data.".format(args.f_genic, key))
    results = sequence_tools.si_count_parallel(args.f_genic, args.f_fasta, args.window, args.N_procs, on_device=False)
    mapfile.write_frame(args.out_file, args.out_key, results)
    print('Saved window context counts of {} genes to {}:{}'.format(len(results), args.out_file, args.out_key))


def preprocess_nonc_contexts(args):
    if args.f_sites:
        print("preprocessing sites data")
        sequence_tools.preprocess_sites(args.f_sites, args.f_element_data, args.f_pretrained, args.save_key, args.window)
        return
    if not args.f_element_bed:
        raise SystemExit("ERROR: need to pass in an elements file (--f-bed) for preprocessing")
    print("Preprocessing elements")
    L = sequence_tools.precount_region_contexts_parallel(args.f_element_bed, args.f_fasta, args.N_procs, args.window,
                                                         args.use_sub_elts)
    print('window counts by elt')
    sequence_tools.preprocess_nonc(args.f_element_bed, args.f_element_data, args.f_pretrained, L, args.save_key, args.window)


def preprocess_tiled(args):
    print("Counting sequence contexts in regions")
    L = sequence_tools.precount_region_contexts_parallel(args.f_nonc_bed, args.f_fasta, args.N_procs, args.window, False)
    mapfile.write_frame(args.f_nonc_data, "{}/L_counts".format(args.save_key), L.astype(np.int32))


def parse_args(text=None):
    parser = argparse.ArgumentParser(description='Sequence-context preprocessing for the burden-test path (MI355X build).')
    sub = parser.add_subparsers()
    a = sub.add_parser('countGenomeContext', help='tri- or penta-nucleotide context counts of genome windows')
    a.add_argument('fasta', type=str, help='reference genome FASTA')
    a.add_argument('fout', type=str, help='container to write')
    a.add_argument('--h5', type=str, default='', help='container holding the windows as `idx`')
    a.add_argument('--bed', type=str, default='', help='headerless bed file of windows')
    a.add_argument('--up', type=int, default=1, help='bases upstream (1)')
    a.add_argument('--down', type=int, default=1, help='bases downstream (1)')
    a.add_argument('--n-procs', type=int, default=1, help='accepted for compatibility')
    a.add_argument('--map-file', type=str, default='', help='not supported here')
    a.add_argument('--map-thresh', type=float, default=0.5, help='unused')
    a.set_defaults(func=count_genome_context)

    b = sub.add_parser('addMutationContext', help='annotate a mutation file with MUT_TYPE and sequence CONTEXT')
    b.add_argument('fmut', type=str, help='8-column mutation file: CHROM START END REF ALT SAMPLE GENE ANNOT (plain or gzip)')
    b.add_argument('fasta', type=str, help='reference genome FASTA')
    b.add_argument('fout', type=str, help='output file name (a trailing .gz is dropped; not compressed)')
    b.add_argument('--up', type=int, default=1, help='bases upstream of the mutation in the context (1)')
    b.add_argument('--down', type=int, default=1, help='bases downstream of the mutation in the context (1)')
    b.add_argument('--n-procs', type=int, default=1, help='accepted for compatibility')
    b.set_defaults(func=add_mutation_context)

    cds_help = ('bed12 file of the coding exons of every gene (strand in column 6, CDS blocks in columns 10-12), e.g. the '
                "reference's DIGDriver/data/genes.MARTINCORENA.bed; required: it and the FASTA replace the refcds_hg19.rda the "
                "reference's R script loads")
    c = sub.add_parser('addMutationFunction', help='annotate a raw call file with GENE and the genic function ANNOT')
    c.add_argument('fmut', type=str, help='raw calls, no header: CHROM POS REF ALT SAMPLE, or CHROM START END REF ALT SAMPLE ...')
    c.add_argument('fout', type=str, help='output file name (a trailing .gz is dropped; not compressed)')
    c.add_argument('--cds-bed', type=str, required=True, help=cds_help)
    c.add_argument('--fasta', type=str, required=True, help='reference genome FASTA (the CDS letters are read from it)')
    c.set_defaults(func=add_mutation_function)

    d = sub.add_parser('annotMutationFile', help='addMutationFunction followed by addMutationContext')
    d.add_argument('fmut', type=str, help='raw calls, no header: CHROM POS REF ALT SAMPLE, or CHROM START END REF ALT SAMPLE ...')
    d.add_argument('fasta', type=str, help='reference genome FASTA')
    d.add_argument('fout', type=str, help='output file name (a trailing .gz is dropped; not compressed)')
    d.add_argument('--cds-bed', type=str, required=True, help=cds_help)
    d.add_argument('--up', type=int, default=1, help='bases upstream of the mutation in the context (1)')
    d.add_argument('--down', type=int, default=1, help='bases downstream of the mutation in the context (1)')
    d.add_argument('--n-procs', type=int, default=1, help='accepted for compatibility')
    d.set_defaults(func=annot_mutation_file)

    c1 = sub.add_parser('preprocess_genic_model', help='the gene container (with --cds-bed) and the context counts of the windows '
                                                      'each gene overlaps')
    c1.add_argument('f_genic', help='gene-data container (see initialize_f_data)')
    c1.add_argument('f_fasta', help='reference genome FASTA (hg19)')
    c1.add_argument('out_file', help='container to save the window counts to')
    c1.add_argument('--out-key', default='cds/window_10kb', help='key of the saved frame')
    c1.add_argument('--n-procs', default=1, type=int, dest='N_procs', help='accepted for compatibility')
    c1.add_argument('--window', type=int, default=10000, help='window size in bp')
    c1.add_argument('--cds-bed', type=str, default='', help='build window_{w}/genes of f_genic first, from this ' + cds_help[0].lower() +
                    cds_help[1:cds_help.index('; required')])
    c1.set_defaults(func=preprocess_cds_contexts)

    e = sub.add_parser('preprocess_element_model', help='per-element context counts from a bed12 file')
    e.add_argument('f_element_data', help='element-data container (see initialize_f_data)')
    e.add_argument('f_pretrained', help='any pretrained map (kept for compatibility)')
    e.add_argument('f_fasta', help='reference genome FASTA (hg19)')
    e.add_argument('save_key', help='key of the element set')
    e.add_argument('--f-bed', dest='f_element_bed', help='bed12 file of the elements')
    e.add_argument('--f-sites', type=str, default=None, help='sites file (element name in the SAMPLE column)')
    e.add_argument('--ignore-sub_elts', action='store_false', default=True, dest='use_sub_elts',
                   help='count whole element spans instead of blocks')
    e.add_argument('--n-procs', default=1, type=int, dest='N_procs', help='accepted for compatibility')
    e.add_argument('--window', type=int, default=10000, help='window size in bp')
    e.set_defaults(func=preprocess_nonc_contexts)

    f = sub.add_parser('initialize_f_data', help='start an element-data container from genome window counts')
    f.add_argument('f_annot_data', help='container to create')
    f.add_argument('f_genome_counts', help='output of countGenomeContext')
    f.set_defaults(func=initialize_data)

    g = sub.add_parser('preprocess_tiled', help='context counts of a tiled genome')
    g.add_argument('f_nonc_bed', help='bed file of the tiles')
    g.add_argument('f_nonc_data', help='element-data container')
    g.add_argument('f_fasta', help='reference genome FASTA')
    g.add_argument('--n-procs', default=1, type=int, dest='N_procs', help='accepted for compatibility')
    g.add_argument('window', type=int, default=10000, help='window size in bp')
    g.add_argument('save_key', help='key of the tile set')
    g.set_defaults(func=preprocess_tiled)
    return parser.parse_args(text.split()) if text else parser.parse_args()


if __name__ == "__main__":
    cli = parse_args()
    cli.func(cli)
    if os.environ.get("DIG_CLI_ASSERT_NO_TORCH") == "1" and cli.func in (add_mutation_context, add_mutation_function,
                                                                            annot_mutation_file, preprocess_cds_contexts):
        assert "torch" not in sys.modules, "a torch-free sub-command imported torch"         # (tests: the claim above)
