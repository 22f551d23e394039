#!/usr/bin/env python
"""DataExtractor.py -- training labels for the region model on MI355X.

Of the reference's scripts/DataExtractor.py this build has what a user must run to train a map for a new cohort, because the
epigenomic tensor x_data is shared across cohorts:

    addObjectives      mutation counts of a cohort per window of the data container's `idx`, stored in the container as float64
                       under a name made from the mutation file's (DataExtractor.py:525-572, 849-861)
    addCnvObjectives   the reference's `addObjectives --cnv` as a sub-command of its own: per window the mean over its positions of the
                       duplication, copy-neutral / LOH and deletion tracks of a cohort's copy-number segments, float64 [N, 3] per file
                       (DataExtractor.py:100-154, 535-539).  Segment files are read whole, plain or gzip / bgzip: no tabix index.

addObjectives: same positional arguments and option names.  mut_file takes one file -- the reference's behaviour -- or several, which are counted
in one pass (one label vector per file).  The join with the windows and the counting run in libdig_hip.so (dig_overlap_join_*,
dig_window_pair_keys, dig_window_sample_hits, dig_window_objectives) through the `_host` entry points: no torch, h5py, pybedtools
or bedtools.  An HDF5 container is extended in place: x_data is neither read nor rewritten.

addCnvObjectives h5_file cnv_file [cnv_file ...] [--suffix S]: the arithmetic runs in libdig_hip.so (dig_cnv_segment_deltas,
dig_cnv_window_means) through the `_host` entry points, all files in one pass.  `addObjectives --cnv` itself stays refused and points here.

Not built: the other sub-commands -- mappability, splitDataIdx, createChunk, rescaleTensor,
countMutations, mergeTracks, concatH5, addMappability, addTracks, unzipH5 (and createMeanPred) -- which build, reshape or extend the
track tensor x_data itself from bigWig files (pyBigWig / bbi) and tabix archives; DESIGN, Training labels.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def add_objectives(args):
    if args.cnv:
        raise SystemExit("addObjectives --cnv is not built: copy-number labels are the sub-command addCnvObjectives h5_file cnv_file "
                         "[cnv_file ...] [--suffix S].")
    from digdriver_amd import _lib
    _lib.TORCH_FREE = True
    _lib.prewarm_in_background()                # (the HIP runtime starts while pandas is imported and the files are parsed)
    from digdriver_amd.data_tools import objectives
    for f in args.mut_file:
        print(f)
        print('Adding mutation counts from {} to {}'.format(f, args.h5_file))
    try:
        names = objectives.add_objectives(args.h5_file, args.mut_file, suffix=args.suffix, max_muts_per_sample=args.max_muts_per_sample,
                                          sample_filter_stdev=args.sample_filter_stdev,
                                          max_muts_per_elt_per_sample=args.max_muts_per_elt_per_sample, on_device=False)
    except ValueError as exc:
        raise SystemExit(str(exc))
    for name in names:
        print('Saving dataset as {}'.format(name))


def add_cnv_objectives(args):
    from digdriver_amd import _lib
    _lib.TORCH_FREE = True
    _lib.prewarm_in_background()
    from digdriver_amd.data_tools import objectives
    for f in args.cnv_file:
        print(f)
        print('Adding CNV counts from {} to {}'.format(f, args.h5_file))
    try:
        names = objectives.add_cnv_objectives(args.h5_file, args.cnv_file, suffix=args.suffix, on_device=False)
    except ValueError as exc:
        raise SystemExit(str(exc))
    for name in names:
        print('Saving dataset as {}'.format(name))


def parse_args(text=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    subparsers = parser.add_subparsers(dest='command', help='addObjectives, addCnvObjectives (the other sub-commands of the reference read bigWig files: not built)')
    subparsers.required = True
    parser_g = subparsers.add_parser('addObjectives', help='count mutations (SNVs) for a cancer type to an hd5 dataset.')
    parser_g.add_argument('h5_file', help='path to h5 file')
    parser_g.add_argument('mut_file', nargs='+', help='path to file of mutations (several files: one label vector each, counted in one pass)')
    parser_g.add_argument('--max-muts-per-sample', type=int, default=None, help='Maximum mutations allowed per sample. Samples with higher mutation counts are removed. (As in the reference, a sample\'s count is the number of windows it hits.)')
    parser_g.add_argument('--sample-filter-stdev', type=float, default=None, help='Remove samples with # mutations > filter-stdev * stdev of mutation counts across cohort. (The same count.)')
    parser_g.add_argument('--max-muts-per-elt-per-sample', type=int, default=None, help='Cap the number of mutations a sample can contribute to any one window. Accepted and without effect, as in the reference: its cap clips OBS_MUT and the label is summed from OBS_SNV.')
    parser_g.add_argument('--suffix', type=str, default='', help='suffix to add to end of cancer name when saving mutation counts to h5 archive.')
    parser_g.add_argument('--cnv', help='designates the mut file is of CNVs (not built: use addCnvObjectives)', action='store_true')
    parser_g.set_defaults(func=add_objectives)
    parser_c = subparsers.add_parser('addCnvObjectives', help='add the mean duplication / LOH / deletion tracks of a cancer type per window to an hd5 dataset.')
    parser_c.add_argument('h5_file', help='path to h5 file')
    parser_c.add_argument('cnv_file', nargs='+', help='path to file of copy-number segments: chr start end cp_num cp_Maj cp_min donor, plain or gzip / bgzip (several files: one [N, 3] dataset each, computed in one pass)')
    parser_c.add_argument('--suffix', type=str, default='', help='suffix to add to end of cancer name when saving the labels to h5 archive.')
    parser_c.set_defaults(func=add_cnv_objectives)
    return parser.parse_args(text)


if __name__ == "__main__":
    cli = parse_args()
    cli.func(cli)
