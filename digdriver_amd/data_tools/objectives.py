"""The region model's training labels: mutation counts per window of a data container's `idx`, for many cohorts in one pass.

scripts/DataExtractor.py:525-572 (add_objectives without --cnv) is the reference: it joins a cohort's mutation file with the windows
(bedtools), tabulates per (window, sample) with duplicates dropped (mutation_tools.py:191-230), filters samples, and stores the sum
of OBS_SNV per window as float64 under a name made from the file's.  Here the join and the counting run in the library
(engine.window_objectives: dig_overlap_join_*, dig_window_pair_keys, dig_window_sample_hits, dig_window_objectives), on host arrays
through the `_host` entry points (no torch) or on device tensors; files are parsed and sample thresholds formed on the host.

Two properties of the reference that are kept on purpose (DESIGN, Training labels):
  * --max-muts-per-elt-per-sample clips OBS_MUT (mutation_tools.py:318-327) and the label is summed from OBS_SNV: the cap never
    changes a label.  The argument is accepted and does nothing.
  * a sample's load in both sample filters is SAMPLE.value_counts() of the (window, sample) frame: the number of distinct windows
    the sample hits, not its number of mutations.

The copy-number branch (add_objectives --cnv, DataExtractor.py:100-154,535-539) is window_cnv_objectives / add_cnv_objectives: per
window [START, START + W), W = idx[0, 2] - idx[0, 1] for every window, the mean over its W positions of the duplication, copy-neutral
/ LOH and deletion tracks of a cohort's segments, float64 [N, 3] per file (engine.window_cnv_means: dig_cnv_segment_deltas,
dig_cnv_window_means).  The reference reads the segments through a tabix index; here the file is read whole (a bgzip file is a
multi-member gzip file) and no index is needed.  DESIGN, Copy-number labels, has the decisions.
"""
import numpy as np

from .._marshal import is_cuda
from . import cohort_rows, tabulate_gpu


def objective_name(f_mut, suffix=''):
    """The dataset name add_objectives gives a cohort's labels (DataExtractor.py:569)."""
    return str(f_mut).split('/')[-1].split('.annot')[0].split('.txt')[0].split('.bed')[0] + suffix


def encode_objective_rows(f_mut, chrom_ids):
    """A mutation file (tab-separated, no header, 8 or more columns: CHROM START END REF ALT SAMPLE GENE ANNOT ...) as the arrays
    engine.window_objectives takes, for one cohort.  The raw rows count, as in the bedtools join: no autosome filter, and chromosome
    labels are compared as TEXT with `chrom_ids` (label -> id of the windows' chromosomes), so '1' is not 'chr1'; rows on other
    chromosomes can hit nothing and are left out, and so are rows without a SAMPLE label (the reference's group-by drops them).
    Returns dict(chrom, start, end i64; sample i32 dense in order of first appearance; uid i32: dense ids of the distinct (CHROM,
    START, END, REF, ALT); indel u8: ANNOT == 'INDEL' of the FIRST row of the file with the row's (uid, sample) -- the row
    drop_duplicates keeps, mutation_tools.py:208; n_uid; sample_names)."""
    import pandas as pd
    try:
        muts = pd.read_csv(f_mut, sep="\t", header=None, low_memory=False, dtype={0: str}, usecols=[0, 1, 2, 3, 4, 5, 7])
    except pd.errors.EmptyDataError:
        muts = pd.DataFrame({c: [] for c in (0, 1, 2, 3, 4, 5, 7)})
    ch = muts[0].map(chrom_ids)
    keep = (ch.notna() & muts[5].notna()).values
    muts, ch = muts.loc[keep], ch[keep].astype(np.int64).values
    n = len(muts)
    if n == 0:
        z = np.zeros(0, np.int64)
        return dict(chrom=z, start=z, end=z, sample=np.zeros(0, np.int32), uid=np.zeros(0, np.int32), indel=np.zeros(0, np.uint8),
                    n_uid=0, sample_names=[])
    start, end = muts[1].to_numpy(np.int64), muts[2].to_numpy(np.int64)
    ref_id = pd.factorize(muts[3].values)[0] + 1                       # (a missing allele: 0; missing equals missing, as in duplicated())
    alt_id = pd.factorize(muts[4].values)[0] + 1
    sample, sample_names = pd.factorize(muts[5].values)
    indel = (muts[7].values == 'INDEL')
    uid = tabulate_gpu._host_record(ch, start, end, ref_id, alt_id, sample, [], np.zeros(n, np.int64), indel, 0)['uid']
    n_uid = int(uid.max()) + 1
    n_ind = np.bincount(uid, weights=indel, minlength=n_uid)
    if ((n_ind > 0) & (n_ind < np.bincount(uid, minlength=n_uid))).any():
        # rows of one mutation that disagree on ANNOT: every row takes the class of the first row of its (uid, sample)
        order = np.lexsort((np.arange(n), sample, uid))
        new = np.concatenate([[True], (uid[order][1:] != uid[order][:-1]) | (sample[order][1:] != sample[order][:-1])])
        first = order[np.flatnonzero(new)][np.cumsum(new) - 1]
        fixed = np.empty(n, bool)
        fixed[order] = indel[first]
        indel = fixed
    return dict(chrom=ch, start=start, end=end, sample=sample.astype(np.int32), uid=uid.astype(np.int32), indel=indel.astype(np.uint8),
                n_uid=n_uid, sample_names=list(sample_names))


def keep_samples(hits, sample_offsets, max_muts_per_sample=None, sample_filter_stdev=None):
    """The samples that stay, u8 per global sample, from hits = the distinct windows each sample has a row in: per cohort
    filter_samples_by_stdev (mutation_tools.py:306-316: count > Series.std() * k with pandas' ddof = 1; one sample gives NaN and
    drops nothing) and filter_hypermut_samples (:293-304: count > m).  Both options are tested for truthiness as
    DataExtractor.py:553-557 tests them: 0 and None mean off.  A sample without any hit is in no row of the reference's frame and
    is left out of the standard deviation."""
    import pandas as pd
    hits = np.asarray(hits)
    keep = np.ones(len(hits), np.uint8)
    for lo, hi in zip(sample_offsets[:-1], sample_offsets[1:]):
        cnt = hits[lo:hi].astype(np.int64)
        if sample_filter_stdev:
            stdev = pd.Series(cnt[cnt > 0]).std()
            keep[lo:hi] &= ~(cnt > stdev * sample_filter_stdev)
        if max_muts_per_sample:
            keep[lo:hi] &= ~(cnt > max_muts_per_sample)
    return keep


def _windows(idx):
    idx = np.asarray(idx)
    if idx.ndim != 2 or idx.shape[1] != 3 or idx.dtype.kind not in "iu":
        raise ValueError("idx: an integer array [N, 3] of CHROM, START, END")
    idx = idx.astype(np.int64)
    if len(idx) and idx.min() < 0:
        raise ValueError("idx: non-negative entries")
    return idx


def window_objectives(idx, f_muts, max_muts_per_sample=None, sample_filter_stdev=None, max_muts_per_elt_per_sample=None,
                      on_device=None, device=0):
    """Labels of the N windows `idx` ([N, 3] ints: CHROM, START, END) for the cohorts `f_muts` (a mutation file, or a list of them;
    an entry may also be the dict encode_objective_rows made of a file): (names, labels float64 [N, C]) with names[c] =
    objective_name(f_muts[c]) and labels[:, c] what add_objectives stores for that file (DataExtractor.py:525-572 without --cnv).
    max_muts_per_elt_per_sample is accepted and changes nothing, as in the reference (this module's docstring).
    on_device: True = device tensors and the device entry points, False = numpy and the `_host` twins (no torch), None = the device
    unless the process is torch-free."""
    del max_muts_per_elt_per_sample
    idx = _windows(idx)
    f_muts = [f_muts] if isinstance(f_muts, (str, bytes, dict)) or hasattr(f_muts, "__fspath__") else list(f_muts)
    if not f_muts:
        raise ValueError("no mutation file")
    # windows with one name ('{}:{}-{}') are one element of the reference's frame: counted once, the label given to each
    uniq, inverse = np.unique(idx, axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    chrom_ids = {str(c): int(c) for c in np.unique(uniq[:, 0])}
    cohorts = [f if isinstance(f, dict) else encode_objective_rows(f, chrom_ids) for f in f_muts]
    names = [f.get("name", "cohort%d" % i) if isinstance(f, dict) else objective_name(f) for i, f in enumerate(f_muts)]
    offs = cohort_rows.sample_offsets(cohorts)
    cat = lambda k, dt, shift=None: cohort_rows.column(cohorts, k, dt, shift)
    rows = cohort_rows.place([cat("chrom", "i64"), cat("start", "i64"), cat("end", "i64"), cat("sample", "i32", offs), cat("uid", "i32"),
                              cat("indel", "u8")], on_device, device)
    from .. import engine
    out = engine.window_objectives(uniq[:, 0], uniq[:, 1], uniq[:, 2], *rows, offs, max([c["n_uid"] for c in cohorts] + [1]),
                                   keep_from_hits=lambda h: keep_samples(h, offs, max_muts_per_sample, sample_filter_stdev),
                                   device=device)
    labels = out["labels"].cpu().numpy() if is_cuda(out["labels"]) else out["labels"]
    return names, np.ascontiguousarray(labels[inverse])


def add_objectives(data_file, f_muts, suffix='', max_muts_per_sample=None, sample_filter_stdev=None,
                   max_muts_per_elt_per_sample=None, on_device=None, device=0):
    """DataExtractor.py addObjectives for one or more cohorts: reads `idx` from the data container (an HDF5 file or a directory
    mirror, io/mapfile.py), computes the labels of every file in one pass and stores each column as float64 [N] under
    objective_name(file, suffix).  An HDF5 container is extended in place (h5lite.append_dataset): no existing dataset is read or
    rewritten.  A name that exists already is refused before any device work, as h5py's create_dataset refuses it.
    Returns the names."""
    from ..io import mapfile
    f_muts = [f_muts] if isinstance(f_muts, (str, bytes)) or hasattr(f_muts, "__fspath__") else list(f_muts)
    names = [objective_name(f, suffix) for f in f_muts]
    for name in names:
        if not name:
            raise ValueError("a mutation file whose name gives an empty dataset name")
        if names.count(name) > 1:
            raise ValueError("two mutation files give the dataset name %r" % name)
        if mapfile.has_key(data_file, name):
            raise ValueError("Unable to create dataset (name already exists): %r in %s" % (name, data_file))
    idx = mapfile.read_array(data_file, 'idx')
    _, labels = window_objectives(idx, f_muts, max_muts_per_sample, sample_filter_stdev, max_muts_per_elt_per_sample, on_device, device)
    for c, name in enumerate(names):
        mapfile.write_array(data_file, name, np.ascontiguousarray(labels[:, c]), append=True)
    return names


def _open_text(path):
    """A text file that may be gzip or bgzip (a multi-member gzip file), told by its first two bytes."""
    import gzip
    with open(path, "rb") as f:
        magic = f.read(2)
    return gzip.open(path, "rt") if magic == b"\x1f\x8b" else open(path, "r")


def encode_cnv_rows(f_cnv, chrom_ids):
    """A copy-number segment file (tab-separated, no header, plain or gzip / bgzip: chr start end cp_num cp_Maj cp_min donor) as the
    arrays engine.window_cnv_means takes, for one cohort.  Only chr, start, end and cp_num are read.  Chromosome labels are compared as
    TEXT with `chrom_ids` (label -> id of the windows' chromosomes), as the reference queries its index with the decimal form of idx's
    CHROM: '1' matches, 'chr1' does not, and rows on other chromosomes are left out.  Every row counts: no de-duplication, no sample
    filter.  Class and weight come from cp_num alone: 2 -> LOH (1), weight 1, whatever cp_min says; below 2 -> deletion (2), weight
    2 - cp_num; above 2 -> duplication (0), weight cp_num - 2.
    ValueError, naming the file and the line, for a cp_num that is missing, negative or not integer-valued ("3" and "3.0" are), for
    coordinates that are not non-negative integers, and for end <= start -- on every row, whatever its chromosome.
    Returns dict(chrom, start, end i64; klass u8; weight i32)."""
    import pandas as pd
    with _open_text(f_cnv) as f:
        try:
            seg = pd.read_csv(f, sep="\t", header=None, dtype=str, usecols=[0, 1, 2, 3], skip_blank_lines=False, na_filter=False,
                              quoting=3)
        except pd.errors.EmptyDataError:
            seg = pd.DataFrame({c: [] for c in range(4)}, dtype=str)
        except ValueError as exc:
            raise ValueError("%s: a segment file has at least the four columns chr start end cp_num (%s)" % (f_cnv, exc)) from exc
    seg = seg[(seg != "").any(axis=1)]                                   # (blank lines; the index keeps the line numbers)
    line = seg.index.to_numpy() + 1

    def refuse(bad, what):
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise ValueError("%s, line %d: %s (%s)" % (f_cnv, line[i], what, "\t".join(seg.iloc[i].tolist())))

    num = [pd.to_numeric(seg[c], errors="coerce").to_numpy(np.float64) for c in (1, 2, 3)]
    whole = lambda x: np.isfinite(x) & (x == np.floor(x)) & (x >= 0) & (x < 2.0 ** 40)
    refuse(~whole(num[2]) | (num[2] > 2.0 ** 31), "cp_num must be a non-negative integer")
    refuse(~whole(num[0]) | ~whole(num[1]), "start and end must be non-negative integers")
    refuse(num[1] <= num[0], "end <= start")
    ch = seg[0].map(chrom_ids)
    keep = ch.notna().to_numpy()
    start, end, cp = (x[keep].astype(np.int64) for x in num)
    klass = np.where(cp == 2, 1, np.where(cp < 2, 2, 0)).astype(np.uint8)
    weight = np.where(cp == 2, 1, np.abs(cp - 2)).astype(np.int32)
    return dict(chrom=ch[keep].to_numpy(np.int64), start=start, end=end, klass=klass, weight=weight)


def window_cnv_objectives(idx, f_cnvs, on_device=None, device=0):
    """Copy-number labels of the N windows `idx` ([N, 3] ints: CHROM, START, END) for the cohorts `f_cnvs` (a segment file, or a list of
    them; an entry may also be the dict encode_cnv_rows made of a file): (names, labels float64 [N, 3, C]) with names[c] =
    objective_name(f_cnvs[c]) and labels[:, :, c] what add_objectives --cnv stores for that file (DataExtractor.py:535-539): columns
    duplications, copy-neutral / LOH, deletions.  Every window is [START, START + W) with W = idx[0, 2] - idx[0, 1], as in the
    reference, which never reads another row's END.  Windows may be unsorted, repeated or overlapping.  A chromosome of idx without a
    row in a file gives zeros (the reference's tabix fetch raises there).
    on_device: as in window_objectives."""
    idx = _windows(idx)
    f_cnvs = [f_cnvs] if isinstance(f_cnvs, (str, bytes, dict)) or hasattr(f_cnvs, "__fspath__") else list(f_cnvs)
    if not f_cnvs:
        raise ValueError("no segment file")
    if len(idx) == 0:
        raise ValueError("idx: no window (the window width is idx[0, 2] - idx[0, 1])")
    W = int(idx[0, 2] - idx[0, 1])
    if W < 1:
        raise ValueError("idx: the first window is empty (the window width is idx[0, 2] - idx[0, 1] = %d)" % W)
    chrom_ids = {str(c): int(c) for c in np.unique(idx[:, 0])}
    cohorts = [f if isinstance(f, dict) else encode_cnv_rows(f, chrom_ids) for f in f_cnvs]
    names = [f.get("name", "cohort%d" % i) if isinstance(f, dict) else objective_name(f) for i, f in enumerate(f_cnvs)]
    cat = lambda k, dt: cohort_rows.column(cohorts, k, dt)
    rows = cohort_rows.place([cat("chrom", "i64"), cat("start", "i64"), cat("end", "i64"), cat("klass", "u8"), cat("weight", "i32"),
                              cohort_rows.cohort_column(cohorts, "chrom")], on_device, device)
    from .. import engine
    labels = engine.window_cnv_means(idx[:, 0], idx[:, 1], W, *rows, len(cohorts), device=device)
    return names, np.ascontiguousarray(labels.cpu().numpy() if is_cuda(labels) else labels)


def add_cnv_objectives(data_file, f_cnvs, suffix='', on_device=None, device=0):
    """DataExtractor.py addObjectives --cnv for one or more cohorts: reads `idx` from the data container (an HDF5 file or a directory
    mirror, io/mapfile.py), computes the labels of every file in one pass and stores each cohort's float64 [N, 3] under
    objective_name(file, suffix).  An HDF5 container is extended in place (h5lite.append_dataset): no existing dataset is read or
    rewritten.  The same refusals as add_objectives, before any device work.  Returns the names."""
    from ..io import mapfile
    f_cnvs = [f_cnvs] if isinstance(f_cnvs, (str, bytes)) or hasattr(f_cnvs, "__fspath__") else list(f_cnvs)
    names = [objective_name(f, suffix) for f in f_cnvs]
    for name in names:
        if not name:
            raise ValueError("a segment file whose name gives an empty dataset name")
        if names.count(name) > 1:
            raise ValueError("two segment files give the dataset name %r" % name)
        if mapfile.has_key(data_file, name):
            raise ValueError("Unable to create dataset (name already exists): %r in %s" % (name, data_file))
    idx = mapfile.read_array(data_file, 'idx')
    _, labels = window_cnv_objectives(idx, f_cnvs, on_device, device)
    for c, name in enumerate(names):
        mapfile.write_array(data_file, name, np.ascontiguousarray(labels[:, :, c]), append=True)
    return names
