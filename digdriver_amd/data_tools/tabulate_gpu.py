"""Observed-count tabulation on the GPU for many cohorts at once: mutations x element blocks -> OBS_SNV,
OBS_SAMPLES, OBS_INDEL as [E, C] int32 tensors, ready for dig_element_stats.

Same integer semantics as mutation_tools.tabulate_mutations_in_element (reference mutation_tools.py:155-230):
interval join -> drop duplicates on (chrom, start, end, ref, alt, sample, element) -> SNV / INDEL counts per
(element, sample) -> drop samples whose total count exceeds max_muts_per_sample -> cap the per-(element, sample)
counts -> per element: number of distinct samples, sum of SNVs, sum of indels.  The join runs in the HIP kernels
dig_overlap_join_{count,fill}; de-duplication and the segmented counts are sort/unique calls on the device
(PyTorch as plumbing).  Results are bit-identical to the host path (tests/test_gpu_tabulate.py).
"""
import numpy as np

from .. import engine
from .._marshal import device_backend
from . import cohort_rows, mutation_tools


class ElementBlocks:
    """bed6 blocks of an element set, sorted by (chrom, start), as device tensors with composite keys."""

    def __init__(self, chrom, start, end, elt_id, n_elements, device):
        import torch
        order, start_key, runmax_key, end_eff = engine.join_blocks(chrom, start, end)
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=device)
        self.start_key, self.runmax_key, self.end = t(start_key), t(runmax_key), t(end_eff)
        self.elt = t(np.asarray(elt_id, np.int64)[order])
        self.n_blocks, self.n_elements, self.device = len(order), int(n_elements), device

    @classmethod
    def from_bed12(cls, f_bed, device, names=None):
        """bed12 file -> blocks; element ids follow `names` (default: first appearance in the file).
        Chromosome labels are compared as TEXT, as bedtools does (mutation_tools.py:193-200): every label of the bed
        file gets an id (`blocks.chrom_ids`, pass it to encode_mutations); '1' and 'chr1' are different chromosomes and
        sex chromosomes are joined like any other."""
        import pandas as pd
        df = pd.read_csv(f_bed, sep="\t", header=None, low_memory=False, dtype={0: str})
        blocks = mutation_tools._bed12_to_bed6(df)
        labels = blocks.CHROM.astype(str)
        chrom_ids = {lab: i + 1 for i, lab in enumerate(dict.fromkeys(labels.tolist()))}
        if names is None:
            names = list(dict.fromkeys(df[3].tolist()))
        pos = {n: i for i, n in enumerate(names)}
        obj = cls(labels.map(chrom_ids).values, blocks.START.values, blocks.END.values, blocks.ELT.map(pos).values,
                  len(names), device)
        obj.chrom_ids = chrom_ids
        return obj, names


def overlap_pairs(blocks, m_chrom, m_start, m_end):
    """(mutation row, block row) pairs on the device: int32 tensors, mutation-major, blocks ascending."""
    return engine.overlap_join(device_backend(blocks.device), blocks.start_key, blocks.runmax_key, blocks.end, m_chrom, m_start, m_end)


def encode_mutations_host(df_mut, cohort_id=0, chrom_ids=None):
    """Mutation frame (reference column names) -> host arrays.  Strings become dense integer ids: `uid` identifies
    (CHROM, START, END, REF, ALT) and `sample` the sample label, both exactly (no hashing).
    `chrom_ids`: label -> id of the block set the mutations will be joined with (ElementBlocks.from_bed12: labels
    compared as text, rows on other chromosomes cannot hit anything and are dropped here).  Without it the blocks
    carry the integer autosome numbers of a pretrained model (bed12_boundaries, mutation_tools.py:383-414) and the
    mutation labels '1' ... '22' (optionally 'chr'-prefixed) are mapped onto them."""
    import pandas as pd
    if chrom_ids is not None:
        ch = df_mut.CHROM.astype(str).map(chrom_ids)
        keep = ch.notna()
        df_mut, ch = df_mut[keep], ch[keep].astype(np.int64)
    else:
        ch = df_mut.CHROM.astype(str).map(_strip_chr)           # (ONE leading "chr", the rule of all three file routes)
        keep = ch.isin(_AUTOSOME_LABELS) & df_mut.SAMPLE.notna()      # (a missing SAMPLE: the reference's groupby drops such rows)
        df_mut, ch = df_mut[keep], ch[keep].astype(np.int64)
    ref_id = pd.factorize(df_mut.REF.astype(str).values)[0]
    alt_id = pd.factorize(df_mut.ALT.astype(str).values)[0]
    samp, sample_names = pd.factorize(df_mut.SAMPLE.astype(str).values)
    # gene label of the row (get_unique_indels keys on it, mutation_tools.py:111-117); files without the column: one label
    gene = pd.factorize(df_mut.GENE.astype(str).values)[0] if 'GENE' in df_mut.columns else np.zeros(len(df_mut), np.int64)
    return _host_record(ch.values, df_mut.START.values, df_mut.END.values, ref_id, alt_id, samp, list(sample_names), gene,
                        (df_mut.ANNOT == 'INDEL').values, cohort_id)


def _host_record(ch, start, end, ref_id, alt_id, samp, sample_names, gene, indel, cohort_id):
    # exact ids of the distinct (CHROM, START, END, REF, ALT): the two string columns are factorized on their own (few
    # distinct alleles), then the five integer columns are grouped as rows (a MultiIndex factorize of the same columns
    # took 0.5 s per 200 000 mutations, 85 % of the many-cohort driver's wall time)
    ch, start, end = np.asarray(ch, np.int64), np.asarray(start, np.int64), np.asarray(end, np.int64)
    ref_id, alt_id = np.asarray(ref_id, np.int64), np.asarray(alt_id, np.int64)
    n = len(ch)
    if n == 0:
        uid = np.zeros(0, np.int64)
    else:
        span = end - start
        if (ch.min() >= 0 and ch.max() < (1 << 20) and start.min() >= 0 and start.max() < (1 << 40) and span.min() >= 0 and
                span.max() < (1 << 22) and ref_id.max() < (1 << 20) and alt_id.max() < (1 << 20)):
            # two packed 62-bit keys and one two-key sort (np.unique over the five-column rows: 0.6 s per 300 000 mutations)
            k1, k2 = (ch << 40) | start, (span << 40) | (ref_id << 20) | alt_id
            order = np.lexsort((k2, k1))
            new = np.concatenate([[True], (k1[order][1:] != k1[order][:-1]) | (k2[order][1:] != k2[order][:-1])])
            uid = np.empty(n, np.int64)
            uid[order] = np.cumsum(new) - 1
        else:
            uid = np.unique(np.stack([ch, start, end, ref_id, alt_id], axis=1), axis=0, return_inverse=True)[1].reshape(-1)
    c = lambda a: np.ascontiguousarray(a, dtype=np.int64)
    first_row, first_indel = dedup_flags(uid, samp, gene, indel)
    return dict(chrom=c(ch), start=c(start), end=c(end), uid=c(uid), sample=c(samp), indel=c(indel), gene=c(gene),
                first_row=first_row, first_indel=first_indel,
                cohort=np.full(n, int(cohort_id), np.int64), sample_names=list(sample_names))


def dedup_flags(uid, sample, gene, indel):
    """The reference's two de-duplications of a cohort's rows, one after the other (read_mutation_file(drop_duplicates=True,
    unique_indels=True), mutation_tools.py:106-117), as per-row 0 / 1 flags in file order: first_row[i] -- no earlier row has
    the same mutation id and sample (drop_duplicate_mutations keeps it); first_indel[i] -- row i is such a row, is an INDEL,
    and no earlier such row has the same mutation id and GENE label (get_unique_indels keeps it).  (The native parser's
    dig_mutation_file_flags_host gives the same arrays.)"""
    uid, sample, gene = np.asarray(uid, np.int64), np.asarray(sample, np.int64), np.asarray(gene, np.int64)
    indel = np.asarray(indel).astype(bool)
    n = len(uid)
    first_row, first_indel = np.zeros(n, np.int64), np.zeros(n, np.int64)
    if n:
        order = np.lexsort((np.arange(n), sample, uid))
        new = np.concatenate([[True], (uid[order][1:] != uid[order][:-1]) | (sample[order][1:] != sample[order][:-1])])
        first_row[order[new]] = 1
        rows = np.flatnonzero((first_row == 1) & indel)
        if len(rows):
            o2 = np.lexsort((rows, gene[rows], uid[rows]))
            r2 = rows[o2]
            new2 = np.concatenate([[True], (uid[r2][1:] != uid[r2][:-1]) | (gene[r2][1:] != gene[r2][:-1])])
            first_indel[r2[new2]] = 1
    return first_row, first_indel


GENE_ROW_CLASSES = {'Synonymous': 0, 'Missense': 1, 'Nonsense': 2, 'Essential_Splice': 3, 'INDEL': 4}     # anything else: 5
_INDEL_KEY = ['CHROM', 'START', 'END', 'REF', 'ALT', 'GENE']


def encode_gene_rows(f_mut, gene_index, cohort_id=0, keep=None):
    """The coding rows of a cohort file as engine.gene_counts takes them: the rows of transfer_tools.read_mutations_cds --
    read_mutation_file(drop_duplicates=False, drop_sex=True) with GENE != '.', i.e. autosomes only, SNV duplicates kept, an INDEL row
    kept only when no earlier INDEL row of the file has the same (CHROM, START, END, REF, ALT, GENE) (get_unique_indels,
    mutation_tools.py:111-117) -- as integer arrays.  That indel rule is NOT dedup_flags' first_indel, which sits behind
    drop_duplicate_mutations and loses a row when one sample carries an indel under two gene labels; the flag is formed here, by a
    lexsort as dedup_flags forms its own.
    gene_index: the gene model's index (G labels).  keep: a set of gene labels; rows of other genes are left out (run_gene_model's
    cgc_genes).  Returns dict(gene i32: the label's place in gene_index, G for a gene outside it, G + 1 for TP53 when gene_index
    has no TP53; sample i32: dense ids in order of first appearance; annot u8: GENE_ROW_CLASSES, 5 for any other label; cohort i32;
    sample_names).  ValueError for a file without a coding row, and for a coding row without a SAMPLE label."""
    import pandas as pd
    rows = mutation_tools.read_mutation_file(f_mut, drop_duplicates=False, drop_sex=True, unique_indels=False)
    if 'GENE' not in rows.columns or 'ANNOT' not in rows.columns:
        raise ValueError("{}: no GENE / ANNOT columns (an annotated mutation file has 8 or more)".format(f_mut))
    rows = rows.loc[rows.GENE != '.']
    if len(rows) == 0:
        raise ValueError("{}: no coding row (a row with a gene label on an autosome)".format(f_mut))
    indel = (rows.ANNOT == 'INDEL').values
    if indel.any():
        cols = [pd.factorize(rows[c].values[indel])[0] for c in _INDEL_KEY]
        at = np.flatnonzero(indel)
        order = np.lexsort([at] + cols[::-1])
        new = np.ones(len(at), bool)
        for col in cols:
            new[1:] &= col[order][1:] == col[order][:-1]
        new[1:] = ~new[1:]
        drop = np.zeros(len(rows), bool)
        drop[at[order[~new]]] = True
        rows = rows.loc[~drop]
    if keep is not None:
        rows = rows.loc[rows.GENE.isin(keep)]
    if rows.SAMPLE.isna().any():
        raise ValueError("{}: a coding row without a SAMPLE label".format(f_mut))
    labels = list(gene_index)
    G = len(labels)
    place = {name: i for i, name in enumerate(labels)}
    codes, uniq = pd.factorize(rows.GENE.values)
    lookup = np.array([place.get(u, G + 1 if u == 'TP53' else G) for u in uniq] + [G], np.int32)       # (a missing label: code -1)
    sample, sample_names = pd.factorize(rows.SAMPLE.values)
    annot = rows.ANNOT.map(GENE_ROW_CLASSES).fillna(5).to_numpy(np.uint8)
    n = len(rows)
    return dict(gene=lookup[codes], sample=sample.astype(np.int32), annot=annot, cohort=np.full(n, int(cohort_id), np.int32),
                sample_names=list(sample_names))


PANEL_ROW_CLASSES = dict(GENE_ROW_CLASSES, Noncoding=6)                                                  # anything else: 5


def encode_panel_rows(f_mut, labels, cohort_id=0):
    """The rows of a cohort file as engine.panel_counts takes them: every row of read_mutation_file(f_mut, drop_duplicates=True) --
    autosomes only, one row per (mutation, sample), then get_unique_indels -- i.e. the rows CohortRun.panel_scale and
    DigPretrain.py countMutations start from, before the blacklist and the class filter (the pandas route: the native parser carries
    no annotation class).
    labels: the gene table (L labels, the union of the panels asked for).  Returns dict(label i32: the GENE's place in `labels`, L for
    a gene in none of them; sample i32: dense ids in order of first appearance; annot u8: PANEL_ROW_CLASSES, 5 for any other label;
    cohort i32; sample_names).  ValueError naming the file when it has no GENE / ANNOT columns, and for a row without a SAMPLE label."""
    import pandas as pd
    rows = mutation_tools.read_mutation_file(f_mut, drop_duplicates=False, unique_indels=False)
    if 'GENE' not in rows.columns or 'ANNOT' not in rows.columns:
        raise ValueError("{}: no GENE / ANNOT columns (an annotated mutation file has 8 or more)".format(f_mut))
    rows = mutation_tools.get_unique_indels(mutation_tools.drop_duplicate_mutations(rows))      # (what drop_duplicates=True does)
    if rows.SAMPLE.isna().any():
        raise ValueError("{}: a row without a SAMPLE label".format(f_mut))
    labels = list(labels)
    L = len(labels)
    place = {name: i for i, name in enumerate(labels)}
    codes, uniq = pd.factorize(rows.GENE.values)
    lookup = np.array([place.get(u, L) for u in uniq] + [L], np.int32)                                  # (a missing label: code -1)
    sample, sample_names = pd.factorize(rows.SAMPLE.values)
    annot = rows.ANNOT.map(PANEL_ROW_CLASSES).fillna(5).to_numpy(np.uint8)
    return dict(label=lookup[codes], sample=sample.astype(np.int32), annot=annot, cohort=np.full(len(rows), int(cohort_id), np.int32),
                sample_names=list(sample_names))


def _encode_mutation_file_native(path, cohort_id):
    """encode_mutation_file through the library's parser (dig_mutation_file_*_host, include/dig_hip.h): the same arrays, no
    interpreter lock held while a file is parsed -- 37 files side by side: 0.83 s -> 0.1 s on the 256 cores of the GPU box.
    None when the file holds something the parser leaves to the Python path (quotes, ragged rows, non-integer coordinates)."""
    import ctypes
    import os
    from .. import _lib
    h, n, ns, nb = ctypes.c_void_p(), ctypes.c_int64(-1), ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.call("dig_mutation_file_parse_host", os.fsencode(path), ctypes.byref(h), ctypes.byref(n), ctypes.byref(ns), ctypes.byref(nb))
    if n.value < 0:
        return None
    try:
        cols = [np.empty(n.value, np.int64) for _ in range(9)]
        names = ctypes.create_string_buffer(max(1, nb.value))
        _lib.call("dig_mutation_file_fetch_host", h, *[c.ctypes.data for c in cols[:7]], names)
        _lib.call("dig_mutation_file_flags_host", h, cols[7].ctypes.data, cols[8].ctypes.data)
    finally:
        _lib.call("dig_mutation_file_free_host", h)
    sample_names = names.raw[:nb.value].decode().split("\n") if ns.value else []
    ch, start, end, uid, samp, indel, gene, first_row, first_indel = cols
    return dict(chrom=ch, start=start, end=end, uid=uid, sample=samp, indel=indel, gene=gene, first_row=first_row,
                first_indel=first_indel, cohort=np.full(n.value, int(cohort_id), np.int64), sample_names=sample_names)


def encode_mutation_file(path, cohort_id=0, native=True):
    """An annotated mutation file (tab-separated, no header; GENE and ANNOT in columns 6 and 7: the reference's 8-, 10- and
    11-column schemas, mutation_tools.py:56-78) -> the host arrays of encode_mutations_host, without a pandas frame in between.
    Three routes, tried in this order, that give the same arrays on the files all of them take:
      * the library's own parser (`native`; it leaves quotes, ragged rows, non-integer coordinates, other column counts and
        label fields that pandas reads as missing -- '', 'NA', 'nan', 'NULL', ... -- to the next routes);
      * pyarrow's multi-threaded reader + dictionary encoding (0.12 s per 300 000 rows; leaves the same files to pandas);
      * pandas, with the reference's schema for the file's column count (what read_mutation_file does: the fall-back that
        defines the semantics -- missing labels are NaN, a row whose SAMPLE is missing is dropped as the reference's groupby does).
    Chromosome labels '1' ... '22', ONE leading 'chr' allowed, in every route."""
    if native:
        enc = _encode_mutation_file_native(path, cohort_id)
        if enc is not None:
            return enc

    def pandas_route():
        from . import mutation_tools
        try:
            df = mutation_tools.read_mutation_file(path, drop_sex=False, drop_duplicates=False, unique_indels=False)
        except StopIteration:                    # (the reference's next(reader) on an empty file)
            raise ValueError("%s: no rows (an annotated mutation file has 7 or more tab-separated columns, mutation_tools.py:45-104)" % path) from None
        if 'ANNOT' not in df.columns:
            raise ValueError("%s: an annotated mutation file has an ANNOT column (7 or more columns, mutation_tools.py:45-104)" % path)
        return encode_mutations_host(df, cohort_id)

    try:
        import pyarrow as pa
        import pyarrow.csv as pcsv
    except ImportError:
        return pandas_route()
    names = ['CHROM', 'START', 'END', 'REF', 'ALT', 'SAMPLE', 'GENE', 'ANNOT']
    with open(path, 'rb') as f:
        n_cols = f.readline().count(b"\t") + 1
    if n_cols not in (8, 10, 11):
        return pandas_route()
    all_names = names + ['X%d' % i for i in range(n_cols - 8)]
    text = {k: pa.string() for k in ('CHROM', 'REF', 'ALT', 'SAMPLE', 'GENE', 'ANNOT')}
    try:
        tb = pcsv.read_csv(path, read_options=pcsv.ReadOptions(column_names=all_names, use_threads=True, block_size=8 << 20),
                           parse_options=pcsv.ParseOptions(delimiter="\t"),
                           convert_options=pcsv.ConvertOptions(column_types=dict(text, START=pa.int64(), END=pa.int64()), include_columns=names,
                                                               strings_can_be_null=False))
    except pa.ArrowInvalid:                      # a header line, a coordinate that is not an integer: pandas says what it says
        return pandas_route()

    def ids(col):
        d = tb[col].combine_chunks().dictionary_encode()
        return d.indices.to_numpy(zero_copy_only=False).astype(np.int64), d.dictionary.to_pylist()
    ch_idx, ch_labels = ids('CHROM')
    label_to_int = np.array([int(_strip_chr(l)) if _strip_chr(l) in _AUTOSOME_LABELS else -1 for l in ch_labels] or [-1], np.int64)
    ch = label_to_int[ch_idx] if len(ch_idx) else np.zeros(0, np.int64)
    keep = ch > 0
    ref_id, ref_labels = ids('REF')
    alt_id, alt_labels = ids('ALT')
    samp, sample_labels = ids('SAMPLE')
    gene, gene_labels = ids('GENE')
    annot_idx, annot_labels = ids('ANNOT')
    if any(l in _PANDAS_NA for labels in (ref_labels, alt_labels, sample_labels, gene_labels, annot_labels) for l in labels):
        return pandas_route()                    # pandas reads such a label as missing
    indel = (np.array([l == 'INDEL' for l in annot_labels] or [False])[annot_idx]) if len(annot_idx) else np.zeros(0, bool)
    start = tb['START'].combine_chunks().to_numpy(zero_copy_only=False)
    end = tb['END'].combine_chunks().to_numpy(zero_copy_only=False)
    # sample ids in order of first appearance among the kept rows (what pandas.factorize gives encode_mutations_host)
    samp_k = samp[keep]
    first = np.full(len(sample_labels), np.iinfo(np.int64).max, np.int64)
    np.minimum.at(first, samp_k, np.arange(len(samp_k)))
    order = np.argsort(first, kind="stable")
    order = order[first[order] < np.iinfo(np.int64).max]
    remap = np.full(len(sample_labels), -1, np.int64)
    remap[order] = np.arange(len(order))
    return _host_record(ch[keep], start[keep], end[keep], ref_id[keep], alt_id[keep], remap[samp_k], [sample_labels[i] for i in order],
                        gene[keep], indel[keep], cohort_id)


_AUTOSOME_LABELS = frozenset(str(i) for i in range(1, 23))
# what pandas.read_csv reads as a missing value (its default na_values)
_PANDAS_NA = frozenset(["", "#N/A", "#N/A N/A", "#NA", "-1.#IND", "-1.#QNAN", "-NaN", "-nan", "1.#IND", "1.#QNAN", "<NA>", "N/A", "NA",
                        "NULL", "NaN", "None", "n/a", "nan", "null"])


def _strip_chr(label):
    """ONE leading 'chr' off a chromosome label (the rule of the native parser's autosome())."""
    return label[3:] if label.startswith("chr") else label


def to_device(enc, device):
    """Host arrays of encode_mutations_host / encode_mutation_file -> device tensors (int64, as the join and the tabulation take
    them).  The upload is narrow -- ids and coordinates that fit 32 bits travel as int32, the three flags as bytes, the constant
    cohort column not at all -- and widened on the device: 31 instead of 88 bytes per row over PCIe from pageable memory."""
    import torch
    out = {}
    n = len(enc["chrom"])
    for k, v in enc.items():
        if k == "sample_names":
            continue
        v = np.asarray(v)
        if k == "cohort":
            out[k] = torch.full((n,), int(v[0]) if n else 0, dtype=torch.int64, device=device)
        elif k in ("indel", "first_row", "first_indel"):
            out[k] = torch.as_tensor(v.astype(np.uint8), device=device).long()
        elif n and v.dtype.kind in "iu" and int(v.min()) >= -2 ** 31 and int(v.max()) < 2 ** 31:
            out[k] = torch.as_tensor(v.astype(np.int32), device=device).long()
        else:
            out[k] = torch.as_tensor(v, device=device)
    out["sample_names"] = list(enc["sample_names"])
    return out


def encode_mutations(df_mut, device, cohort_id=0, chrom_ids=None):
    """Mutation frame (reference column names) -> device tensors (encode_mutations_host + to_device)."""
    return to_device(encode_mutations_host(df_mut, cohort_id, chrom_ids), device)


def tabulate_cohorts(blocks, cohorts, drop_duplicates=True, max_muts_per_sample=1e9, max_muts_per_elt_per_sample=3e9,
                     return_sample_keys=False):
    """`cohorts`: list of encode_mutations() dicts (one per cohort).  Returns (OBS_SNV, OBS_SAMPLES, OBS_INDEL) int32
    [E, C] device tensors and the per-cohort lists of blacklisted sample names.
    return_sample_keys: a fifth value, dict(keys: int64 [K, 3] device tensor, one distinct (cohort, element, sample) row per kept
    sample of an element -- the rows OBS_SAMPLES counts --, the sample numbered 0 .. n - 1 within its cohort over the samples that
    were not blacklisted; n_samples: host int64 [C], that n per cohort)."""
    import torch
    dev = blocks.device
    C, E = len(cohorts), blocks.n_elements
    # sample and mutation ids are per cohort: make them globally distinct with an offset
    offs = cohort_rows.sample_offsets(cohorts)
    sample = cohort_rows.column(cohorts, "sample", shift=offs)
    uid = cohort_rows.column(cohorts, "uid", shift=cohort_rows.id_offsets(cohorts, "uid"))
    chrom, start, end, indel, cohort = (cohort_rows.column(cohorts, k) for k in ("chrom", "start", "end", "indel", "cohort"))
    pm, pb = overlap_pairs(blocks, chrom, start, end)
    pm = pm.long()
    elt = blocks.elt[pb.long()]
    rec = torch.stack([cohort[pm], elt, sample[pm], uid[pm], indel[pm]], dim=1)        # [n_pairs, 5]
    if drop_duplicates and rec.shape[0]:
        # duplicates on (chrom, start, end, ref, alt, sample, element): ANNOT is a function of the mutation here
        rec = _unique_rows_keep_flag(rec)
    # per (cohort, element, sample): SNV and INDEL counts
    key3, inv = torch.unique(rec[:, :3], dim=0, return_inverse=True)
    n3 = key3.shape[0]
    snv = torch.zeros(n3, dtype=torch.int64, device=dev).index_add_(0, inv, 1 - rec[:, 4])
    ind = torch.zeros(n3, dtype=torch.int64, device=dev).index_add_(0, inv, rec[:, 4])
    # hypermutator blacklist per (cohort, sample): total over elements of OBS_MUT
    n_samp_tot = int(offs[-1])
    tot = torch.zeros(max(n_samp_tot, 1), dtype=torch.int64, device=dev).index_add_(0, key3[:, 2], snv + ind)
    black = tot > max_muts_per_sample
    keep = ~black[key3[:, 2]]
    key3, snv, ind = key3[keep], snv[keep], ind[keep]
    cap = int(min(max_muts_per_elt_per_sample, 2 ** 62))
    snv, ind = snv.clamp(max=cap), ind.clamp(max=cap)
    flat = key3[:, 1] * C + key3[:, 0]                                                  # [E, C] layout
    z = lambda: torch.zeros(E * C, dtype=torch.int64, device=dev)
    obs_snv = z().index_add_(0, flat, snv).view(E, C).to(torch.int32)
    obs_ind = z().index_add_(0, flat, ind).view(E, C).to(torch.int32)
    obs_smp = z().index_add_(0, flat, torch.ones_like(snv)).view(E, C).to(torch.int32)
    black_np = black.cpu().numpy()
    blacklists = [[n for j, n in enumerate(c["sample_names"]) if black_np[int(o) + j]] for c, o in zip(cohorts, offs[:-1])]
    if return_sample_keys:
        kept = np.concatenate([[0], np.cumsum(~black_np[:n_samp_tot])])                  # kept samples in front of every global sample
        first = torch.as_tensor(kept[np.asarray(offs[:-1], np.int64)], device=dev)      # ... in front of every cohort
        local = torch.as_tensor(kept[:-1], device=dev)[key3[:, 2]] - first[key3[:, 0]] if n3 else key3[:, 2]
        keys = torch.stack([key3[:, 0], key3[:, 1], local], dim=1)
        return obs_snv, obs_smp, obs_ind, blacklists, dict(keys=keys, n_samples=np.diff(kept[np.asarray(offs, np.int64)]))
    return obs_snv, obs_smp, obs_ind, blacklists


def _unique_rows_keep_flag(rec):
    """Unique on the first four columns (cohort, element, sample, mutation uid), keeping the indel flag of the
    first occurrence (identical for all occurrences: the flag is a property of the mutation)."""
    import torch
    key, inv = torch.unique(rec[:, :4], dim=0, return_inverse=True)
    flag = torch.zeros(key.shape[0], dtype=rec.dtype, device=rec.device)
    flag.scatter_reduce_(0, inv, rec[:, 4], reduce="amax", include_self=True)
    return torch.cat([key, flag[:, None]], dim=1)
