"""Mutation-file handling and integer observed-count tabulation.

Host mirror of DIGDriver/data_tools/mutation_tools.py.  Same function names, arguments and output
frames; the reference shells out to ``bedtools intersect`` through pybedtools, here the interval
join is a sort + binary-search in numpy (half-open ``[START, END)`` overlap, exactly bedtools'
default: two intervals overlap when ``a.start < b.end and b.start < a.end``; zero-length features
are treated like bedtools does, as overlapping when ``b.start <= a.start < b.end``... see
``_overlap_pairs``).  All outputs of this module are integer counts and must be bit-exact.
"""
import csv
import gzip

import numpy as np
import pandas as pd

_MUT_COLS = {
    5: ['CHROM', 'POS', 'REF', 'ALT', 'SAMPLE'],
    6: ['CHROM', 'START', 'END', 'REF', 'ALT', 'SAMPLE'],
    7: ['CHROM', 'START', 'END', 'REF', 'ALT', 'SAMPLE', 'ANNOT'],
    8: ['CHROM', 'START', 'END', 'REF', 'ALT', 'SAMPLE', 'GENE', 'ANNOT'],
    9: ['CHROM', 'START', 'END', 'REF', 'ALT', 'SAMPLE', 'ANNOT', 'MUT_TYPE', 'CONTEXT'],
    10: ['CHROM', 'START', 'END', 'REF', 'ALT', 'SAMPLE', 'GENE', 'ANNOT', 'MUT_TYPE', 'CONTEXT'],
    11: ['CHROM', 'START', 'END', 'REF', 'ALT', 'SAMPLE', 'GENE', 'ANNOT', 'MUT_TYPE', 'CONTEXT', 'STRAND'],
}
_INT_COLS = ('POS', 'START', 'END')
_AUTOSOMES = [str(i) for i in range(1, 23)]


_MUT_KEY = ['CHROM', 'START', 'END', 'REF', 'ALT']


def _first_row_width(path):
    """Number of tab-separated fields of the first row of a plain or gzip file."""
    for opener in (open, lambda q: gzip.open(q, 'rt')):
        try:
            with opener(path) as handle:
                return len(next(csv.reader(handle, delimiter='\t', skipinitialspace=True)))
        except UnicodeDecodeError:
            continue
    raise ValueError("cannot read {}".format(path))


def read_mutation_file(path, drop_sex=True, drop_duplicates=False, unique_indels=True):
    """mutation_tools.py:45-104: header-less TSV whose schema follows from its column count (5 ... 11), plain or gzip;
    optionally autosomes only (CHROM becomes int), unique rows, unique indels."""
    names = _MUT_COLS[_first_row_width(path)]
    rows = pd.read_csv(path, sep="\t", names=names, low_memory=False, dtype={c: (int if c in _INT_COLS else str) for c in names})
    if drop_sex:
        autosomal = rows.CHROM.isin(_AUTOSOMES)
        if not autosomal.all():
            print('Restricting to autosomes')
            rows = rows.loc[autosomal]
        rows = rows.assign(CHROM=rows.CHROM.astype(int))
    if drop_duplicates:
        rows = drop_duplicate_mutations(rows)
    return get_unique_indels(rows) if unique_indels else rows


def drop_duplicate_mutations(df_mut):
    """mutation_tools.py:107-109: one row per (mutation, sample)."""
    return df_mut.drop_duplicates(_MUT_KEY + ['SAMPLE'])


def get_unique_indels(df_mut):
    """mutation_tools.py:111-117: an indel seen in several samples is kept once per GENE label; SNV rows come first."""
    indel = df_mut.ANNOT == 'INDEL'
    return pd.concat([df_mut.loc[~indel], df_mut.loc[indel].drop_duplicates(subset=_MUT_KEY + ['GENE'])])


def filter_hypermut_samples(df_mut, max_muts_per_sample, return_blacklist=False):
    """mutation_tools.py:293-304: drop every row of the samples with more than `max_muts_per_sample` rows."""
    load = df_mut.SAMPLE.value_counts()
    hyper = load.index[load > max_muts_per_sample].to_list()
    kept = df_mut.loc[~df_mut.SAMPLE.isin(hyper)]
    return (kept, hyper) if return_blacklist else kept


_ANNOT_TO_OBS = {'Missense': 'OBS_MIS', 'Nonsense': 'OBS_NONS', 'Synonymous': 'OBS_SYN', 'Essential_Splice': 'OBS_SPL',
                 'INDEL': 'OBS_INDEL'}


def mutations_per_gene(df_mut_cds, max_muts_per_gene_per_sample=3e9):
    """mutation_tools.py:329-361: rows per (GENE, SAMPLE, ANNOT), capped per sample, summed per (GENE, ANNOT) -> integer
    frame indexed by GENE with one column per annotation class present, the five tested classes named OBS_* (0 when the
    cohort has none)."""
    per_sample = df_mut_cds.groupby(['GENE', 'SAMPLE', 'ANNOT']).size().clip(upper=max_muts_per_gene_per_sample)
    table = per_sample.groupby(level=['GENE', 'ANNOT']).sum().unstack('ANNOT').fillna(0).astype(int)
    table.columns = table.columns.to_list()
    for annot in _ANNOT_TO_OBS:
        if annot not in table.columns:
            table[annot] = 0
    return table.rename(columns=_ANNOT_TO_OBS)


def bed12_boundaries(f_bed):
    """mutation_tools.py:383-414: bed12 -> frame (CHROM int, ELT, STRAND, BLOCK_STARTS, BLOCK_ENDS), autosomes only.
    As in the reference the 'chr' prefix is stripped only when the FIRST row carries it."""
    names = ['CHROM', 'START', 'END', "ELT", "SCORE", "STRAND", 'thickStart', 'thickEnd', 'rgb', 'blockCount',
             'blockSizes', 'blockStarts']
    df = pd.read_table(f_bed, names=names, low_memory=False)
    df.CHROM = df.CHROM.astype(str)
    df.blockSizes = df.blockSizes.astype(str)
    df.blockStarts = df.blockStarts.astype(str)
    if 'chr' in str(df['CHROM'][0]):
        df['CHROM'] = df['CHROM'].map(lambda x: x.lstrip('chr'))
    df = df[df.CHROM.isin(_AUTOSOMES)].copy()
    df.CHROM = df.CHROM.astype(int)

    def _ints(s):
        return [int(x) for x in s.rstrip(',').split(',')]

    starts = [[x + st for x in _ints(bs)] for bs, st in zip(df.blockStarts, df.START)]
    ends = [[s + z for s, z in zip(ss, _ints(bz))] for ss, bz in zip(starts, df.blockSizes)]
    df['BLOCK_STARTS'] = starts
    df['BLOCK_ENDS'] = ends
    return df[['CHROM', 'ELT', 'STRAND', 'BLOCK_STARTS', 'BLOCK_ENDS']]


# ---------------------------------------------------------------------------------------------
# interval join (replaces `bedtools intersect -wa -wb` on mutations x bed6 blocks)
# ---------------------------------------------------------------------------------------------
def _chrom_key(chrom):
    """Chromosome labels compare as text in bedtools: '1' and 'chr1' are different chromosomes."""
    return np.asarray(chrom).astype(str)


def _overlap_pairs(m_chrom, m_start, m_end, b_chrom, b_start, b_end):
    """All (mutation row, block row) pairs with bedtools-intersect semantics:
    overlap iff  m.start < b.end  and  b.start < m.end  (half-open).  A zero-length mutation
    (start == end, bedtools >= 2.27) overlaps block b iff  b.start <= m.start < b.end ... bedtools treats
    it as the 1-bp feature [start, start+1) for the test; the same is done for zero-length blocks.
    Output order: mutation-major (file order of the mutation file), blocks in bed order."""
    m_chrom, b_chrom = _chrom_key(m_chrom), _chrom_key(b_chrom)
    m_start = np.asarray(m_start, np.int64)
    m_end = np.asarray(m_end, np.int64)
    b_start = np.asarray(b_start, np.int64)
    b_end = np.asarray(b_end, np.int64)
    m_end_eff = np.where(m_end == m_start, m_start + 1, m_end)
    b_end_eff = np.where(b_end == b_start, b_start + 1, b_end)
    mi_all, bi_all = [], []
    for ch in np.unique(b_chrom):
        bsel = np.nonzero(b_chrom == ch)[0]
        msel = np.nonzero(m_chrom == ch)[0]
        if len(bsel) == 0 or len(msel) == 0:
            continue
        order = np.argsort(b_start[bsel], kind="stable")
        bs, be, bidx = b_start[bsel][order], b_end_eff[bsel][order], bsel[order]
        # blocks may overlap/nest: candidates are all blocks with start < m.end; filter by end > m.start.
        # running max of block ends bounds the scan from the left
        run_max = np.maximum.accumulate(be)
        hi = np.searchsorted(bs, m_end_eff[msel], side="left")        # blocks [0, hi) have start < m.end
        lo = np.searchsorted(run_max, m_start[msel], side="right")     # first block whose running max end > m.start
        cnt = np.maximum(hi - lo, 0)
        tot = int(cnt.sum())
        if tot == 0:
            continue
        rep_m = np.repeat(np.arange(len(msel)), cnt)
        offs = np.arange(tot) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        cand = np.repeat(lo, cnt) + offs
        keep = be[cand] > m_start[msel][rep_m]
        mi_all.append(msel[rep_m[keep]])
        bi_all.append(bidx[cand[keep]])
    if not mi_all:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    mi = np.concatenate(mi_all)
    bi = np.concatenate(bi_all)
    order = np.lexsort((bi, mi))
    return mi[order], bi[order]


def _bed12_to_bed6(df_bed12):
    """bedtools bed12tobed6: one row per block, keeping the parent's name and strand."""
    cols = ['CHROM', 'START', 'END', 'ELT', 'STRAND']
    if len(df_bed12) and df_bed12[10].dtype == object and df_bed12[11].dtype == object:
        # the usual file -- both lists of every row with, or of every row without, the trailing comma -- by array operations: the
        # lists joined into one text and read as numbers in one call (0.13 -> 0.04 s per 120 000 elements)
        try:
            a, b = df_bed12[10].values.astype(str), df_bed12[11].values.astype(str)
            ta, tb = np.char.endswith(a, ','), np.char.endswith(b, ',')
            if (ta.all() or not ta.any()) and (tb.all() or not tb.any()):
                n = np.char.count(a, ',') + (0 if ta.all() else 1)
                if np.array_equal(n, np.char.count(b, ',') + (0 if tb.all() else 1)) and (n > 0).all():
                    sizes = np.fromstring(('' if ta.all() else ',').join(a.tolist()), dtype=np.int64, sep=',')
                    starts = np.fromstring(('' if tb.all() else ',').join(b.tolist()), dtype=np.int64, sep=',')
                    if len(sizes) == len(starts) == int(n.sum()):
                        rep = np.repeat(np.arange(len(a)), n)
                        s0 = np.asarray(df_bed12[1].values, np.int64)[rep] + starts
                        return pd.DataFrame({'CHROM': df_bed12[0].values[rep], 'START': s0, 'END': s0 + sizes,
                                             'ELT': df_bed12[3].values[rep], 'STRAND': df_bed12[5].values[rep]}, columns=cols)
        except (ValueError, TypeError):
            pass                                   # (anything unusual in the lists: the row-by-row forms below)
    bsz = [str(x).rstrip(',') for x in df_bed12[10]]
    bst = [str(x).rstrip(',') for x in df_bed12[11]]
    n = np.fromiter((x.count(',') + 1 for x in bsz), np.int64, len(bsz))
    if len(bsz) and np.array_equal(n, np.fromiter((x.count(',') + 1 for x in bst), np.int64, len(bst))):
        # all rows at once (a Python loop over the blocks of 120 000 elements was 0.3 s of a command-line run)
        sizes = np.array(",".join(bsz).split(','), dtype=np.int64)
        starts = np.array(",".join(bst).split(','), dtype=np.int64)
        rep = np.repeat(np.arange(len(bsz)), n)
        s0 = np.asarray(df_bed12[1].values, np.int64)[rep] + starts
        return pd.DataFrame({'CHROM': df_bed12[0].values[rep], 'START': s0, 'END': s0 + sizes, 'ELT': df_bed12[3].values[rep],
                             'STRAND': df_bed12[5].values[rep]}, columns=cols)
    rows = []                                      # (rows whose two lists differ in length: block by block, the shorter list counts)
    for chrom, start, name, strand, z_, s_ in zip(df_bed12[0], df_bed12[1], df_bed12[3], df_bed12[5], bsz, bst):
        for s, z in zip([int(x) for x in s_.split(',')], [int(x) for x in z_.split(',')]):
            rows.append((chrom, start + s, start + s + z, name, strand))
    return pd.DataFrame(rows, columns=cols)


def tabulate_muts_per_sample_per_element(f_mut, f_elt_bed, bed12=False, drop_duplicates=False, unique_indels=True):
    """mutation_tools.py:191-230: mutations x element blocks -> per (ELT, SAMPLE) integer counts
    OBS_SNV / OBS_INDEL / OBS_MUT.  The raw file rows are joined (no autosome filter), duplicates on
    (chrom, start, end, ref, alt, sample, elt) dropped when asked (:208), SNV vs INDEL by ANNOT (:211-213)."""
    muts = pd.read_csv(f_mut, sep="\t", header=None, low_memory=False, dtype={0: str})
    bed = pd.read_csv(f_elt_bed, sep="\t", header=None, low_memory=False, dtype={0: str})
    blocks = _bed12_to_bed6(bed) if bed12 else bed.rename(columns={0: 'CHROM', 1: 'START', 2: 'END', 3: 'ELT'})
    mi, bi = _overlap_pairs(muts[0].values, muts[1].values, muts[2].values, blocks.CHROM.values, blocks.START.values,
                            blocks.END.values)
    out_cols = ['ELT', 'SAMPLE', 'OBS_SNV', 'OBS_INDEL', 'OBS_MUT']
    if len(mi) == 0:
        return pd.DataFrame({c: [] for c in out_cols})
    hits = pd.DataFrame({'ELT': blocks.ELT.values[bi], 'SAMPLE': muts[5].values[mi],
                         'KIND': np.where(muts[7].values[mi] == 'INDEL', 'OBS_INDEL', 'OBS_SNV')})
    if drop_duplicates:
        ident = muts.iloc[mi, :5].reset_index(drop=True)
        hits = hits.loc[~pd.concat([ident, hits[['SAMPLE', 'ELT']]], axis=1).duplicated().values]
    # counts per (element, sample): the SNV table outer-joined with the INDEL table on (ELT, SAMPLE) (:219-222) -- the
    # row order of the result is pandas' (key-sorted since pandas 2.2, SNV pairs first before)
    snv = hits.loc[hits.KIND == 'OBS_SNV'].groupby(['ELT', 'SAMPLE']).size().reset_index(name='OBS_SNV')
    ind = hits.loc[hits.KIND == 'OBS_INDEL'].groupby(['ELT', 'SAMPLE']).size().reset_index(name='OBS_INDEL')
    wide = snv.merge(ind, how='outer').fillna({'OBS_SNV': 0.0, 'OBS_INDEL': 0.0})
    wide['OBS_MUT'] = wide.OBS_SNV + wide.OBS_INDEL
    return wide[out_cols].rename_axis(columns=None)


def _summary_by_codes(f_mut, f_elt_bed, bed12, drop_duplicates, max_muts_per_sample, max_muts_per_elt_per_sample):
    """The per-element summary and the blacklist of tabulate_mutations_in_element WITHOUT the per-(element, sample) frame of
    strings in between: the joined rows carry integer codes of element and sample, the pair counts are one np.unique + two
    bincounts, names come back at the end (the group-by / merge chain over 200 000 string pairs was 0.25 s of a one-cohort
    command line).  The same table, dtypes, row order (elements by name) and blacklist as the frame route below
    (tests/test_host_tabulate.py); None when there is nothing to count (the caller's frame route handles the empty shapes)."""
    muts = pd.read_csv(f_mut, sep="\t", header=None, low_memory=False, dtype={0: str}, usecols=[0, 1, 2, 3, 4, 5, 7])
    bed = pd.read_csv(f_elt_bed, sep="\t", header=None, low_memory=False, dtype={0: str})
    blocks = _bed12_to_bed6(bed) if bed12 else bed.rename(columns={0: 'CHROM', 1: 'START', 2: 'END', 3: 'ELT'})
    mi, bi = _overlap_pairs(muts[0].values, muts[1].values, muts[2].values, blocks.CHROM.values, blocks.START.values,
                            blocks.END.values)
    if len(mi) == 0:
        return None
    ecode, enames = pd.factorize(blocks.ELT.values[bi])
    scode, snames = pd.factorize(muts[5].values[mi])
    indel = muts[7].values[mi] == 'INDEL'
    if drop_duplicates:                              # (chrom, start, end, ref, alt, sample, element), first occurrence kept (:208)
        ident = pd.DataFrame({0: muts[0].values[mi], 1: muts[1].values[mi], 2: muts[2].values[mi], 3: muts[3].values[mi],
                              4: muts[4].values[mi], 5: scode, 6: ecode})
        keep = ~ident.duplicated().values
        ecode, scode, indel = ecode[keep], scode[keep], indel[keep]
    ns, ne = len(snames), len(enames)
    pairs, inv = np.unique(ecode.astype(np.int64) * ns + scode, return_inverse=True)
    ind = np.bincount(inv, weights=indel, minlength=len(pairs))
    snv = np.bincount(inv, weights=~indel, minlength=len(pairs))
    pe, ps = pairs // ns, pairs % ns
    load = np.bincount(ps, weights=snv + ind, minlength=ns)
    black = load > max_muts_per_sample
    blacklist = pd.Index(np.sort(np.asarray(snames, dtype=object)[black]), name='SAMPLE')
    ok = ~black[ps]
    pe, snv, ind = pe[ok], np.minimum(snv[ok], max_muts_per_elt_per_sample), np.minimum(ind[ok], max_muts_per_elt_per_sample)
    if len(pe) == 0:
        return None
    n_pairs = np.bincount(pe, minlength=ne)
    present = np.nonzero(n_pairs)[0]
    names = np.asarray(enames)[present]                  # (numeric names stay numbers, as in the group-by's index)
    if names.dtype == object and all(type(x) is str for x in names):
        order = np.argsort(names.astype(str), kind="stable")          # (code-point order = Python's string order = the group-by's)
    else:
        order = np.argsort(names, kind="stable")
    present = present[order]
    summary = pd.DataFrame({'OBS_INDEL': np.bincount(pe, weights=ind, minlength=ne)[present],
                            'OBS_SAMPLES': n_pairs[present].astype(np.int64),
                            'OBS_SNV': np.bincount(pe, weights=snv, minlength=ne)[present]},
                           index=pd.Index(names[order], name='ELT'))
    return summary, blacklist


def tabulate_mutations_in_element(f_mut, f_elt_bed, bed12=False, drop_duplicates=False, all_elements=False,
                                  max_muts_per_sample=1e9, max_muts_per_elt_per_sample=3e9, return_blacklist=False):
    """mutation_tools.py:155-189: hypermutator blacklist, per-(element, sample) cap, then per-element
    OBS_SAMPLES (= number of distinct samples), OBS_SNV, OBS_INDEL."""
    fast = None
    try:
        fast = _summary_by_codes(f_mut, f_elt_bed, bed12, drop_duplicates, max_muts_per_sample, max_muts_per_elt_per_sample)
    except (ValueError, TypeError, KeyError):            # (an unusual file -- fewer columns, mixed types: the frame route decides)
        fast = None
    if fast is not None:
        summary, blacklist = fast
    else:
        per_pair = tabulate_muts_per_sample_per_element(f_mut, f_elt_bed, bed12=bed12, drop_duplicates=drop_duplicates)
        blacklist = []
        if len(per_pair):
            load = per_pair.groupby('SAMPLE').OBS_MUT.sum()
            blacklist = load.index[load > max_muts_per_sample]
            per_pair = per_pair.loc[~per_pair.SAMPLE.isin(blacklist)]
        capped = per_pair.assign(OBS_SNV=per_pair.OBS_SNV.clip(upper=max_muts_per_elt_per_sample),
                                 OBS_INDEL=per_pair.OBS_INDEL.clip(upper=max_muts_per_elt_per_sample))
        if len(capped):
            summary = capped.groupby('ELT').agg(OBS_INDEL=('OBS_INDEL', 'sum'), OBS_SAMPLES=('SAMPLE', 'size'), OBS_SNV=('OBS_SNV', 'sum'))        # ('size' = the reference's len per group, without a Python call per element: 0.5 s of a 120 000-element run)
        else:
            summary = pd.DataFrame({'OBS_SAMPLES': [], 'OBS_SNV': [], 'OBS_INDEL': [], 'ELT': []}).set_index('ELT')
    if all_elements:                                  # every element of the bed, zero counts included (:176-183)
        listed = pd.read_csv(f_elt_bed, sep="\t", header=None).set_index(3).rename_axis('ELT')
        summary = listed.merge(summary, left_index=True, right_index=True, how='left')
        summary[['OBS_SNV', 'OBS_INDEL', 'OBS_SAMPLES']] = summary[['OBS_SNV', 'OBS_INDEL', 'OBS_SAMPLES']].fillna(0)
    table = summary[['OBS_SAMPLES', 'OBS_SNV', 'OBS_INDEL']]
    return (table, blacklist) if return_blacklist else table


def restrict_mutations_by_bed_efficient(f_mut, f_bed, bed12=False, drop_duplicates=False, drop_sex=False,
                                        replace_cols=False):
    """mutation_tools.py:32-43: `bedtools intersect -wa`: one output row per (mutation, overlapped block) pair."""
    import os
    import tempfile
    df_raw = pd.read_csv(f_mut, sep="\t", header=None, low_memory=False, dtype=str)
    df_bed = pd.read_csv(f_bed, sep="\t", header=None, low_memory=False, dtype={0: str})
    blocks = _bed12_to_bed6(df_bed) if bed12 else df_bed.rename(columns={0: 'CHROM', 1: 'START', 2: 'END'})
    mi, _ = _overlap_pairs(df_raw[0].values, df_raw[1].astype(np.int64).values, df_raw[2].astype(np.int64).values,
                           blocks.CHROM.values, blocks.START.values, blocks.END.values)
    fd, tmp = tempfile.mkstemp(suffix=".tsv")
    os.close(fd)
    try:
        df_raw.iloc[mi].to_csv(tmp, sep="\t", header=False, index=False)
        if len(mi) == 0:
            cols = _MUT_COLS[df_raw.shape[1]]
            return pd.DataFrame({c: [] for c in cols})
        return read_mutation_file(tmp, drop_duplicates=drop_duplicates, drop_sex=drop_sex)
    finally:
        os.remove(tmp)


def restrict_mutations_by_bed(df_mut, df_bed, unique=True, remove_X=True, replace_cols=False):
    """mutation_tools.py:8-30 (frame-level `bedtools intersect`, reports the overlapping part of each mutation:
    for 1-bp SNVs inside a block that is the mutation itself)."""
    if remove_X:
        df_mut = df_mut[df_mut.iloc[:, 0] != "X"]
        df_bed = df_bed[df_bed.iloc[:, 0] != "X"]
    mi, bi = _overlap_pairs(df_mut.iloc[:, 0].values, df_mut.iloc[:, 1].values, df_mut.iloc[:, 2].values,
                            df_bed.iloc[:, 0].values, df_bed.iloc[:, 1].values, df_bed.iloc[:, 2].values)
    inter = df_mut.iloc[mi].copy()
    s = np.maximum(df_mut.iloc[mi, 1].values, df_bed.iloc[bi, 1].values)
    e = np.minimum(df_mut.iloc[mi, 2].values, df_bed.iloc[bi, 2].values)
    inter.iloc[:, 1] = s
    inter.iloc[:, 2] = np.maximum(e, s)
    if unique:
        inter = inter.drop_duplicates()
    return inter


# ---------------------------------------------------------------------------------------------
# sites route: mutations that hit listed (position, substitution) sites exactly
# ---------------------------------------------------------------------------------------------
_SITE_KEY = ['CHROM', 'START', 'END', 'REF', 'ALT', 'GENE', 'ANNOT', 'MUT_TYPE', 'CONTEXT']


def tabulate_nonc_mutations_at_sites(f_sites, f_mut, return_sites=False):
    """mutation_tools.py:232-276.  The sites file has the mutation-file layout with the element name in the SAMPLE
    column; a mutation counts for a site when the nine annotation columns agree.  Indels are dropped.  Per element:
    OBS_SAMPLES = distinct samples, OBS_SNV = matching rows."""
    df_sites = read_mutation_file(f_sites)
    df_sites = df_sites.rename({"SAMPLE": "ELT"}, axis=1)
    assert 'GENE' in df_sites.columns and 'ANNOT' in df_sites.columns and 'MUT_TYPE' in df_sites.columns
    if 'STRAND' not in df_sites.columns:
        print("WARNING: strand column not detected in sites file. Defaulting all sites to + strand.")
        df_sites['STRAND'] = "+"
    df_mut = read_mutation_file(f_mut, drop_duplicates=False)
    assert 'GENE' in df_mut.columns and 'ANNOT' in df_mut.columns and 'MUT_TYPE' in df_mut.columns
    if len(df_mut[df_mut.ANNOT == 'INDEL']):
        print('WARNING: INDELS found in mutation file. Dig sites model is only applicable to SNVs. INDELS will be dropped.')
    df_mut = df_mut[df_mut.ANNOT != 'INDEL']
    at_sites = df_mut.merge(df_sites, on=_SITE_KEY, how='inner')
    counts = at_sites.groupby('ELT').agg(OBS_SAMPLES=('SAMPLE', lambda x: len(set(x))), OBS_SNV=('CHROM', len)).reset_index()
    if return_sites:
        sites = df_sites.drop(columns=['GENE', 'ANNOT', 'REF', 'ALT']).rename(columns={'SAMPLE': 'GENE'})
        return counts, sites
    return counts


def tabulate_sites_in_element(f_sites, f_mut):
    """mutation_tools.py:279-283"""
    return tabulate_nonc_mutations_at_sites(f_sites, f_mut).set_index('ELT')[['OBS_SAMPLES', 'OBS_SNV']]


# ---------------------------------------------------------------------------------------------
# genic function of mutations (DigPreprocess.py addMutationFunction; reference: scripts/mutationFunction.R, which needs R,
# Bioconductor and dNdScv's refcds_hg19.rda) -- the gene table from a bed12 of coding exons, the CDS letters from the FASTA,
# the interval join by dig_overlap_join_* and the per-(mutation, gene) work by dig_mutation_function
# ---------------------------------------------------------------------------------------------
_MF_LABEL = ('Synonymous', 'Missense', 'Nonsense', 'Stop_loss', 'Essential_Splice')
_MF_CODE = "KNKNTTTTRSRSIIMI" "QHQHPPPPRRRRLLLL" "EDEDAAAAGGGGVVVV" "*Y*YSSSS*CWCLFLF"     # codon 16 b0 + 4 b1 + b2, A C G T = 0 1 2 3
_MF_COMP = {'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A'}


def read_raw_mutations(f_mut):
    """Steps 1-3 of the annotation rule: the raw call file (no header; tab separated when its first line holds a tab, else
    whitespace separated; 5 columns CHROM POS REF ALT SAMPLE, or 6 and more CHROM START END REF ALT SAMPLE ... with pos = START + 1,
    plain or gzip) -> frame CHROM, pos, REF, ALT, SAMPLE, start, end (1-based closed) in file order, without REF == ALT rows, rows with an
    empty field and later copies of (SAMPLE, CHROM, pos, REF, ALT)."""
    opener = gzip.open if f_mut.endswith('.gz') else open
    with opener(f_mut, 'rt') as handle:
        first = handle.readline()
    sep = "\t" if "\t" in first else r"\s+"
    width = len(first.rstrip("\r\n").split("\t") if sep == "\t" else first.split())
    if width < 5:
        raise ValueError("{}: {} columns; a raw mutation file has 5 (CHROM POS REF ALT SAMPLE) or 6 and more "
                         "(CHROM START END REF ALT SAMPLE ...)".format(f_mut, width))
    raw = pd.read_csv(f_mut, sep=sep, header=None, names=list(range(width)), dtype=str, keep_default_na=False, na_filter=False,
                      engine="c" if sep == "\t" else "python", skip_blank_lines=True)
    cols = [0, 1, 2, 3, 4] if width == 5 else [0, 1, 3, 4, 5]
    df = raw[cols].fillna('')                                           # (a row shorter than the first one: its missing fields are empty)
    df.columns = ['CHROM', 'pos', 'REF', 'ALT', 'SAMPLE']
    for c in df.columns:
        df[c] = df[c].str.strip()
    df = df[(df != '').all(axis=1) & (df.REF != df.ALT)]
    try:
        df = df.assign(pos=df.pos.astype(np.int64) + (0 if width == 5 else 1))
    except ValueError as exc:
        raise ValueError("{}: a position that is not an integer ({})".format(f_mut, exc))
    df = df.drop_duplicates(['SAMPLE', 'CHROM', 'pos', 'REF', 'ALT']).reset_index(drop=True)
    shift = (df.REF.str[:1] == df.ALT.str[:1]) & (df.REF.str.len() > df.ALT.str.len())     # a deletion written from the base in front
    return df.assign(start=df.pos + shift.astype(np.int64), end=df.pos + df.REF.str.len().astype(np.int64) - 1)


def _gene_range_join(r_chrom, r_start, r_end, m_chrom, m_start, m_end, on_device):
    """(mutation row, range row) pairs of the closed overlap of mutations and gene ranges (both 1-based closed, same chromosome
    label; ranges sorted by (chrom, start)): engine.overlap_join on the device or through the `_host` twins, as host int64 arrays."""
    from .. import engine
    from .._marshal import backend_on
    labels = {lab: i + 1 for i, lab in enumerate(dict.fromkeys(r_chrom.tolist()))}
    rc = np.array([labels[c] for c in r_chrom.tolist()], np.int64)
    codes, uniq = pd.factorize(m_chrom)
    mc = np.array([labels.get(u, 0) for u in uniq], np.int64)[codes] if len(codes) else np.zeros(0, np.int64)
    # half-open, 0-based (the ranges are sorted already: join_blocks keeps their order, a block row is a range row)
    _, start_key, runmax_key, blk_end = engine.join_blocks(rc, np.asarray(r_start, np.int64) - 1, r_end)
    pm, pb = engine.overlap_join(backend_on(0, on_device), start_key, runmax_key, blk_end, mc, np.asarray(m_start, np.int64) - 1, m_end)
    if on_device:
        pm, pb = pm.cpu().numpy(), pb.cpu().numpy()
    return pm.astype(np.int64), pb.astype(np.int64)


def _snv_function_from_letters(genome, genes, gene_chrom, g, pos, ref, alt):
    """(impact, wrong_ref) of one SNV pair the kernel left to the host (DIG_MF_HOST: the base or its codon holds a letter other
    than ACGT), from PackedGenome's letters: a codon with such a letter translates to X, as seqinr::translate does."""
    ci = int(gene_chrom[g])
    letter = lambda p: genome.letters(ci, p - 1, p).decode('ascii')
    minus = bool(genes.minus[g])
    wrong = letter(pos) != ref
    spl = genes.spl_pos[genes.spl_ptr[g]:genes.spl_ptr[g + 1]]
    if (spl == pos).any():
        return 4, wrong
    b0, b1 = int(genes.blk_ptr[g]), int(genes.blk_ptr[g + 1])
    b = b0 + int(np.searchsorted(genes.blk_start[b0:b1], pos, side='right')) - 1
    f = int(genes.cds_off[b] + pos - genes.blk_start[b])                 # 0-based, genome order
    n = int(genes.cds_len[g])
    pos_ind = n - f if minus else f + 1
    k = (pos_ind + 2) // 3
    old = []
    for t in range(3 * k - 2, 3 * k + 1):                                # the codon's CDS indices, transcript direction
        ft = n - t if minus else t - 1
        bt = b0 + int(np.searchsorted(genes.cds_off[b0:b1], ft, side='right')) - 1
        c = letter(int(genes.blk_start[bt] + ft - genes.cds_off[bt]))
        old.append(_MF_COMP.get(c, 'N') if minus else c)
    new = list(old)
    new[pos_ind - 3 * (k - 1) - 1] = _MF_COMP[alt] if minus else alt
    aa = lambda cod: _MF_CODE[16 * "ACGT".index(cod[0]) + 4 * "ACGT".index(cod[1]) + "ACGT".index(cod[2])] \
        if all(x in "ACGT" for x in cod) else 'X'
    old_aa, new_aa = aa(old), aa(new)
    impact = 0 if new_aa == old_aa else 2 if new_aa == '*' else 1 if old_aa != '*' else 3
    return impact, wrong


def classify_pairs_on_gpu(genome, genes, gene_chrom, pair_gene, pair_start, pair_end, pair_kind, pair_ref, pair_alt, on_device=False):
    """The classifier of annotate_mutation_function: engine.mutation_function on the pairs, the DIG_MF_HOST pairs finished from
    the genome's letters -> host arrays (impact, wrong_ref, n_cds, cds_min, cds_max)."""
    from .. import engine
    out = engine.mutation_function(genome, genes, gene_chrom, pair_gene, pair_start, pair_end, pair_kind, pair_ref, pair_alt,
                                   on_device=on_device)
    impact, status, n_cds, cds_min, cds_max = [a.cpu().numpy() if on_device else a for a in out]
    if (status == engine.MF_OUTSIDE).any():
        raise ValueError("a (mutation, gene) pair of the join lies outside the gene's ranges")
    wrong = status == engine.MF_WRONG_REF
    impact = impact.copy()
    for i in np.flatnonzero(status == engine.MF_HOST):
        impact[i], wrong[i] = _snv_function_from_letters(genome, genes, gene_chrom, int(pair_gene[i]), int(pair_start[i]),
                                                         "ACGT"[pair_ref[i]], "ACGT"[pair_alt[i]])
    return impact, wrong, n_cds, cds_min, cds_max


def annotate_mutation_function(f_mut, f_out, genes, genome, splice_offsets=None, on_device=None, join=None, classify=None):
    """scripts/mutationFunction.R: the raw call file f_mut annotated with GENE and ANNOT, written to f_out as CHROM START END REF
    ALT SAMPLE GENE ANNOT (tab separated, no header, START 0-based, integers).  genes: a bed12 file of coding exons or a GeneSet;
    genome: a FASTA path or a PackedGenome.  A mutation outside every gene range (CDS blocks and essential-splice positions) gets
    GENE "." and Noncoding / Noncoding_INDEL; every other one a row per gene it touches: an SNV (REF and ALT each one of ACGT)
    Synonymous / Missense / Nonsense / Stop_loss / Essential_Splice, anything else cds_INDEL or INDEL_{min}_{max}_{ins|del}{frshift|
    inframe} / INDEL_{min}_{max}_mnv with the range of CDS indices it covers.  SNV pairs whose REF is not the genome's base are
    left out: 10 % or more of the coding SNV pairs raise ValueError, fewer print a warning.  Rows are sorted (stably, from the
    order coding SNVs, noncoding SNVs, coding others, noncoding others) by (CHROM as bytes, START, END).
    join / classify: the two GPU steps as functions (default: dig_overlap_join_* and dig_mutation_function; `on_device` None = the
    device forms unless the process declared itself torch-free) -- join(r_chrom, r_start, r_end, m_chrom, m_start, m_end) ->
    (mutation row, range row) pairs; classify(genome, genes, gene_chrom, gene, start, end, kind, ref, alt) -> (impact, wrong_ref,
    n_cds, cds_min, cds_max).  Returns a dict of row counts."""
    from .. import _lib
    from ..sequence_model import sequence_tools
    from . import gene_annotation
    dev = (not _lib.TORCH_FREE) if on_device is None else bool(on_device)
    if join is None:
        join = lambda *a: _gene_range_join(*a, on_device=dev)
    if classify is None:
        classify = lambda *a: classify_pairs_on_gpu(*a, on_device=dev)
    if not isinstance(genes, gene_annotation.GeneSet):
        genes = gene_annotation.load_cds_bed12(genes, splice_offsets=splice_offsets)
    if genome is not None and not hasattr(genome, 'chrom_index'):
        genome = sequence_tools.load_genome(genome)
    gene_chrom = None
    if genome is not None:
        genes, gene_chrom = genes.on_genome(genome)
    df = read_raw_mutations(f_mut)
    M = len(df)
    ref, alt = df.REF.to_numpy(dtype=object), df.ALT.to_numpy(dtype=object)
    is_snv = (df.REF.isin(list("ACGT")) & df.ALT.isin(list("ACGT"))).to_numpy()
    start, end = df.start.to_numpy(np.int64), df.end.to_numpy(np.int64)

    r_chrom, r_start, r_end, r_gene = genes.ranges()
    pm, pr = join(r_chrom, r_start, r_end, df.CHROM.to_numpy(dtype=object), start, end)
    pair = np.unique(np.stack([np.asarray(pm, np.int64), r_gene[np.asarray(pr, np.int64)]], axis=1), axis=0) if len(pm) \
        else np.zeros((0, 2), np.int64)                                   # distinct (mutation, gene), mutation-major, genes ascending
    pmut, pgene = pair[:, 0], pair[:, 1]
    coding = np.zeros(M, bool)
    coding[pmut] = True

    code = {c: i for i, c in enumerate("ACGT")}
    bare_ref = df.REF.str.replace('-', '', regex=False).str.len().to_numpy()
    bare_alt = df.ALT.str.replace('-', '', regex=False).str.len().to_numpy()
    kind = np.where(is_snv, 0, np.where(bare_ref < bare_alt, 1, 2)).astype(np.uint8)
    snv_code = lambda col: np.array([code.get(x, 0) for x in col.tolist()], np.uint8)
    p_ref, p_alt = snv_code(ref[pmut]), snv_code(alt[pmut])
    impact, wrong, n_cds, cds_min, cds_max = classify(genome, genes, gene_chrom, pgene.astype(np.int32), start[pmut], end[pmut],
                                                      kind[pmut], p_ref, p_alt) if len(pmut) else \
        (np.zeros(0, np.uint8), np.zeros(0, bool), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    impact, wrong = np.asarray(impact), np.asarray(wrong, bool)
    p_snv = is_snv[pmut]
    n_coding_snv, n_wrong = int(p_snv.sum()), int((wrong & p_snv).sum())
    if n_wrong:
        text = "{} ({:.2g}%) mutations have a wrong reference base".format(n_wrong, 100.0 * n_wrong / n_coding_snv)
        if 10 * n_wrong >= n_coding_snv:
            raise ValueError(text + ": wrong assembly? Confirm that the mutations and the FASTA are of the same assembly and species.")
        print("WARNING: " + text + " and were left out.")

    annot = np.empty(len(pmut), dtype=object)
    label = np.array(_MF_LABEL, dtype=object)
    if (impact[p_snv & ~wrong] > 4).any():
        raise ValueError("the classifier left {} SNV pairs without an effect class".format(int((impact[p_snv & ~wrong] > 4).sum())))
    annot[p_snv] = label[np.minimum(impact[p_snv], 4)]                  # (wrong-REF pairs are left out below, whatever their class)
    other = np.flatnonzero(~p_snv)
    if other.size:
        k, n = kind[pmut[other]], np.asarray(n_cds)[other]
        what = np.where(bare_ref[pmut[other]] < bare_alt[pmut[other]], 'ins', np.where(bare_ref[pmut[other]] > bare_alt[pmut[other]], 'del', 'mnv'))
        tail = np.where(what == 'mnv', '', np.where(n % 3 == 0, 'inframe', 'frshift'))
        annot[other] = ["cds_INDEL" if c == 0 else "INDEL_%d_%d_%s%s" % (a, b, w, t)
                        for c, a, b, w, t in zip(n.tolist(), np.asarray(cds_min)[other].tolist(), np.asarray(cds_max)[other].tolist(),
                                                 what.tolist(), tail.tolist())]
    names = np.array(genes.names, dtype=object)
    keep_snv = p_snv & ~wrong
    # the reference's row order in front of its sort: coding SNVs, noncoding SNVs, coding others, noncoding others
    rows = np.concatenate([pmut[keep_snv], np.flatnonzero(~coding & is_snv), pmut[~p_snv], np.flatnonzero(~coding & ~is_snv)])
    nc_snv, nc_other = int((~coding & is_snv).sum()), int((~coding & ~is_snv).sum())
    gene_col = np.concatenate([names[pgene[keep_snv]], np.full(nc_snv, '.', dtype=object), names[pgene[~p_snv]],
                               np.full(nc_other, '.', dtype=object)])
    annot_col = np.concatenate([annot[keep_snv], np.full(nc_snv, 'Noncoding', dtype=object), annot[~p_snv],
                                np.full(nc_other, 'Noncoding_INDEL', dtype=object)])
    chrom = df.CHROM.to_numpy(dtype=object)[rows]
    _, chrom_rank = np.unique(np.array([c.encode() for c in chrom.tolist()], dtype=object), return_inverse=True) if len(rows) \
        else (None, np.zeros(0, np.int64))
    order = np.lexsort((end[rows], start[rows] - 1, chrom_rank))          # (lexsort is stable)
    rows = rows[order]
    out = pd.DataFrame({'CHROM': chrom[order], 'START': start[rows] - 1, 'END': end[rows], 'REF': ref[rows], 'ALT': alt[rows],
                        'SAMPLE': df.SAMPLE.to_numpy(dtype=object)[rows], 'GENE': gene_col[order], 'ANNOT': annot_col[order]})
    out.to_csv(f_out, sep="\t", index=False, header=False)
    if len(out) > M:
        print("WARNING: {} mutation entries were duplicated because they overlap multiple genes.".format(len(out) - M))
    return dict(n_mutations=M, n_rows=len(out), coding_snv=int(keep_snv.sum()), noncoding_snv=nc_snv, coding_other=int((~p_snv).sum()),
                noncoding_other=nc_other, wrong_ref=n_wrong)
