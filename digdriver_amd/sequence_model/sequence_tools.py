"""Trinucleotide sequence model: substitution indexing, context counting, sequence-model training.

Mirror of the parts of DIGDriver/sequence_model/sequence_tools.py that the hot path needs
(reverse_complement :18-19, mk_context_sequences :30-40, seq_to_context :42-57, type_mutation :59-65,
count_sequence_context :67-80, mk_mutation_context :232-262, mk_trans_idx :282-289,
train_sequence_model + mutation_freq_conditional :321-373).  The live path is the 192-type / 64-context
model (collapse=False everywhere, DigPreprocess.py:47,91); collapse=True (96 types) is kept for
completeness.  Genome context counts also come in the reference's default penta-nucleotide form (n_up = n_down = 2:
1 024 contexts, 3 072 substitution types), which trains the per-base route's default S_prob.
"""
import itertools as it

import numpy as np
import pandas as pd

from ..data_tools import mutation_tools

_COMP = str.maketrans('NTCGA', 'NAGCT')
_DNA = 'ACGT'


def reverse_complement(seq):
    return seq[::-1].translate(_COMP)


def mk_context_sequences(n_up=2, n_down=2, collapse=False):
    centre = 'CT' if collapse else _DNA
    keys = [''.join(t) for t in it.product(*([_DNA] * n_up + [centre] + [_DNA] * n_down))]
    return {k: 0 for k in keys}


def seq_to_context(seq, baseix=2, collapse=False):
    if 'N' in seq:
        return ''
    if collapse and seq[baseix] in 'GA':
        return reverse_complement(seq)
    return seq


def type_mutation(REF, ALT, collapse=False):
    if collapse and REF in 'GA':
        REF, ALT = REF.translate(_COMP), ALT.translate(_COMP)
    return "{}>{}".format(REF, ALT)


_CODE = np.full(256, -1, np.int64)
for _i, _c in enumerate(_DNA):
    _CODE[ord(_c)] = _i


def count_sequence_context(seq, n_up=2, n_down=2, nuc_dict=None, collapse=False):
    """Counts of every (n_up + 1 + n_down)-mer centred on each position; windows containing N are skipped.
    Vectorised (base-4 rolling code + bincount) instead of the reference's per-position Python loop."""
    if nuc_dict is None:
        nuc_dict = mk_context_sequences(n_up=n_up, n_down=n_down, collapse=collapse)
    k = n_up + 1 + n_down
    codes = _CODE[np.frombuffer(seq.upper().encode('ascii'), dtype=np.uint8)]
    if len(codes) < k:
        return nuc_dict
    win = np.lib.stride_tricks.sliding_window_view(codes, k)
    ok = (win >= 0).all(axis=1)
    val = (win[ok] * (4 ** np.arange(k - 1, -1, -1))).sum(axis=1)
    cnt = np.bincount(val, minlength=4 ** k)
    for idx in np.flatnonzero(cnt):
        s = ''.join(_DNA[(idx // 4 ** (k - 1 - j)) % 4] for j in range(k))
        s = seq_to_context(s, baseix=n_up, collapse=collapse)
        nuc_dict[s] += int(cnt[idx])
    return nuc_dict


def mk_mutation_context(n_up=1, n_down=1, collapse=False, return_df=False):
    """Rows (MUT_TYPE, CONTEXT) in the reference's order: per reference base (A, C, G, T; C, T only when
    collapsed) the three substitutions are the outer loop and the contexts the inner one."""
    muts = {'A': ['A>T', 'A>C', 'A>G'], 'C': ['C>A', 'C>G', 'C>T'], 'G': ['G>T', 'G>C', 'G>A'], 'T': ['T>A', 'T>G', 'T>C']}
    tups = []
    for ref in ('CT' if collapse else 'ACGT'):
        keys = [''.join(t) for t in it.product(*([_DNA] * n_up + [ref] + [_DNA] * n_down))]
        tups += list(it.product(muts[ref], keys))
    if return_df:
        return pd.DataFrame(tups, columns=['MUT_TYPE', 'CONTEXT'])
    return {t: 0 for t in tups}


def mk_trans_idx(n_up=1, n_down=1, collapse=False):
    """Sorted 'XYZ>XaZ' strings (sequence_tools.py:282-289)."""
    keys = mk_mutation_context(n_up=n_up, n_down=n_down, collapse=collapse)
    return sorted(k[1] + '>' + k[1][:n_up] + k[0][2] + k[1][n_up + 1:] for k in keys)


def mutation_freq_conditional(df_freq, S_gen):
    """sequence_tools.py:356-373: FREQ = COUNT / genome count of the context."""
    df_freq["FREQ"] = df_freq.COUNT.values / np.array([S_gen[c] for c in df_freq.CONTEXT], dtype=float)
    return df_freq


def sequence_model_counts(df_mut_white, n_up=1, n_down=1):
    """The per-cohort sufficient statistic of the sequence model: 192 integer counts of (MUT_TYPE, CONTEXT) in the
    model's row order.  Shards of one cohort add (all-reduce / rank-ordered all-gather sum)."""
    empty = mk_mutation_context(n_up=n_up, n_down=n_down, collapse=False, return_df=True)
    pos = {(m, c): i for i, (m, c) in enumerate(zip(empty.MUT_TYPE, empty.CONTEXT))}
    cnt = np.zeros(len(empty), np.int64)
    keys = pd.Series(list(zip(df_mut_white.MUT_TYPE, df_mut_white.CONTEXT))).value_counts()
    for key, v in keys.items():
        if key in pos:
            cnt[pos[key]] = v
    return empty, cnt


def train_sequence_model(regions, df_mut, genome_counts, n_up=1, n_down=1, key_prefix=None, counts=None):
    """sequence_tools.py:321-354 -> (df_freq_mut [192: MUT_TYPE, CONTEXT, COUNT, FREQ], df_freq_context [64: FREQ]); with
    n_up = n_down = 2, 3 072 and 1 024 rows.  `counts` lets a caller pass pre-reduced counts in the model's row order
    (multi-GPU / multi-shard path)."""
    if counts is None:
        df_bed = pd.DataFrame(regions, columns=['CHROM', 'START', 'END'])
        white = mutation_tools.restrict_mutations_by_bed(df_mut, df_bed, unique=True, remove_X=False)
        white.columns = df_mut.columns
        df_ct, counts = sequence_model_counts(white, n_up=n_up, n_down=n_down)
    else:
        df_ct = mk_mutation_context(n_up=n_up, n_down=n_down, collapse=False, return_df=True)
    df_ct["COUNT"] = np.asarray(counts, dtype=float)
    df_freq_mut = mutation_freq_conditional(df_ct, genome_counts)
    df_freq_context = df_freq_mut.pivot_table('FREQ', index=['CONTEXT'], aggfunc="sum")
    return df_freq_mut, df_freq_context


# ---------------------------------------------------------------------------------------------
# sequence models of many cohorts in one pass (reference: DigPretrain.py sequenceModel, one cohort per process)
# ---------------------------------------------------------------------------------------------
_TYPE_TABLES = {}


def _type_table(n_up, n_down):
    """(MUT_TYPE label -> row, CONTEXT label -> column, table i32 [13, n_contexts + 1], K): table[row, column] is the row of
    mk_mutation_context(n_up, n_down) that holds the label pair, K where it holds none; the last row and column stand for a label
    the model does not know."""
    if (n_up, n_down) not in _TYPE_TABLES:
        df = mk_mutation_context(n_up=n_up, n_down=n_down, collapse=False, return_df=True)
        muts = {m: i for i, m in enumerate(dict.fromkeys(df.MUT_TYPE))}
        ctxs = {c: i for i, c in enumerate(dict.fromkeys(df.CONTEXT))}
        table = np.full((len(muts) + 1, len(ctxs) + 1), len(df), np.int32)
        table[[muts[m] for m in df.MUT_TYPE], [ctxs[c] for c in df.CONTEXT]] = np.arange(len(df), dtype=np.int32)
        _TYPE_TABLES[(n_up, n_down)] = (muts, ctxs, table, len(df))
    return _TYPE_TABLES[(n_up, n_down)]


def _label_codes(values, ids):
    """Per value its id, len(ids) for a value without one (a missing label included)."""
    codes, uniq = pd.factorize(values)
    of_uniq = np.array([ids.get(u, len(ids)) for u in uniq] + [len(ids)], np.int64)          # (code -1, a missing label: the last entry)
    return of_uniq[codes]


def encode_sequence_rows(f_mut, chrom_ids, n_up=1, n_down=1):
    """An annotated mutation file (10 or 11 columns: ... ANNOT MUT_TYPE CONTEXT) as the arrays engine.sequence_counts takes, for one
    cohort: the rows DigPretrain.py sequenceModel counts from -- read_mutation_file(drop_duplicates=True): autosomes, the first row
    of every (CHROM, START, END, REF, ALT, SAMPLE), unique indels -- without ANNOT == 'INDEL'.  Chromosomes are compared as the join
    compares them, as text, with `chrom_ids` (label -> id of the windows' chromosomes); rows on other chromosomes can join nothing
    and are left out.
    Returns dict(chrom, start, end i64; type i32: the row of mk_mutation_context(n_up, n_down) with the row's (MUT_TYPE, CONTEXT),
    K for a pair the table does not hold; one_base: whether every kept row has END - START == 1, the rows a window holds whole or
    not at all; frame: the kept rows as a frame when one_base is False -- such a cohort is counted by the serial statement)."""
    df = mutation_tools.read_mutation_file(f_mut, drop_duplicates=True)
    df = df[df.ANNOT != 'INDEL']
    one_base = bool((df.END.values - df.START.values == 1).all())
    muts, ctxs, table, _K = _type_table(n_up, n_down)
    ch = _label_codes(df.CHROM.values.astype(str), {label: i for i, label in enumerate(chrom_ids)})
    known = ch < len(chrom_ids)
    ch = np.array(list(chrom_ids.values()) + [0], np.int64)[ch]
    t = table[_label_codes(df.MUT_TYPE.values, muts), _label_codes(df.CONTEXT.values, ctxs)]
    return dict(chrom=ch[known], start=df.START.to_numpy(np.int64)[known], end=df.END.to_numpy(np.int64)[known],
                type=np.ascontiguousarray(t[known], np.int32), one_base=one_base, frame=None if one_base else df)


def train_sequence_models(f_muts, idx, mappability, genome_counts_frame, map_thresh=0.5, n_up=1, n_down=1, on_device=None, device=0):
    """DigPretrain.py sequenceModel (:179-208) for the cohorts `f_muts` (annotated mutation files) in one pass: idx [N, 3] ints
    (CHROM, START, END), mappability [N] and genome_counts_frame (all_window_genome_counts: a row per window, a column per context)
    as the genome-counts container holds them.  The whitelist is the windows with mappability > map_thresh; S_genome, the column sum
    of the frame over them, is formed once.  The substitution counts of all cohorts come from one engine.sequence_counts call
    (dig_overlap_join_* + dig_sequence_counts), whose rule -- a row counts once when a whitelisted window holds it -- is the
    reference's for one-base rows.  A cohort with a kept row of another length (a multi-base substitution carrying an SNV class, an
    empty interval), of which the reference counts every distinct clipped piece, is counted on the host by the serial statement
    (restrict_mutations_by_bed + sequence_model_counts) and named in the result.
    on_device: True = device tensors and the device entry points, False = numpy and the `_host` twins (no torch), None = the device
    unless the process is torch-free.
    Returns (models, counts, serial): models[c] = (df_freq_mut, df_freq_context) of train_sequence_model for f_muts[c], counts i64
    [C, K] in the model's row order, serial = the indices of the cohorts counted on the host."""
    from .. import engine
    from ..data_tools import cohort_rows
    f_muts = [f_muts] if isinstance(f_muts, (str, bytes)) or hasattr(f_muts, "__fspath__") else list(f_muts)
    if not f_muts:
        raise ValueError("no mutation file")
    idx = np.asarray(idx)
    if idx.ndim != 2 or idx.shape[1] != 3 or idx.dtype.kind not in "iu":
        raise ValueError("idx: an integer array [N, 3] of CHROM, START, END")
    keep = np.asarray(mappability).reshape(-1) > map_thresh
    if len(keep) != len(idx) or len(genome_counts_frame) != len(idx):
        raise ValueError("idx, mappability and the genome counts: one row per window")
    S_genome = genome_counts_frame[keep].sum(axis=0)
    white = idx[keep].astype(np.int64)
    chrom_ids = {str(c): int(c) for c in np.unique(white[:, 0])}
    C, K = len(f_muts), _type_table(n_up, n_down)[3]
    cohorts = [encode_sequence_rows(f, chrom_ids, n_up, n_down) for f in f_muts]
    serial = [c for c in range(C) if not cohorts[c]["one_base"]]
    batch = [c for c in range(C) if cohorts[c]["one_base"]]
    cat = lambda k, dt: cohort_rows.column(cohorts, k, dt, subset=batch)
    rows = cohort_rows.place([cat("chrom", "i64"), cat("start", "i64"), cat("end", "i64"), cat("type", "i32"),
                              cohort_rows.cohort_column(cohorts, "type", batch)], on_device, device)
    counts = engine.sequence_counts(white[:, 0], white[:, 1], white[:, 2], *rows, K, C, device=device)
    counts = np.array(counts.cpu().numpy() if engine.is_cuda(counts) else counts, np.int64)
    df_bed = pd.DataFrame(white, columns=['CHROM', 'START', 'END'])
    for c in serial:
        df_mut = cohorts[c]["frame"]
        inside = mutation_tools.restrict_mutations_by_bed(df_mut, df_bed, unique=True, remove_X=False)
        inside.columns = df_mut.columns
        counts[c] = sequence_model_counts(inside, n_up=n_up, n_down=n_down)[1]
    models = [train_sequence_model(None, None, S_genome, n_up=n_up, n_down=n_down, counts=counts[c]) for c in range(C)]
    return models, counts, serial


# ---------------------------------------------------------------------------------------------
# context counting from sequence on the GPU (reference: pysam fetch + Python loop per region)
# ---------------------------------------------------------------------------------------------
_GENOMES = {}


def load_genome(f_fasta):
    """FASTA -> PackedGenome (4 bits per base, cached in memory per path and as <fasta>.dig4.npz on disk)."""
    from ..data_tools.genome import PackedGenome
    if f_fasta not in _GENOMES:
        _GENOMES[f_fasta] = f_fasta if isinstance(f_fasta, PackedGenome) else PackedGenome.from_fasta(f_fasta)
    return _GENOMES[f_fasta]


def _require_supported(n_up, n_down):
    if (n_up, n_down) not in ((1, 1), (2, 2)):
        raise NotImplementedError("the GPU context counter handles (n_up, n_down) = (1, 1) (trinucleotides, what the driver "
                                  "path uses: onthefly_tools.py:70-71,120) and (2, 2) (penta-nucleotides, the per-base model); "
                                  "got (%s, %s)" % (n_up, n_down))


def count_contexts_by_regions(f_fasta, chrom_lst, start_lst, end_lst, n_up=2, n_down=2, collapse=False):
    """sequence_tools.py:82-99: frame [regions x 4^(n_up + 1 + n_down) contexts] (columns in mk_context_sequences order, index
    "{CHROM}:{START}-{END}") -- one dig_count_contexts2 (trinucleotides) or dig_count_contexts5 (penta-nucleotides) launch for
    all regions; collapse=True: the pyrimidine-centred half of the contexts.  `f_fasta`: path or PackedGenome."""
    from .. import engine
    _require_supported(n_up, n_down)
    genome = f_fasta if hasattr(f_fasta, "words") else load_genome(f_fasta)
    cnt = engine.count_contexts(genome, list(chrom_lst), np.asarray(start_lst, np.int64), np.asarray(end_lst, np.int64),
                                n_up=n_up, n_down=n_down)
    idx = ["{}:{}-{}".format(c, s, e) for c, s, e in zip(chrom_lst, start_lst, end_lst)]
    cnt = cnt.cpu().numpy().astype(np.int64)
    ctx = list(mk_context_sequences(n_up, n_down).keys())
    if not collapse:
        return pd.DataFrame(cnt, index=idx, columns=ctx)
    # collapse=True (the K = 96 model): a window centred on A or G counts as its reverse complement (seq_to_context,
    # sequence_tools.py:42-55): the pyrimidine-centred columns, each the sum of a context and its reverse complement
    pos = {c: i for i, c in enumerate(ctx)}
    half = list(mk_context_sequences(n_up, n_down, collapse=True).keys())
    cols = np.array([pos[c] for c in half]), np.array([pos[reverse_complement(c)] for c in half])
    return pd.DataFrame(cnt[:, cols[0]] + cnt[:, cols[1]], index=idx, columns=half)


def nonc_elt_context_count(regions, trans_idx, f_fasta, n_up=1, n_down=1):
    """sequence_tools.py:527-566: `regions` = (chrom, start, end, strand) tuples; '-' / -1 strand regions count the
    reverse-complemented sequence; result [regions x substitutions] (192 for trinucleotides, 3 072 for penta-nucleotides)
    with the sorted substitution keys as columns, every substitution column holding the count of its context; index
    "chr{chrom}:{start}-{end}"."""
    from .. import engine
    _require_supported(n_up, n_down)
    genome = f_fasta if hasattr(f_fasta, "words") else load_genome(f_fasta)
    chroms = ['chr' + str(r[0]) for r in regions]
    starts = np.array([r[1] for r in regions], np.int64)
    ends = np.array([r[2] for r in regions], np.int64)
    minus = np.array([(r[3] == '-' or r[3] == -1) for r in regions], bool)
    cnt = engine.count_contexts(genome, chroms, starts, ends, minus, n_up=n_up, n_down=n_down).cpu().numpy().astype(np.float64)
    keys = sorted(set(trans_idx))
    ctx = list(mk_context_sequences(n_up, n_down).keys())
    pos = {c: i for i, c in enumerate(ctx)}
    cols = np.array([pos[k.split('>')[0]] for k in keys])
    idx = ["{}:{}-{}".format(c, s, e) for c, s, e in zip(chroms, starts, ends)]
    return pd.DataFrame(cnt[:, cols], index=idx, columns=keys)


def precount_region_contexts_parallel(f_nonc_bed, f_fasta, n_procs, window, sub_elts=True, n_up=1, n_down=1):
    """sequence_tools.py:481-525: context counts of every block of a bed12 (sub_elts) or of every bed row, rows with a
    repeated index removed.  n_procs is accepted for compatibility (one launch does all regions).  As in the reference, the
    counts are trinucleotide ones (192 columns, what preprocess_nonc reads) whatever n_up / n_down say: it builds the
    (1, 1) substitution index and does not pass n_up / n_down on."""
    from ..data_tools import mutation_tools
    _require_supported(n_up, n_down)
    trans_idx = mk_trans_idx(n_up=1, n_down=1, collapse=False)
    df = pd.read_csv(f_nonc_bed, sep='\t', header=None, names=None, low_memory=False, dtype={0: str})
    if sub_elts:
        df6 = mutation_tools._bed12_to_bed6(df)
        chrom = df6.CHROM.astype(str)
        if 'chr' in str(chrom.iloc[0]):
            chrom = chrom.map(lambda x: x.lstrip('chr'))
        regions = list(zip(chrom, df6.START, df6.END, df6.STRAND))
    else:
        chrom = df[0].astype(str)
        if 'chr' in str(chrom.iloc[0]):
            chrom = chrom.map(lambda x: x.lstrip('chr'))
        regions = list(zip(chrom, df[1], df[2], df[5]))
    results = nonc_elt_context_count(regions, trans_idx, f_fasta)
    return results.loc[~results.index.duplicated()]


def count_contexts_in_bed(f_fasta, df_bed, n_up=1, n_down=1, N_proc=1, N_chunk=10, collapse=False):
    """sequence_tools.py:101-137: context counts of every row of a bed-like frame (columns 0-2 = chrom, start, end;
    'chr' is prepended to the chromosome label).  One launch; N_proc / N_chunk accepted for compatibility."""
    chrom_lst = ['chr{}'.format(val) for val in df_bed.iloc[:, 0].values]
    return count_contexts_by_regions(f_fasta, chrom_lst, df_bed.iloc[:, 1].values, df_bed.iloc[:, 2].values, n_up=n_up,
                                     n_down=n_down, collapse=collapse)


def initialize_nonc_data(f_nonc_data, f_genome_counts, window, n_up=1, n_down=1):
    """sequence_tools.py:451-478: start an element-data container from the genome-wide window counts: the sorted
    substitution index and window_{w}/full_window_si_{index,values}."""
    from ..io import mapfile
    key = 'window_{}'.format(window)
    with mapfile.batch(f_nonc_data):
        if not mapfile.has_key(f_nonc_data, 'substitution_idx'):
            mapfile.write_array(f_nonc_data, 'substitution_idx', np.array(mk_trans_idx(n_up=n_up, n_down=n_down, collapse=False)))
        if not (mapfile.has_key(f_nonc_data, key + '/full_window_si_index') and
                mapfile.has_key(f_nonc_data, key + '/full_window_si_values')):
            idx = mapfile.read_array(f_genome_counts, 'idx')
            genome_df = mapfile.read_frame(f_genome_counts, 'all_window_genome_counts')
            assert int(str(genome_df.index[0]).split('-')[-1]) == window      # the counts must be on this window size (:476)
            mapfile.write_array(f_nonc_data, key + '/full_window_si_values', genome_df.values.astype(np.int64))
            mapfile.write_array(f_nonc_data, key + '/full_window_si_index', idx)


def preprocess_nonc(f_nonc_bed, f_nonc_data, f_pretrained, L_contexts, save_key, window):
    """sequence_tools.py:596-641: per-element L counts (sum of the block rows of L_contexts) and geometry under
    window_{w}/{save_key}.  The reference stores one h5 group per element plus its overlapped-window counts; the
    overlaps and region counts are recomputed on the GPU at model time here (dig_ideal_overlaps_host +
    dig_accumulate_elements), so the container holds flat arrays: names, chrom, strand, blk_ptr, blk_start, blk_end, L."""
    from ..data_tools import mutation_tools
    from ..io import mapfile
    df_elts = mutation_tools.bed12_boundaries(f_nonc_bed)
    E = len(df_elts)
    blk_ptr = np.concatenate([[0], np.cumsum([len(b) for b in df_elts.BLOCK_STARTS])]).astype(np.int64)
    blk_start = np.array([s for b in df_elts.BLOCK_STARTS for s in b], np.int64)
    blk_end = np.array([e for b in df_elts.BLOCK_ENDS for e in b], np.int64)
    chrom = df_elts.CHROM.values.astype(np.int32)
    owner = np.repeat(np.arange(E), np.diff(blk_ptr))
    keys = ['chr{}:{}-{}'.format(c, s, e) for c, s, e in zip(chrom[owner], blk_start, blk_end)]
    L = np.zeros((E, 192))
    np.add.at(L, owner, L_contexts.loc[keys].values)
    base = 'window_{}/{}/'.format(window, save_key)
    with mapfile.batch(f_nonc_data):                 # one rewrite of the container instead of one per key
        mapfile.write_array(f_nonc_data, base + 'names', df_elts.ELT.values.astype(str))
        mapfile.write_array(f_nonc_data, base + 'chrom', chrom)
        mapfile.write_array(f_nonc_data, base + 'strand', df_elts.STRAND.astype(str).values)
        mapfile.write_array(f_nonc_data, base + 'blk_ptr', blk_ptr)
        mapfile.write_array(f_nonc_data, base + 'blk_start', blk_start)
        mapfile.write_array(f_nonc_data, base + 'blk_end', blk_end)
        mapfile.write_array(f_nonc_data, base + 'L', np.rint(L).astype(np.int32))


def preprocess_sites(f_sites, f_nonc_data, f_pretrained, save_key, window):
    """sequence_tools.py:643-700: element data for a SITES file (mutation-file layout, element name in the SAMPLE
    column, one row per (position, substitution) site, optional STRAND column).  Per element: L[key] = number of its
    sites with substitution key "XYZ>XaZ" (reverse-complemented for '-' strand elements, rows without context
    skipped); its overlapped windows come from all site intervals.  Stored as the flat arrays preprocess_nonc writes
    (names in sorted order, as the reference's groupby gives them); f_pretrained is accepted for compatibility."""
    from ..data_tools import mutation_tools
    from ..io import mapfile
    keys = sorted(mk_trans_idx(n_up=1, n_down=1, collapse=False))
    pos = {k: i for i, k in enumerate(keys)}
    df = mutation_tools.read_mutation_file(f_sites)
    df = df.drop(columns=['GENE', 'ANNOT', 'REF', 'ALT']).rename(columns={'SAMPLE': 'GENE'})
    df.loc[df.CONTEXT.isna(), 'CONTEXT'] = 'nan'
    if 'STRAND' not in df.columns:
        df['STRAND'] = '.'
    names, chroms, strands, blk_ptr, bs, be, Ls = [], [], [], [0], [], [], []
    for name, group in df.groupby('GENE'):
        strand = list(group['STRAND'])[0]
        minus = strand == "-1" or strand == "-"
        L = np.zeros(192, np.int32)
        for m, c in zip(group['MUT_TYPE'], group['CONTEXT']):
            key = (reverse_complement(c) + '>' + reverse_complement(c[0] + m[2] + c[2])) if minus else (c + '>' + c[0] + m[2] + c[2])
            if 'nan' in key:
                continue
            L[pos[key]] += 1
        names.append(str(name))
        chroms.append(int(list(group['CHROM'])[0]))
        strands.append(str(strand))
        bs.extend(int(x) for x in group['START'])
        be.extend(int(x) for x in group['END'])
        blk_ptr.append(len(bs))
        Ls.append(L)
    base = 'window_{}/{}/'.format(window, save_key)
    with mapfile.batch(f_nonc_data):                 # one rewrite of the container instead of one per key
        mapfile.write_array(f_nonc_data, base + 'names', np.array(names))
        mapfile.write_array(f_nonc_data, base + 'chrom', np.array(chroms, np.int32))
        mapfile.write_array(f_nonc_data, base + 'strand', np.array(strands))
        mapfile.write_array(f_nonc_data, base + 'blk_ptr', np.array(blk_ptr, np.int64))
        mapfile.write_array(f_nonc_data, base + 'blk_start', np.array(bs, np.int64))
        mapfile.write_array(f_nonc_data, base + 'blk_end', np.array(be, np.int64))
        mapfile.write_array(f_nonc_data, base + 'L', np.stack(Ls) if Ls else np.zeros((0, 192), np.int32))


# ---------------------------------------------------------------------------------------------
# the gene container from a bed12 of coding exons + FASTA, and the window counts of the genes (DigPreprocess.py
# preprocess_genic_model; reference: L_data from refcds_hg19.rda, si_count_* as a Python loop per base, sequence_tools.py:375-449)
# ---------------------------------------------------------------------------------------------
def _region_counts(genome, chroms, starts, ends, minus, on_device):
    from .. import engine
    cnt = engine.count_contexts(genome, chroms, starts, ends, minus, on_device=on_device)
    return (cnt.cpu().numpy() if on_device else cnt).astype(np.int64)


def _context_columns(trans_idx):
    """(sorted substitution keys, for each the column of its context among mk_context_sequences(1, 1))."""
    keys = sorted(set(str(k) for k in trans_idx))
    pos = {c: i for i, c in enumerate(mk_context_sequences(1, 1))}
    return keys, np.array([pos[k.split('>')[0]] for k in keys], np.int64)


def si_by_regions(f_fasta, trans_idx, regions, strand=1, n_up=1, n_down=1, normed=True, on_device=None, count=None):
    """sequence_tools.py:396-425: for regions "chrom:start-end" the number of positions at which each substitution of trans_idx can
    happen -- the count of its trinucleotide in the regions (each fetched with one base on either side, cut off at the contig's
    ends; windows with an N skipped), on the reverse-complemented sequence for strand -1 / '-'.  One-column frame indexed by the
    sorted substitution keys.  count(genome, chroms, starts, ends, minus) -> [R, 64] replaces dig_count_contexts2."""
    if (n_up, n_down) != (1, 1):
        raise NotImplementedError("si_by_regions counts trinucleotides (n_up = n_down = 1)")
    genome = load_genome(f_fasta)
    chroms = [r.split(':')[0] for r in regions]
    starts = np.array([int(r.split(':')[1].split('-')[0]) for r in regions], np.int64)
    ends = np.array([int(r.split('-')[1]) for r in regions], np.int64)
    minus = np.full(len(regions), strand == -1 or strand == '-', bool)
    count = count or (lambda *a: _region_counts(*a, _on_device(on_device)))
    cnt = np.asarray(count(genome, chroms, starts, ends, minus), np.int64).reshape(-1, 64).sum(axis=0)
    keys, cols = _context_columns(trans_idx)
    return pd.DataFrame(cnt[cols], index=keys)


def si_count_pretrain(gene_lst, f_genic, f_fasta, window, on_device=None, count=None):
    """sequence_tools.py:375-393: frame [genes x 192 sorted substitutions] of the context counts of the windows each gene of
    gene_lst overlaps (get_ideal_overlaps of its CDS blocks), on the gene's strand; every substitution column holds its context's
    count.  The genes come from window_{w}/genes/ of f_genic (preprocess_genic).  All genes at once: the distinct windows are
    counted by one dig_count_contexts2 launch on the + strand (a - gene reads the reverse-complemented contexts) and summed per
    gene."""
    from .. import engine
    from ..io import mapfile
    base = 'window_{}/genes/'.format(window)
    names = mapfile.read_array(f_genic, base + 'names').astype(str)
    pos = {n: i for i, n in enumerate(names)}
    sel = np.array([pos[g] for g in gene_lst], np.int64)
    chrom_str = mapfile.read_array(f_genic, base + 'chrom_str').astype(str)[sel]
    strand = mapfile.read_array(f_genic, base + 'strand').astype(str)[sel]
    blk_ptr = mapfile.read_array(f_genic, base + 'blk_ptr').astype(np.int64)
    bs, be = (mapfile.read_array(f_genic, base + k).astype(np.int64) for k in ('blk_start', 'blk_end'))
    cnt_blk = (blk_ptr[1:] - blk_ptr[:-1])[sel]
    ptr = np.concatenate([[0], np.cumsum(cnt_blk)]).astype(np.int64)
    take = np.repeat(blk_ptr[sel] - ptr[:-1], cnt_blk) + np.arange(int(ptr[-1]), dtype=np.int64)
    bs, be = bs[take], be[take]
    if mapfile.has_key(f_genic, 'substitution_idx'):
        trans_idx = mapfile.read_array(f_genic, 'substitution_idx').astype(str)
    else:
        trans_idx = mk_trans_idx(n_up=1, n_down=1, collapse=False)
    keys, cols = _context_columns(trans_idx)
    out = np.zeros((len(sel), 64), np.int64)
    if len(sel) and len(bs):
        labels, code = np.unique(chrom_str, return_inverse=True)
        owner = np.repeat(np.arange(len(sel)), cnt_blk)
        # the table of every window a block can touch: per contig 0, w, ... beyond the last block's end
        top = np.zeros(len(labels), np.int64)
        np.maximum.at(top, code[owner], be)
        n_bins = top // window + 2
        bin_chrom = np.repeat(np.arange(len(labels), dtype=np.int32), n_bins)
        bin_start = np.concatenate([np.arange(n, dtype=np.int64) * window for n in n_bins])
        ov_ptr, ov_idx = engine.ideal_overlaps(code.astype(np.int32), ptr, bs, be, window, bin_chrom, bin_start)
        used, inv = np.unique(ov_idx, return_inverse=True)
        genome = load_genome(f_fasta)
        count = count or (lambda *a: _region_counts(*a, _on_device(on_device)))
        chroms = ['chr{}'.format(labels[c]) for c in bin_chrom[used]]
        cnt = np.asarray(count(genome, chroms, bin_start[used], bin_start[used] + window, np.zeros(len(used), bool)), np.int64)
        has = np.diff(ov_ptr) > 0
        out[has] = np.add.reduceat(cnt[inv], ov_ptr[:-1][has], axis=0)
        ctx = list(mk_context_sequences(1, 1))
        rc = np.array([ctx.index(reverse_complement(c)) for c in ctx], np.int64)
        flip = (strand == '-') | (strand == '-1')
        out[flip] = out[flip][:, rc]
    return pd.DataFrame(out[:, cols], index=list(gene_lst), columns=keys)


def si_count_parallel(f_genic, f_fasta, window, n_procs=1, on_device=None, count=None):
    """sequence_tools.py:428-449 for every gene of the container; n_procs is accepted for compatibility (one launch)."""
    from ..io import mapfile
    names = mapfile.read_array(f_genic, 'window_{}/genes/names'.format(window)).astype(str)
    return si_count_pretrain(list(names), f_genic, f_fasta, window, on_device=on_device, count=count)


def preprocess_genic(f_cds_bed, f_fasta, f_genic, window, on_device=None, counts=None):
    """The gene container of genicModel / geneDriver from a bed12 of coding exons and a FASTA: under window_{w}/genes/ of f_genic
    the arrays genic_model reads -- names, chrom (i32), chrom_str, strand, blk_ptr, blk_start, blk_end (the GeneSet's 1-based closed
    CDS blocks) and L i32 [G, 4, 192], the possible substitutions of every gene by class (silent, missense, nonsense, essential
    splice) and sorted substitution type (dig_gene_site_counts) -- plus n_stop_loss.  The reference takes L (L_data) from dNdScv's
    refcds_hg19.rda and has no code that makes it.  Genes on X / Y are kept (chrom 23 / 24; genic_model skips them by chrom_str),
    genes on any other non-numeric contig are dropped with a printed count.  f_cds_bed: a bed12 file or a GeneSet; f_fasta: a
    path or a PackedGenome.  counts(genome, genes, gene_chrom) -> (L, n_stop_loss) replaces the kernel.  Returns the GeneSet
    written."""
    from .. import engine
    from ..data_tools import gene_annotation
    from ..io import mapfile
    genes = f_cds_bed if isinstance(f_cds_bed, gene_annotation.GeneSet) else gene_annotation.load_cds_bed12(f_cds_bed)
    genome = load_genome(f_fasta)
    genes, gene_chrom = genes.on_genome(genome)
    label = np.array([c[3:] if c.startswith('chr') else c for c in genes.chrom.astype(str)], dtype=object)
    sex = {'X': 23, 'Y': 24}
    keep = np.array([c.isdigit() or c in sex for c in label], bool)
    if not keep.all():
        print("Dropping {} genes on contigs other than the numbered ones, X and Y: {}".format(
            int((~keep).sum()), ", ".join(sorted(set(label[~keep].tolist())))))
        genes, gene_chrom, label = genes.subset(keep), gene_chrom[keep], label[keep]
    dev = _on_device(on_device)
    counts = counts or (lambda *a: engine.gene_site_counts(*a, on_device=dev))
    L, n_stop_loss = counts(genome, genes, gene_chrom)
    L = np.ascontiguousarray(L, np.int32).reshape(len(genes), 4, 192)
    base = 'window_{}/genes/'.format(window)
    with mapfile.batch(f_genic):
        mapfile.write_array(f_genic, base + 'names', np.array(genes.names, dtype=str))
        mapfile.write_array(f_genic, base + 'chrom', np.array([sex[c] if c in sex else int(c) for c in label], np.int32))
        mapfile.write_array(f_genic, base + 'chrom_str', label.astype(str))
        mapfile.write_array(f_genic, base + 'strand', np.where(genes.minus != 0, '-', '+').astype(str))
        mapfile.write_array(f_genic, base + 'blk_ptr', genes.blk_ptr)
        mapfile.write_array(f_genic, base + 'blk_start', genes.blk_start)
        mapfile.write_array(f_genic, base + 'blk_end', genes.blk_end)
        mapfile.write_array(f_genic, base + 'L', L)
        mapfile.write_array(f_genic, base + 'n_stop_loss', np.ascontiguousarray(n_stop_loss, np.int32))
    return genes


# ---------------------------------------------------------------------------------------------
# sequence context of mutations (DigPreprocess.py addMutationContext; reference: a Python loop per row over a whole
# chromosome string, one pool worker per chromosome, sequence_tools.py:130-222) -- dig_mutation_contexts on the GPU
# ---------------------------------------------------------------------------------------------
_BASES = np.frombuffer(b'ACGT', np.uint8)
_COMP_BYTES = bytes.maketrans(b'NTCGA', b'NAGCT')


def _on_device(on_device):
    from .. import _lib
    return (not _lib.TORCH_FREE) if on_device is None else bool(on_device)


def _host_window(genome, ci, start, n_up, n_down, collapse):
    """The context of one row whose window the kernel left to the host (a letter other than ACGT, a chromosome end): the
    reference's seq[START - n_up : START + n_down + 1] with Python slice semantics, then seq_to_context."""
    a, b, _ = slice(start - n_up, start + n_down + 1).indices(int(genome.lengths[ci]))
    w = genome.letters(ci, a, b) if b > a else b''
    if b'N' in w:
        return ''
    if collapse:
        if len(w) <= n_up:
            raise ValueError("START %d of %s: with collapse=True the reference indexes past its %d-letter window (IndexError)"
                             % (start, genome.names[ci], len(w)))
        if w[n_up:n_up + 1] in (b'G', b'A'):
            w = w[::-1].translate(_COMP_BYTES)
    return w.decode('ascii')


def _kernel_rows(genome, chroms, starts, refs, n_up, n_down, collapse, on_device):
    """engine.mutation_contexts on host arrays: (status, code, host, host_ctx) -- host: the rows the kernel left to the host
    (MC_HOST), host_ctx: their contexts."""
    from .. import engine
    status, code = engine.mutation_contexts(genome, chroms, starts, refs, n_up=n_up, n_down=n_down, collapse=collapse,
                                            on_device=on_device)
    if on_device:
        status, code = status.cpu().numpy(), code.cpu().numpy().view(np.uint32)
    host = np.flatnonzero(status == engine.MC_HOST)
    host_ctx = []
    if host.size:
        ci = genome.chrom_index(np.asarray(chroms)[host])
        st = np.asarray(starts, np.int64)[host]
        host_ctx = [_host_window(genome, int(c), int(s), n_up, n_down, collapse) for c, s in zip(ci, st)]
    return status, code, host, host_ctx


def _row_contexts(genome, chroms, starts, refs, n_up, n_down, collapse, on_device):
    """(status, contexts): the kernel's status per row and the CONTEXT strings ('' for a dropped row), rows in group order."""
    from .. import engine
    status, code, host, host_ctx = _kernel_rows(genome, chroms, starts, refs, n_up, n_down, collapse, on_device)
    W = n_up + n_down + 1
    ctx = np.full(len(status), '', dtype=object)
    kept = np.flatnonzero(status == engine.MC_KEPT)
    if kept.size:
        letters = _BASES[(code[kept, None] >> (2 * np.arange(W, dtype=np.uint32))) & np.uint32(3)]
        ctx[kept] = np.ascontiguousarray(letters).view('S%d' % W).ravel().astype('U%d' % W)
    if host.size:
        ctx[host] = host_ctx
    return status, ctx


def _mut_types(ref, alt, collapse):
    """type_mutation over columns: REF>ALT, both complemented letter by letter when REF is G or A (collapse)."""
    ref, alt = ref.astype(str), alt.astype(str)
    if collapse:
        flip = ref.isin(['G', 'A'])
        table = str.maketrans('NTCGA', 'NAGCT')
        ref, alt = ref.where(~flip, ref.str.translate(table)), alt.where(~flip, alt.str.translate(table))
    return (ref + '>' + alt).to_numpy(dtype=object)


def mutation_contexts_by_chrom(f_fasta, df, n_up=2, n_down=2, collapse=False, on_device=None):
    """sequence_tools.py:130-177: MUT_TYPE and CONTEXT columns appended to `df` (rows of the chromosome of its first row, in
    order), rows without a context dropped.  f_fasta: a FASTA path or a PackedGenome.  on_device: None = the device form
    unless the process declared itself torch-free (_lib.TORCH_FREE)."""
    genome = load_genome(f_fasta)
    CHROM = str(df.CHROM.iloc[0])
    if not CHROM.startswith('chr'):
        CHROM = "chr{}".format(CHROM)
    _, ctx = _row_contexts(genome, [CHROM] * len(df), df.START.to_numpy(np.int64), df.REF.to_numpy(), n_up, n_down, collapse,
                           _on_device(on_device))
    df.insert(df.shape[1], 'MUT_TYPE', _mut_types(df.REF, df.ALT, collapse))
    df.insert(df.shape[1], 'CONTEXT', ctx)
    return df[df.CONTEXT != ""]


def add_context_to_mutations(f_fasta, df_mut, n_up=2, n_down=2, N_proc=1, collapse=False, on_device=None):
    """sequence_tools.py:179-222: SNV rows (ANNOT not containing INDEL) get MUT_TYPE and CONTEXT chromosome by chromosome
    (CHROM ascending, order kept inside), indel rows ANNOT 'INDEL', their ANNOT as MUT_TYPE and CONTEXT '.'; with any indel the
    frame is sorted by (CHROM, START, END).  All chromosomes go through one kernel call; N_proc is accepted and unused.
    No row in either branch: ValueError (the reference fails with UnboundLocalError)."""
    is_indel = df_mut.ANNOT.str.contains('INDEL')
    df_indel = df_mut[is_indel]
    df_mut = df_mut[~is_indel]
    if len(df_mut) == 0 and len(df_indel) == 0:
        raise ValueError("add_context_to_mutations: no mutation left to annotate")
    if len(df_mut) > 0:
        codes, uniq = pd.factorize(df_mut.CHROM, sort=True)       # groupby('CHROM') order, rows in order inside a group
        keep = np.array(['MT' not in str(u) for u in uniq], bool)
        order = np.argsort(codes, kind='stable')
        order = order[keep[codes[order]]]
        if order.size == 0:
            raise ValueError("add_context_to_mutations: no chromosome left to annotate")
        df = df_mut.iloc[order].copy()
        chroms = np.array(['chr{}'.format(u) if not str(u).startswith('chr') else str(u) for u in uniq], dtype=object)[codes[order]]
        _, ctx = _row_contexts(load_genome(f_fasta), chroms, df.START.to_numpy(np.int64), df.REF.to_numpy(), n_up, n_down, collapse,
                               _on_device(on_device))
        df.insert(df.shape[1], 'MUT_TYPE', _mut_types(df.REF, df.ALT, collapse))
        df.insert(df.shape[1], 'CONTEXT', ctx)
        df_out = df[df.CONTEXT != ""]
    if len(df_indel) > 0:
        print('Adding context to indels')
        df_indel = df_indel.rename({'ANNOT': 'MUT_TYPE'}, axis=1)
        df_indel.insert(df_indel.shape[1] - 1, 'ANNOT', 'INDEL')
        df_indel.insert(df_indel.shape[1], 'CONTEXT', '.')
        if len(df_mut) > 0:
            df_out = pd.concat([df_out, df_indel]).sort_values(['CHROM', 'START', 'END'])
        else:
            df_out = df_indel.sort_values(['CHROM', 'START', 'END'])
    return df_out


def write_mutation_contexts(f_mut, f_fasta, f_out, n_up=1, n_down=1, native=True, on_device=None, timings=None):
    """DigPreprocess.py addMutationContext (:75-100): the 8-column file f_mut annotated with MUT_TYPE and CONTEXT, written to
    f_out (a trailing .gz is dropped; the output is not compressed).  A file pandas would echo unchanged goes through the native
    reader / writer (dig_mutctx_file_*_host) when `native`; anything else through read_mutation_file, add_context_to_mutations
    and to_csv -- the same bytes.  Returns the path taken ('native' or 'pandas'); `timings` (a dict) receives the seconds of the
    parse, kernel and write steps."""
    import ctypes
    import time
    from .. import _lib

    if f_out.endswith('.gz'):
        f_out = f_out[:-3]
    width = mutation_tools._first_row_width(f_mut)
    if width != 8:
        raise ValueError("addMutationContext reads the 8-column mutation file CHROM START END REF ALT SAMPLE GENE ANNOT; "
                         "{} has {} columns".format(f_mut, width))
    timings = {} if timings is None else timings
    dev = _on_device(on_device)
    genome = load_genome(f_fasta)
    t0 = time.perf_counter()
    handle, n_snv, n_indel = ctypes.c_void_p(), ctypes.c_int64(-1), ctypes.c_int64(0)
    if native:
        _lib.call("dig_mutctx_file_parse_host", f_mut.encode(), ctypes.byref(handle), ctypes.byref(n_snv), ctypes.byref(n_indel))
    if n_snv.value < 0:
        df_mut = mutation_tools.read_mutation_file(f_mut, drop_duplicates=False)
        timings['parse'] = time.perf_counter() - t0
        t0 = time.perf_counter()
        df_out = add_context_to_mutations(genome, df_mut, n_up=n_up, n_down=n_down, collapse=False, on_device=dev)
        timings['kernel'] = time.perf_counter() - t0
        t0 = time.perf_counter()
        df_out.to_csv(f_out, sep="\t", index=False, header=False)
        timings['write'] = time.perf_counter() - t0
        return 'pandas'
    try:
        n = n_snv.value
        if n == 0 and n_indel.value == 0:
            raise ValueError("add_context_to_mutations: no mutation left to annotate")
        chrom, start, ref = np.empty(n, np.int32), np.empty(n, np.int64), np.empty(n, np.uint8)
        _lib.call("dig_mutctx_file_fetch_host", handle, _lib.host_ptr(chrom), _lib.host_ptr(start), _lib.host_ptr(ref))
        timings['parse'] = time.perf_counter() - t0
        t0 = time.perf_counter()
        status, code, _, host_ctx = _kernel_rows(genome, chrom, start, ref, n_up, n_down, False, dev)
        host_text = ''.join(host_ctx).encode('ascii')
        host_off = np.zeros(len(host_ctx) + 1, np.int64)
        np.cumsum([len(h) for h in host_ctx], out=host_off[1:])
        timings['kernel'] = time.perf_counter() - t0
        t0 = time.perf_counter()
        _lib.call("dig_mutctx_file_write_host", handle, f_out.encode(), _lib.host_ptr(status), _lib.host_ptr(code),
                  host_text, _lib.host_ptr(host_off), int(n_up), int(n_down))
        timings['write'] = time.perf_counter() - t0
    finally:
        _lib.call("dig_mutctx_file_free_host", handle)
    return 'native'
