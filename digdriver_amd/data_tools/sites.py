"""The sites route's files as integer arrays: what engine.site_counts takes.

mutation_tools.tabulate_nonc_mutations_at_sites (reference mutation_tools.py:233-281) merges a cohort's rows with the sites file on
nine columns, CHROM, START, END, REF, ALT, GENE, ANNOT, MUT_TYPE, CONTEXT.  Here the first two are one integer, pos = CHROM << 40 |
START, and the six labels are one integer, attr: each label column has a dictionary of the values the SITES file holds, and attr is
the mixed-radix number of the six codes -- injective, so equal attr means six equal labels.  A missing label (pandas reads an empty
field, `nan`, `NA`, ... as missing) is a value of its own: the merge pairs missing keys with missing keys.  A label of a mutation row
that the sites file does not hold gives attr -1, which matches nothing.

Both files are read by mutation_tools.read_mutation_file, as the serial route reads them: its rules (column count, autosomes only,
gzip, the indel de-duplication) decide which rows exist.
"""
import numpy as np
import pandas as pd

from . import mutation_tools

LABEL_COLS = ('REF', 'ALT', 'GENE', 'ANNOT', 'MUT_TYPE', 'CONTEXT')
_MISSING = None                     # the dictionaries' key of a missing label


def _need_site_columns(rows, path):
    lacking = [c for c in ('START', 'END') + LABEL_COLS if c not in rows.columns]
    if lacking:
        raise ValueError("{}: no {} column (the sites route needs the 10- or 11-column layout)".format(path, ", ".join(lacking)))


def _positions(rows, path):
    chrom, start = rows.CHROM.to_numpy(np.int64), rows.START.to_numpy(np.int64)
    if len(start) and (start.min() < 0 or start.max() >= (1 << 40)):
        raise ValueError("{}: START within [0, 2^40)".format(path))
    return (chrom << 40) | start


def _codes(column, lookup):
    """The codes of a label column under `lookup` (label -> code, _MISSING -> the code of a missing label); -1 for any other label."""
    codes, uniq = pd.factorize(column.to_numpy(dtype=object), use_na_sentinel=True)
    table = np.array([lookup.get(u, -1) for u in uniq] + [lookup.get(_MISSING, -1)], np.int64)      # (a missing label: code -1, the last entry)
    return table[codes]


def _attr(rows, site_dicts):
    attr, bad = np.zeros(len(rows), np.int64), np.zeros(len(rows), bool)
    radix = 1
    for col in LABEL_COLS:
        code = _codes(rows[col], site_dicts[col])
        bad |= code < 0
        attr += np.where(code < 0, 0, code) * radix
        radix *= max(len(site_dicts[col]), 1)
    attr[bad] = -1
    return attr


def encode_sites_file(f_sites):
    """The sites file -- the mutation-file layout with the element's name in the SAMPLE column; STRAND takes no part in the match -- as
    the site table of engine.site_counts.  A row without an element label is dropped: the reference's groupby('ELT') drops it.
    Returns dict(site_pos, site_end, site_attr i64 [S] and site_elt i32 [S], sorted (stably) by site_pos; elt_names: the E element
    labels in order of first appearance; dicts: column -> {label: code} for REF, ALT, GENE, ANNOT, MUT_TYPE, CONTEXT, a missing
    label under the key None)."""
    rows = mutation_tools.read_mutation_file(f_sites)
    _need_site_columns(rows, f_sites)
    rows = rows.loc[rows.SAMPLE.notna()]
    dicts, radix = {}, 1
    for col in LABEL_COLS:
        codes, uniq = pd.factorize(rows[col].to_numpy(dtype=object), use_na_sentinel=True)
        dicts[col] = {u: i for i, u in enumerate(uniq)}
        if (codes < 0).any():
            dicts[col][_MISSING] = len(uniq)
        radix *= max(len(dicts[col]), 1)
    if radix >= 1 << 62:
        raise ValueError("{}: the six label columns hold too many distinct values for one 62-bit code".format(f_sites))
    elt, elt_names = pd.factorize(rows.SAMPLE.to_numpy(dtype=object))
    pos = _positions(rows, f_sites)
    order = np.argsort(pos, kind="stable")
    c = np.ascontiguousarray
    return dict(site_pos=c(pos[order]), site_end=c(rows.END.to_numpy(np.int64)[order]), site_attr=c(_attr(rows, dicts)[order]),
                site_elt=c(elt.astype(np.int32)[order]), elt_names=list(elt_names), dicts=dicts)


def encode_site_rows(f_mut, site_dicts, cohort_id=0):
    """A cohort's rows as engine.site_counts takes them: the rows of read_mutation_file(f_mut, drop_duplicates=False) with ANNOT !=
    'INDEL' -- SNV duplicates stay and count twice -- under the dictionaries of encode_sites_file.
    Returns dict(pos, end, attr i64 [n]; sample i32: dense ids in order of first appearance (the caller adds the cohort's first global
    sample); cohort i32; sample_names; n_syn: the rows with ANNOT == 'Synonymous' and GENE != 'TP53' of the frame in front of the
    INDEL filter, the numerator of the scale factor, transfer_tools.py:1117-1119).  A row that cannot match (attr -1) and has no
    SAMPLE label is left out; one that could match raises ValueError (the serial route's len(set(x)) over missing values is not
    well defined)."""
    rows = mutation_tools.read_mutation_file(f_mut, drop_duplicates=False)
    _need_site_columns(rows, f_mut)
    n_syn = int(((rows.ANNOT == 'Synonymous') & (rows.GENE != 'TP53')).sum())
    rows = rows.loc[rows.ANNOT != 'INDEL']
    attr = _attr(rows, site_dicts)
    nameless = rows.SAMPLE.isna().to_numpy()
    if (nameless & (attr >= 0)).any():
        raise ValueError("{}: a row that could match a site has no SAMPLE label".format(f_mut))
    rows, attr = rows.loc[~nameless], attr[~nameless]
    sample, sample_names = pd.factorize(rows.SAMPLE.to_numpy(dtype=object))
    c = np.ascontiguousarray
    return dict(pos=c(_positions(rows, f_mut)), end=c(rows.END.to_numpy(np.int64)), attr=c(attr), sample=c(sample.astype(np.int32)),
                cohort=np.full(len(rows), int(cohort_id), np.int32), sample_names=list(sample_names), n_syn=n_syn)
