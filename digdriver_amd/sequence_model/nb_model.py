"""Negative-binomial burden tests -- host mirror of DIGDriver/sequence_model/nb_model.py.

Same names, argument meaning and NaN behaviour as the reference functions; the
arithmetic runs in the HIP kernels of libdig_hip.so (dig_nb.hip / dig_math.hpp).
Inputs may be scalars, numpy arrays, pandas Series (host path: staged through
the *_host entry points) or torch CUDA tensors (device path: no copies, enqueued
on torch's current stream).  There is no CPU fallback.
"""
import numpy as np

from .._marshal import backend_of


def _series_like(*xs):
    for x in xs:
        if type(x).__name__ == "Series":
            return x
    return None


def _elementwise(name, ins, n_out, device):
    """Entry point `name` over the broadcast of `ins` (float64), n_out results of that shape.  Device tensors in -> device tensors
    out; on the host a Series among the inputs gives Series, scalars give floats."""
    be = backend_of(*ins, device=device)
    xs = be.broadcast(ins, "f64")
    shape = tuple(xs[0].shape)
    outs = [be.empty(shape, "f64") for _ in range(n_out)]
    n = 1
    for s in shape:
        n *= s
    be.call(name, *[be.ptr(x) for x in xs], *[be.ptr(o) for o in outs], n)
    if be.is_device:
        return outs
    ser = _series_like(*ins)
    if ser is not None:
        import pandas as pd
        return [pd.Series(o, index=ser.index) for o in outs]
    return outs if shape else [float(o) for o in outs]


def _vec3(name, k, alpha, p, device=0):
    return _elementwise(name, (k, alpha, p), 1, device)[0]


def normal_params_to_gamma(mu, sigma, device=0):
    """nb_model.py:237-241 -- alpha = mu**2 / sigma**2, theta = sigma**2 / mu."""
    return tuple(_elementwise("dig_normal_params_to_gamma", (mu, sigma), 2, device))


def nb_pvalue_greater_midp(k, alpha, p, device=0):
    """UPPER TAIL NB p-value with mid-p correction (nb_model.py:271-278)."""
    return _vec3("dig_nb_midp_upper", k, alpha, p, device)


def nb_pvalue_greater(k, alpha, p, device=0):
    """UPPER TAIL NB p-value (nb_model.py:243-256); vectorised over the reference's scalar form."""
    return _vec3("dig_nb_greater", k, alpha, p, device)


def nb_pvalue_exact(k, alpha, p, mu=None, device=0):
    """Upper or lower tail depending on k vs the expectation (nb_model.py:298-314).
    `mu` other than None/0 is not supported (no live caller passes it)."""
    if mu:
        raise NotImplementedError("explicit mu is not supported; the reference's callers never pass it")
    return _vec3("dig_nb_exact", k, alpha, p, device)


def nb_pvalue_midp(k, alpha, p, mu=None, device=0):
    """Two-sided-by-side mid-p variant (nb_model.py:316-337)."""
    if mu:
        raise NotImplementedError("explicit mu is not supported; the reference's callers never pass it")
    return _vec3("dig_nb_midp_twosided", k, alpha, p, device)


def fisher_combine(p1, p2, device=0):
    """chi2.sf(-2 (ln p1 + ln p2), df=4) (transfer_tools.py:860-861,1086-1087)."""
    return _elementwise("dig_fisher", (p1, p2), 1, device)[0]


def fisher_combine_groups(p, member, device=0):
    """Fisher's method over groups of the rows of p: p [C, E] (or [R, C, E]; a DataFrame's rows are the cohorts), member [M, C] with
    non-zero where row c belongs to group g.  chi2.sf(-2 sum ln p_c, 2 m) over the m members whose p is a number: NaN for m = 0, the
    member's own p for m = 1, fisher_combine of the pair for m = 2 (engine.group_fisher).  f64 [M, E] ([R, M, E]); device tensors in ->
    device tensors out, a DataFrame in -> a DataFrame with its columns."""
    from .. import engine
    is_frame = lambda v: type(v).__name__ == "DataFrame"
    got = engine.group_fisher(p.values if is_frame(p) else p, member.values if is_frame(member) else member, device=device,
                              counts=False)["pval"]
    if is_frame(p):
        import pandas as pd
        return pd.DataFrame(got, columns=p.columns, index=member.index if is_frame(member) else None)
    return got


def nb_critical_count(alpha, p, level, k_max=1 << 20, device=0):
    """The smallest count k in [0, k_max] at which nb_pvalue_greater_midp(k, alpha, p) <= level (one number), per entry of the broadcast
    of alpha and p; -1 where no k <= k_max reaches the level, the statistic is NaN or the level is not inside (0, 1).  The one-array
    convenience of engine.nb_power, called with theta = (1 - p) / p and pi = 1: the kernel's own p = 1 / (theta + 1) then reproduces p
    only to rounding (an ulp or two), so a count whose statistic lies within that of the level may differ; a caller that needs the
    route's bits hands engine.nb_power the route's planes.  i32 of the inputs' shape; device tensors in -> a device tensor out."""
    from .. import engine
    be = backend_of(alpha, p, device=device)
    alpha, p = be.broadcast((alpha, p), "f64")
    got = engine.nb_power(alpha.reshape(-1), ((1.0 - p) / p).reshape(-1), be.broadcast((1.0, alpha), "f64")[0].reshape(-1), level,
                          k_max=k_max, device=device)["k_crit"]
    return got.reshape(tuple(alpha.shape))


class PairTests:
    """What pair_fisher_exact returns for one cohort of H rows: n_row i32 [H] and, per pair i < j at slot pair_index(i, j), n_both
    i32, pval_cooccur and pval_exclusive f64 [H (H - 1) / 2] (row-major upper triangle; arrays or device tensors)."""

    def __init__(self, H, n_samples, got):
        self.H, self.n_samples = H, n_samples
        self.n_row, self.n_both = got["n_row"], got["n_both"]
        self.pval_cooccur, self.pval_exclusive = got["pval_cooccur"], got["pval_exclusive"]

    def pair_index(self, i, j):
        """The slot of the pair of rows i != j (numbers or arrays)."""
        from .. import engine
        i, j = np.minimum(i, j), np.maximum(i, j)
        if np.any(i == j) or np.any(i < 0) or np.any(j >= self.H):
            raise IndexError("a pair is two different rows of 0 .. %d" % (self.H - 1))
        return engine.pair_index(i, j, self.H)


def pair_fisher_exact(rows, n_samples=None, device=0):
    """One-sided Fisher exact tests of co-occurrence and exclusivity for every pair of rows of one cohort's incidence matrix
    (engine.pair_fisher; include/dig_hip.h states the rule).  rows: a bool [H, n] array, DataFrame or tensor (non-zero: the sample
    is in the row) -- or the bit matrix of engine.pair_bits (int64 / uint64 [H, W]) with n_samples given.  n_samples: the universe,
    at least n (samples that no row holds; default n).  pval_cooccur is scipy's fisher_exact(alternative='greater') of the pair's
    2 x 2 table, pval_exclusive its alternative='less'.  Returns PairTests; device tensors in -> device tensors out."""
    from .. import engine
    if type(rows).__name__ == "DataFrame":
        rows = rows.values
    be = backend_of(rows, device=device)
    if getattr(rows, "ndim", None) != 2:
        rows = np.asarray(rows)
    if rows.ndim != 2:
        raise ValueError("rows must be a [H, n] matrix")
    H = int(rows.shape[0])
    if str(rows.dtype).split(".")[-1] in ("int64", "uint64"):
        if n_samples is None:
            raise ValueError("a bit matrix needs n_samples")
        bits = rows
    else:
        n = int(rows.shape[1])
        n_samples = n if n_samples is None else int(n_samples)
        if n_samples < n:
            raise ValueError("n_samples must be at least the matrix's %d columns" % n)
        if be.is_device:
            at = be.torch.nonzero(rows)
            r, s = at[:, 0], at[:, 1]
        else:
            r, s = np.nonzero(rows)
        bits = engine.pair_bits(r, s, H, engine.pair_words(n_samples), device=device)
    return PairTests(H, int(n_samples), engine.pair_fisher(bits, [H], [int(n_samples)], device=device))


# ---------------------------------------------------------------------------------------------
# per-base / tiled route (nb_model.py:126-234, 340-342)
# ---------------------------------------------------------------------------------------------
def _s_prob_table(d_pr, n_up=1, collapse=False):
    """S_prob (dict / Series keyed by the (2 n_up + 1)-mer) -> 4^(2 n_up + 1) values in context index order: 64 for the
    trinucleotide models of the live pipeline, 1 024 for the penta-nucleotide default of the reference's signatures.
    collapse=True (pyrimidine-collapsed contexts: K = 96 substitution types, 32 / 512 contexts): the table holds the C- and
    T-centred windows only; a window centred on A or G is looked up as its reverse complement (seq_to_context,
    sequence_tools.py:42-55) -- expanded here into the full table, so that the kernels look every window up directly."""
    import itertools
    from . import sequence_tools
    keys = ["".join(t) for t in itertools.product("ACGT", repeat=2 * n_up + 1)]
    if collapse:
        keys = [k if k[n_up] in "CT" else sequence_tools.reverse_complement(k) for k in keys]
    try:
        return np.array([float(d_pr[k]) for k in keys])
    except KeyError as exc:
        raise KeyError("S_prob has no entry for context %s (n_up = n_down = %d%s needs all %s%d-mers)" % (
            exc, n_up, ", collapse=True" if collapse else "", "C- and T-centred " if collapse else "", 2 * n_up + 1)) from exc


def _mutation_rows(f_mut, samples=False):
    """The rows a tabix fetch hands to tabix_to_dataframe (nb_model.py:13-33): CHROM, START, END of a bed-like mutation
    file (plain or gzip; 6-9 columns).  samples=True: column 6 as well, the row's sample label ID (as a string, nothing read as a
    missing value); ValueError for a file with fewer than 6 columns."""
    import pandas as pd
    if not samples:
        df = pd.read_csv(f_mut, sep="\t", header=None, usecols=[0, 1, 2], names=["CHROM", "START", "END"], dtype={0: str},
                         comment="#", low_memory=False)
    else:
        try:
            df = pd.read_csv(f_mut, sep="\t", header=None, usecols=[0, 1, 2, 5], dtype={0: str, 5: str}, comment="#", low_memory=False,
                             keep_default_na=False)
        except (ValueError, pd.errors.ParserError) as exc:
            raise ValueError("{}: the sample options read the sample label from column 6, and the file has fewer than 6 "
                             "columns ({})".format(f_mut, exc)) from exc
        df.columns = ["CHROM", "START", "END", "ID"]
    df["CHROM"] = df.CHROM.str.replace("chr", "", regex=False)
    return df


def _sample_ids(muts, what):
    """The sample labels of a cohort's counted rows -> (dense ids int32 per row, the labels in id order).  ValueError for a frame
    without the column ID or a row with an empty label."""
    if "ID" not in muts.columns:
        raise ValueError("{}: the sample options need the sample label of every row (column ID, column 6 of a file)".format(what))
    lab = muts.ID
    empty = lab.isna() | (lab.astype(str).str.strip() == "")
    if bool(empty.any()):
        raise ValueError("{}: {} rows without a sample label in column 6".format(what, int(empty.sum())))
    names, ids = np.unique(lab.astype(str).values, return_inverse=True)
    return ids.astype(np.int32).reshape(-1), list(names)


def sample_keep(n_rows, max_muts_per_sample):
    """keep u8 [S] of --max-muts-per-sample: a sample stays unless its rows (n_rows [S], counted over the cohort's file after the
    "chromosome known to the genome" filter) number MORE than max_muts_per_sample.  None: every sample stays."""
    n_rows = np.asarray(n_rows)
    if max_muts_per_sample is None:
        return np.ones(len(n_rows), np.uint8)
    return (n_rows <= max_muts_per_sample).astype(np.uint8)


def _cohort_rows(f_muts, known, samples, max_muts_per_sample=None):
    """The rows of C mutation files or frames on the chromosomes `known`, as the records cohort_rows stacks: chrom, start, end and,
    with samples, sample (dense per cohort), sample_names and keep (sample_keep of the cohort's own row counts)."""
    import pandas as pd
    rows = []
    for c, f in enumerate(f_muts):
        m = f if isinstance(f, pd.DataFrame) else _mutation_rows(f, samples)
        m = m[m.CHROM.astype(str).str.replace("chr", "", regex=False).isin(known)]
        rec = dict(chrom=m.CHROM.astype(str).values, start=m.START.values, end=m.END.values)
        if samples:
            rec["sample"], rec["sample_names"] = _sample_ids(m, f if isinstance(f, str) else "cohort %d" % c)
            rec["keep"] = sample_keep(np.bincount(rec["sample"], minlength=len(rec["sample_names"])), max_muts_per_sample)
        rows.append(rec)
    return rows


def _sample_arguments(rows, max_muts_per_tile_per_sample, by_sample):
    """The keywords engine.tiled_nb_model takes for the counts by sample, from the records of _cohort_rows(samples=True)."""
    from ..data_tools import cohort_rows
    off = cohort_rows.sample_offsets(rows)
    return dict(mut_sample=cohort_rows.column(rows, "sample", "i32", shift=off), sample_offsets=off,
                keep=cohort_rows.column(rows, "keep", "u8"), cap=max_muts_per_tile_per_sample, by_sample=by_sample)


def _check_sample_options(max_muts_per_sample, max_muts_per_tile_per_sample, by_sample, cut_on="PVAL"):
    """True when any sample option is set (the reader then takes column 6); ValueError for values outside their domains."""
    if max_muts_per_sample is not None and max_muts_per_sample < 0:
        raise ValueError("max_muts_per_sample: a number >= 0")
    cap = max_muts_per_tile_per_sample
    if cap is not None and (int(cap) != cap or cap < 1):
        raise ValueError("max_muts_per_tile_per_sample: an integer >= 1")
    if cut_on not in ("PVAL", "PVAL_SAMPLE"):
        raise ValueError("cut_on: PVAL or PVAL_SAMPLE")
    if cut_on == "PVAL_SAMPLE" and not by_sample:
        raise ValueError("cut_on PVAL_SAMPLE requires by_sample")
    return max_muts_per_sample is not None or cap is not None or bool(by_sample)


def nb_model(d_pr, idx, mu_lst, sigma_lst, f_tabix, f_fasta, n_up=2, n_down=2, binsize=50, collapse=False, device=0,
             max_muts_per_sample=None, max_muts_per_tile_per_sample=None, by_sample=False):
    """nb_model.py:188-234: the tiled NB test over the bins `idx` [(chrom, start, end)] of one cohort; returns the
    reference's frame (CHROM, POS, OBS, EXP, PVAL, Pi, MU, SIGMA, REGION; numeric columns as float, as its np.hstack makes
    them).  `f_tabix`: the cohort's bed-like mutation file (the reference reads it through tabix; here it is joined on the
    GPU in one pass); `f_fasta`: the genome (data_tools.genome.PackedGenome or a FASTA path).  All bins in three launches
    (engine.tiled_nb_model).  n_up = n_down = 2 (penta-nucleotide contexts, the reference's default) or 1 (the trinucleotide
    models every live part of the pipeline trains); collapse=True: S_prob keyed by the pyrimidine-centred contexts (the
    96-substitution model), windows centred on a purine looked up as their reverse complement.
    The sample options (not in the reference; DESIGN.md "Samples in the per-base route") read the sample label from column 6 (ID):
    max_muts_per_sample drops the samples with more rows in the file than that; max_muts_per_tile_per_sample caps what one sample
    adds to a tile's OBS; by_sample adds two columns behind REGION: OBS_SAMPLES (the kept samples with a row in the tile) and
    PVAL_SAMPLE (the same test on OBS_SAMPLES).  Without them the frame, the launches and the columns read are those of today."""
    import pandas as pd
    from .. import engine
    from ..data_tools import genome as genome_mod
    if n_up != n_down or n_up not in (1, 2):
        raise NotImplementedError("the tile kernels take n_up = n_down = 1 or 2")
    samples = _check_sample_options(max_muts_per_sample, max_muts_per_tile_per_sample, by_sample)
    g = f_fasta if isinstance(f_fasta, genome_mod.PackedGenome) else genome_mod.PackedGenome.from_fasta(f_fasta)
    idx = np.asarray(idx)
    chroms = [str(c) for c in idx[:, 0]]
    starts, ends = idx[:, 1].astype(np.int64), idx[:, 2].astype(np.int64)
    known = set(n.replace("chr", "") for n in g.names)
    rows = _cohort_rows([f_tabix], known, samples, max_muts_per_sample)
    extra = _sample_arguments(rows, max_muts_per_tile_per_sample, by_sample) if samples else {}
    m = rows[0]
    res = engine.tiled_nb_model(g, chroms, starts, ends, _s_prob_table(d_pr, n_up, collapse)[None, :], np.asarray(mu_lst, float)[None, :],
                                np.asarray(sigma_lst, float)[None, :], m["chrom"], m["start"], m["end"],
                                np.zeros(len(m["start"]), np.int32), binsize=binsize, device=device, **extra)
    host = {k: v.cpu().numpy() for k, v in res.items()}
    first, nval = host["first_pos"], host["n_valid"].astype(np.int64)
    columns = _TILE_COLUMNS + (_SAMPLE_COLUMNS if by_sample else [])
    if len(idx) == 0 or nval.sum() == 0:
        return pd.DataFrame(columns=columns)
    # all regions at once (the reference appends one block per region): region of every tile, tile number inside it
    reg = np.repeat(np.arange(len(idx)), nval)
    t = np.arange(nval.sum()) - np.repeat(np.cumsum(nval) - nval, nval)
    take = lambda a: a[0][reg, t]
    df = _tile_frame(idx, mu_lst, sigma_lst, first, _region_positions(g, chroms, ends, first, n_up), binsize, reg, t,
                     take(host["k"]), take(host["exp"]), take(host["pval"]), take(host["pt"]))
    if by_sample:
        df["OBS_SAMPLES"], df["PVAL_SAMPLE"] = take(host["k_samples"]).astype(float), take(host["pval_sample"])
    return df


_TILE_COLUMNS = ["CHROM", "POS", "OBS", "EXP", "PVAL", "Pi", "MU", "SIGMA", "REGION"]
_SAMPLE_COLUMNS = ["OBS_SAMPLES", "PVAL_SAMPLE"]      # behind the reference's columns, in front of QVAL; only with by_sample


def _region_positions(g, chroms, ends, first, n_up):
    """The positions every region has from its first one on (a window must fit in front of the chromosome's end)."""
    return np.minimum(ends, np.array([g.lengths[i] for i in g.chrom_index(chroms)], np.int64) - n_up) - first


def _tile_frame(idx, mu, sigma, first, n_pos, binsize, reg, t, obs, exp, pval, pi):
    """Rows of the reference's frame (nb_model.py:141-186) for the tiles (reg[i], t[i]) of one cohort, from host arrays: idx
    [R, 3], mu, sigma, first, n_pos [R]; obs, exp, pval, pi: the tiles' values.  What nb_model builds for every tile and
    nb_model_hits for the hits."""
    import pandas as pd
    idx, reg, t = np.asarray(idx), np.asarray(reg, np.int64), np.asarray(t, np.int64)
    lo = np.asarray(first)[reg] + t * binsize
    hi = np.minimum(lo + binsize, (np.asarray(first) + np.asarray(n_pos))[reg]) - 1
    used, inv = np.unique(reg, return_inverse=True)          # (a label per region that has a row: a hit list names few regions)
    labels = np.array(["{}:{}-{}".format(c, s_, e) for c, s_, e in idx[used]], dtype=object)
    return pd.DataFrame({
        "CHROM": idx[reg, 0].astype(float), "POS": (lo + hi) / 2.0 if binsize > 1 else lo.astype(float),
        "OBS": np.asarray(obs).astype(float), "EXP": np.asarray(exp, float), "PVAL": np.asarray(pval, float), "Pi": np.asarray(pi, float),
        "MU": np.asarray(mu, float)[reg], "SIGMA": np.asarray(sigma, float)[reg],
        "REGION": labels[inv.reshape(-1)] if len(reg) else np.empty(0, object)})[_TILE_COLUMNS]


def bh_cut(p, q, fdr):
    """p*: the largest p-value of a list whose Benjamini-Hochberg q-value is <= fdr; below 0 when there is none.  q is a
    non-decreasing step function of p (tied p-values share one q), so {q <= fdr} = {p <= p*}.  p, q: one cohort's testable
    p-values and their q-values in any common order, numpy arrays or tensors."""
    sel = q <= fdr
    return float(p[sel].max()) if bool(sel.any()) else -1.0


def hits_q_values(p_hits, n):
    """The q-values, in a list of n testable p-values, of the hits {p <= p*} of bh_cut, from the hits alone: statsmodels'
    operations (get_q_vals) with the ranks of the hits and the length of the whole list.  The same bits as the whole list gives:
    ascending, the hits are the list's head with their own ranks, and the running minimum that arrives from behind the cut is a q
    above fdr, which every hit's own q lies below."""
    p = np.asarray(p_hits, dtype=np.float64)
    if p.size == 0:
        return p.copy()
    order = np.argsort(p, kind="stable")
    q = p[order] / (np.arange(1, p.size + 1) / float(n))
    q = np.minimum(np.minimum.accumulate(q[::-1])[::-1], 1.0)
    out = np.empty_like(q)
    out[order] = q
    return out


def _fdr_cuts(pval, n_valid, fdr):
    """Per cohort (p*, the number of testable tiles) for BH q <= fdr over the cohort's TESTABLE tiles -- the existing tiles with a
    non-NaN p-value: the ragged lists come from engine.tile_select at cut = +inf (the plane as it lies when every tile is
    testable), their q-values from bh_ragged; no q plane is kept."""
    import torch
    from .. import engine
    C, R, T = pval.shape
    if R and T and int(n_valid.min()) >= T and not bool(torch.isnan(pval).any()):
        lists, ptr = pval.reshape(-1), np.arange(C + 1, dtype=np.int64) * (R * T)
    else:
        got = engine.tile_select(pval, n_valid, float("inf"), index=False)
        lists, ptr = got["score"], got["cohort_ptr"]
    cuts = np.full(C, -1.0)
    if lists.numel():
        q, _ = bh_ragged(lists, ptr)
        for c in range(C):
            cuts[c] = bh_cut(lists[ptr[c]:ptr[c + 1]], q[ptr[c]:ptr[c + 1]], fdr)
    return cuts, np.diff(ptr)


def nb_model_hits(d_prs, idx, mu, sigma, f_muts, f_fasta, n_up=2, n_down=2, binsize=50, collapse=False, pval_max=None, fdr=None,
                  device=0, max_muts_per_sample=None, max_muts_per_tile_per_sample=None, by_sample=False, cut_on="PVAL"):
    """The rows of nb_model's frame that pass a cut, for C cohorts on one bin grid, without building the frame: frame c equals
    nb_model(d_prs[c], idx, mu[c], sigma[c], f_muts[c], ...) filtered by PVAL <= pval_max, or by q <= fdr -- bit for bit, in
    order, with the rows' numbers in that full frame as the (int64) index.  Exactly one of pval_max / fdr.
    fdr: Benjamini-Hochberg over the cohort's TESTABLE tiles, the existing tiles with a non-NaN p-value (a tile whose positions
    are all non-ACGT has Pi = 0 and a NaN p-value, and one NaN makes every q-value of get_q_vals NaN): q = get_q_vals of
    frame.PVAL.dropna(); the frame then has a QVAL column as well.
    d_prs: C S_prob mappings; mu, sigma [C, R]; f_muts: C bed-like mutation files or frames (as nb_model's f_tabix).
    One engine.tiled_nb_model call over all cohorts, the selection (engine.tile_select) on the device; only the hits come back.
    The four planes take 28 bytes per (tile, cohort), fdr adds 8 for the lists and the sort's workspace; regions are NOT chunked:
    the caller passes as many regions as fit.  frame.attrs holds n_testable and n_tiles of the cohort.
    The sample options as nb_model takes them; cut_on: the score that pval_max / fdr select on, PVAL or (with by_sample) PVAL_SAMPLE
    -- the testable tiles, the Benjamini-Hochberg pass, QVAL and n_testable then belong to that score.  OBS_SAMPLES and PVAL_SAMPLE
    stand behind REGION, in front of QVAL."""
    if (pval_max is None) == (fdr is None):
        raise ValueError("exactly one of pval_max and fdr must be given")
    if n_up != n_down or n_up not in (1, 2):
        raise NotImplementedError("the tile kernels take n_up = n_down = 1 or 2")
    samples = _check_sample_options(max_muts_per_sample, max_muts_per_tile_per_sample, by_sample, cut_on)
    import pandas as pd
    from .. import engine
    from ..data_tools import cohort_rows, genome as genome_mod
    C = len(d_prs)
    f_muts = list(f_muts)
    idx = np.asarray(idx)
    R = len(idx)
    mu, sigma = np.asarray(mu, float).reshape(C, R), np.asarray(sigma, float).reshape(C, R)
    if len(f_muts) != C:
        raise ValueError("one mutation file per cohort: %d files for %d cohorts" % (len(f_muts), C))
    g = f_fasta if isinstance(f_fasta, genome_mod.PackedGenome) else genome_mod.PackedGenome.from_fasta(f_fasta)
    chroms = [str(c) for c in idx[:, 0]] if R else []
    starts, ends = (idx[:, 1].astype(np.int64), idx[:, 2].astype(np.int64)) if R else (np.zeros(0, np.int64),) * 2
    known = set(n.replace("chr", "") for n in g.names)
    rows = _cohort_rows(f_muts, known, samples, max_muts_per_sample)
    extra = _sample_arguments(rows, max_muts_per_tile_per_sample, by_sample) if samples else {}
    mc, ms, me = cohort_rows.column(rows, "chrom"), cohort_rows.column(rows, "start", "i64"), cohort_rows.column(rows, "end", "i64")
    co = cohort_rows.cohort_column(rows, "start")
    s_prob = np.stack([_s_prob_table(d, n_up, collapse) for d in d_prs])
    res = engine.tiled_nb_model(g, chroms, starts, ends, s_prob, mu, sigma, mc, ms, me, co, binsize=binsize, device=device, **extra)
    nval_dev = res["n_valid"]
    score = res["pval_sample" if cut_on == "PVAL_SAMPLE" else "pval"]
    if fdr is not None:
        cuts, n_test = _fdr_cuts(score, nval_dev, fdr)
    else:
        cuts = np.full(C, float(pval_max))
        n_test = engine.tile_select_counts(score, nval_dev, float("inf")).sum(dim=1).cpu().numpy()
    hits = engine.tile_select(score, nval_dev, cuts, pt=res["pt"], exp=res["exp"], k=res["k"])
    ptr = hits.pop("cohort_ptr")
    if by_sample:
        # the planes tile_select does not gather, taken at the hits' (cohort, region, tile) (not a hot path: the hits are few)
        import torch
        at = (torch.as_tensor(np.repeat(np.arange(C), np.diff(ptr)), device=score.device), hits["region"].long(), hits["tile"].long())
        hits.update(pval=res["pval"][at], k_samples=res["k_samples"][at], pval_sample=res["pval_sample"][at])
    hits = {k: v.cpu().numpy() for k, v in hits.items()}
    hits.setdefault("pval", hits["score"])                     # (without by_sample the score is PVAL)
    first, nval = res["first_pos"].cpu().numpy(), np.maximum(res["n_valid"].cpu().numpy().astype(np.int64), 0)
    n_pos = _region_positions(g, chroms, ends, first, n_up) if R else np.zeros(0, np.int64)
    row0 = np.cumsum(nval) - nval                              # a region's first row in the full frame
    frames = []
    for c in range(C):
        sel = slice(int(ptr[c]), int(ptr[c + 1]))
        reg, t = hits["region"][sel].astype(np.int64), hits["tile"][sel].astype(np.int64)
        df = _tile_frame(idx, mu[c], sigma[c], first, n_pos, binsize, reg, t, hits["k"][sel], hits["exp"][sel], hits["pval"][sel],
                         hits["pt"][sel])
        if by_sample:
            df["OBS_SAMPLES"], df["PVAL_SAMPLE"] = hits["k_samples"][sel].astype(float), hits["pval_sample"][sel]
        if fdr is not None:
            df["QVAL"] = hits_q_values(hits["score"][sel], int(n_test[c]))
        df.index = pd.Index(row0[reg] + t, dtype=np.int64)
        df.attrs.update(n_testable=int(n_test[c]), n_tiles=int(nval.sum()))
        frames.append(df)
    return frames


# ---------------------------------------------------------------------------------------------
# sliding windows of consecutive tiles (DESIGN.md "Sliding windows in the per-base route")
# ---------------------------------------------------------------------------------------------
_WINDOW_COLUMNS = ["WIDTH", "PEAK"]                    # behind the reference's columns, in front of QVAL
_SAMPLE_WINDOW_PLANES = ("k_samples", "pval_sample")   # what window_samples gathers at the hits: OBS_SAMPLES, PVAL_SAMPLE, in front of WIDTH


def _check_widths(widths):
    """The window widths of nb_model_window_hits as a list of ints, in the order given; ValueError for none, for one that is not an
    integer >= 1 and for one given twice."""
    try:
        given = list(widths)
    except TypeError:
        given = [widths]
    if not given:
        raise ValueError("widths: at least one window width")
    out = []
    for w in given:
        if isinstance(w, (bool, np.bool_)) or not isinstance(w, (int, np.integer, float, np.floating)) or w != w or int(w) != w or w < 1:
            raise ValueError("widths: every width an integer >= 1 (got %r)" % (w,))
        if int(w) in out:
            raise ValueError("widths: width %d is given twice" % int(w))
        out.append(int(w))
    return out


def window_peaks(region, tile, score, width):
    """PEAK of the hits of one cohort at one width (host arrays, one entry per hit): inside every region the hits are walked in the
    order of (score, tile); a hit is a peak unless a hit already marked as a peak overlaps it, |t1 - t2| < width.  Returns bool [hits]."""
    region, tile, score = np.asarray(region, np.int64), np.asarray(tile, np.int64), np.asarray(score, float)
    peak = np.zeros(len(tile), bool)
    taken = {}                                          # region -> the tiles of its peaks
    for i in np.lexsort((tile, score)):                 # (score first, then tile; regions do not interact)
        mine = taken.setdefault(int(region[i]), [])
        if all(abs(int(tile[i]) - t) >= width for t in mine):
            peak[i] = True
            mine.append(int(tile[i]))
    return peak


def nb_model_window_hits(d_prs, idx, mu, sigma, f_muts, f_fasta, n_up=2, n_down=2, binsize=50, widths=(2,), collapse=False, pval_max=None,
                         fdr=None, device=0, max_muts_per_sample=None, max_muts_per_tile_per_sample=None, by_sample=False, cut_on="PVAL",
                         window_samples=False):
    """nb_model_hits over every window of m consecutive tiles, for each m of `widths`: "any m binsize consecutive positions of a
    region" instead of the tiles of one grid.  One base_tile_probs and one counting pass (tile_mut_counts, or tile_sample_counts with
    max_muts_per_sample / max_muts_per_tile_per_sample: OBS is then the capped count) over all cohorts; the base test is not run.  Per
    width, in the order given: one engine.tile_window_test into planes that are reused from width to width, then the selection of
    nb_model_hits (engine.tile_select, _fdr_cuts) with n_windows in the place of n_valid.
    Window t of a region covers its tiles t .. t + m - 1; a region with fewer than m tiles has one window over all of them.
    Returns C frames; rows by width as given, then as nb_model_hits orders them.  Columns: the reference's nine (POS: the middle of
    the window's positions, (lo + hi) / 2 with hi cut at the region's last position; Pi, OBS, EXP, PVAL: the window's), WIDTH (hi -
    lo + 1), PEAK (window_peaks per cohort, width and region), and QVAL with fdr: Benjamini-Hochberg per cohort and PER WIDTH over that
    width's testable windows.  The index is the row number in the full frame of that width (the exclusive cumulative sum of n_windows,
    plus t); attrs n_testable and n_windows hold one entry per width.
    window_samples (DESIGN.md "Samples in sliding windows"; the sample label is read from column 6, as by the other sample options):
    the keys of the counting pass are kept, re-keyed sample-major and sorted once; per width engine.tile_window_samples counts the
    DISTINCT kept samples with a counted row in the window (one sample with rows in ten tiles of a window is one sample) into one
    reused plane, and engine.tiled_nb_test runs on (the window's Pi, that count).  The frames gain OBS_SAMPLES and PVAL_SAMPLE
    behind REGION, in front of WIDTH.  cut_on="PVAL_SAMPLE" (only with window_samples) selects on that score: the testable windows,
    Benjamini-Hochberg, QVAL, n_testable and PEAK then belong to it.  OBS stays the (capped) row count.
    ValueError before any device work: by_sample, or cut_on other than PVAL without window_samples (the distinct samples of a window
    are not the sum of its tiles'; window_samples counts them), an empty widths, a width that is not an integer >= 1 or above
    engine.TILE_WINDOW_MAX_WIDTH, a width given twice."""
    if (pval_max is None) == (fdr is None):
        raise ValueError("exactly one of pval_max and fdr must be given")
    if by_sample or (cut_on != "PVAL" and not window_samples):
        raise ValueError("windows take no by_sample and no cut_on other than PVAL: the distinct samples of a window are not the sum "
                         "of its tiles' samples (window_samples=True counts them and takes cut_on PVAL_SAMPLE)")
    if cut_on not in ("PVAL", "PVAL_SAMPLE"):
        raise ValueError("cut_on: PVAL or PVAL_SAMPLE")
    widths = _check_widths(widths)
    from .. import engine
    if max(widths) > engine.TILE_WINDOW_MAX_WIDTH:
        raise ValueError("widths: at most %d tiles" % engine.TILE_WINDOW_MAX_WIDTH)
    if n_up != n_down or n_up not in (1, 2):
        raise NotImplementedError("the tile kernels take n_up = n_down = 1 or 2")
    samples = _check_sample_options(max_muts_per_sample, max_muts_per_tile_per_sample, False) or bool(window_samples)
    import pandas as pd
    from ..data_tools import cohort_rows, genome as genome_mod
    C = len(d_prs)
    f_muts = list(f_muts)
    idx = np.asarray(idx)
    R = len(idx)
    mu, sigma = np.asarray(mu, float).reshape(C, R), np.asarray(sigma, float).reshape(C, R)
    if len(f_muts) != C:
        raise ValueError("one mutation file per cohort: %d files for %d cohorts" % (len(f_muts), C))
    g = f_fasta if isinstance(f_fasta, genome_mod.PackedGenome) else genome_mod.PackedGenome.from_fasta(f_fasta)
    chroms = [str(c) for c in idx[:, 0]] if R else []
    starts, ends = (idx[:, 1].astype(np.int64), idx[:, 2].astype(np.int64)) if R else (np.zeros(0, np.int64),) * 2
    known = set(n.replace("chr", "") for n in g.names)
    rows = _cohort_rows(f_muts, known, samples, max_muts_per_sample)
    mc, ms, me = cohort_rows.column(rows, "chrom"), cohort_rows.column(rows, "start", "i64"), cohort_rows.column(rows, "end", "i64")
    co = cohort_rows.cohort_column(rows, "start")
    s_prob = np.stack([_s_prob_table(d, n_up, collapse) for d in d_prs])
    # the front half, once for every width
    pt, first_d, nval_d = engine.base_tile_probs(g, chroms, starts, ends, s_prob, binsize, device=device)
    T = int(pt.shape[2])
    if samples:
        sa = _sample_arguments(rows, max_muts_per_tile_per_sample, False)
        k, _, keys = engine.tile_sample_counts(g, chroms, starts, ends, first_d, nval_d, mc, ms, me, co, sa["mut_sample"],
                                               sa["sample_offsets"], sa["keep"], sa["cap"], C, binsize, T, return_keys=True)
        if window_samples:
            n_samples = int(sa["sample_offsets"][-1])
            keys = engine.tile_window_sample_keys(keys, C, R, T, n_samples)        # sample-major, sorted: once for every width
    else:
        k = engine.tile_mut_counts(g, chroms, starts, ends, first_d, nval_d, mc, ms, me, co, C, binsize, T)
    first, nval = first_d.cpu().numpy(), np.clip(nval_d.cpu().numpy().astype(np.int64), 0, T)
    n_pos = _region_positions(g, chroms, ends, first, n_up) if R else np.zeros(0, np.int64)
    last = first + n_pos                                       # one past a region's last position
    planes = s_w = None
    per_width = []                                             # (m, hits as host arrays, cohort_ptr, n_testable [C], n_windows [R])
    for m in widths:
        planes = engine.tile_window_test(pt, k, mu, sigma, nval_d, m, device=device, out=planes)
        nwin_d = planes["n_windows"]
        score = planes["pval"]
        if window_samples:
            s_w = engine.tile_window_samples(keys, nval_d, C, R, T, n_samples, m, device=device, out=s_w)
            pval_s = engine.tiled_nb_test(planes["pt"], s_w, mu, sigma, device=device)[0]
            score = pval_s if cut_on == "PVAL_SAMPLE" else score
        if fdr is not None:
            cuts, n_test = _fdr_cuts(score, nwin_d, fdr)
        else:
            cuts = np.full(C, float(pval_max))
            n_test = engine.tile_select_counts(score, nwin_d, float("inf")).sum(dim=1).cpu().numpy()
        hits = engine.tile_select(score, nwin_d, cuts, pt=planes["pt"], exp=planes["exp"], k=planes["k"])
        ptr = hits.pop("cohort_ptr")
        if window_samples:
            # the planes tile_select does not gather, taken at the hits' (cohort, region, tile), as nb_model_hits does
            import torch
            at = (torch.as_tensor(np.repeat(np.arange(C), np.diff(ptr)), device=score.device), hits["region"].long(), hits["tile"].long())
            hits.update(pval=planes["pval"][at], k_samples=s_w[at], pval_sample=pval_s[at])
        per_width.append((m, {name: v.cpu().numpy() for name, v in hits.items()}, ptr, np.asarray(n_test), nwin_d.cpu().numpy().astype(np.int64)))
    frames = []
    for c in range(C):
        cols = {name: [] for name in ("reg", "t", "k", "exp", "pval", "pt", "lo", "hi", "peak", "q", "row", "k_samples", "pval_sample")}
        for m, hits, ptr, n_test, nwin in per_width:
            sel = slice(int(ptr[c]), int(ptr[c + 1]))
            reg, t, score = hits["region"][sel].astype(np.int64), hits["tile"][sel].astype(np.int64), hits["score"][sel]
            lo = first[reg] + t * binsize
            hi = np.minimum(lo + np.minimum(m, nval[reg] - t) * binsize, last[reg]) - 1
            cols["reg"].append(reg), cols["t"].append(t), cols["lo"].append(lo), cols["hi"].append(hi)
            cols["k"].append(hits["k"][sel]), cols["exp"].append(hits["exp"][sel]), cols["pt"].append(hits["pt"][sel])
            cols["pval"].append(hits["pval"][sel] if window_samples else score)      # (without window_samples the score is PVAL)
            for name in _SAMPLE_WINDOW_PLANES if window_samples else ():
                cols[name].append(hits[name][sel])
            cols["peak"].append(window_peaks(reg, t, score, m))
            cols["q"].append(hits_q_values(score, int(n_test[c])) if fdr is not None else score)
            cols["row"].append((np.cumsum(nwin) - nwin)[reg] + t)
        cat = {name: np.concatenate(v) for name, v in cols.items() if v}
        df = _tile_frame(idx, mu[c], sigma[c], first, n_pos, binsize, cat["reg"], cat["t"], cat["k"], cat["exp"], cat["pval"], cat["pt"])
        df["POS"] = (cat["lo"] + cat["hi"]) / 2.0
        if window_samples:
            df["OBS_SAMPLES"], df["PVAL_SAMPLE"] = cat["k_samples"].astype(float), cat["pval_sample"]
        df["WIDTH"], df["PEAK"] = (cat["hi"] - cat["lo"] + 1).astype(float), cat["peak"].astype(bool)
        if fdr is not None:
            df["QVAL"] = cat["q"]
        df.index = pd.Index(cat["row"], dtype=np.int64)
        df.attrs.update(n_testable=[int(w[3][c]) for w in per_width], n_windows=[int(w[4].sum()) for w in per_width])
        frames.append(df)
    return frames


# ---------------------------------------------------------------------------------------------
# the per-base scan over the mutated tiles only (DESIGN.md "Sparse per-base scan")
# ---------------------------------------------------------------------------------------------
ZERO_FLOOR_MARGIN = 4e-6       # p-values are pinned to 1e-6 relative, pt to 1e-12: both sides' error twice over


def _one_cut(pval_max, fdr, bonferroni):
    if sum(x is not None for x in (pval_max, fdr, bonferroni)) != 1:
        raise ValueError("exactly one of pval_max, fdr and bonferroni must be given")
    if bonferroni is not None and not 0.0 < bonferroni <= 1.0:
        raise ValueError("bonferroni: a level within (0, 1]")


def testable_regions(mu, sigma):
    """[C, R] bool: the (cohort, region) rows whose empty tiles with pt > 0 have a p-value -- the NaN rule of nb_exact
    (csrc/dig_math.hpp) at k = 0: alpha = mu^2 / sigma^2 must be a finite number > 0 and theta = sigma^2 / mu a number > 0.  (mu NaN,
    0 or negative, sigma NaN, 0 or infinite: k = 0 is then not below the NB mean, the upper tail is betainc(0, alpha, .) = NaN.)"""
    mu, sigma = np.asarray(mu, float), np.asarray(sigma, float)
    with np.errstate(all="ignore"):
        alpha, theta = (mu * mu) / (sigma * sigma), (sigma * sigma) / mu
    return np.isfinite(alpha) & (alpha > 0) & (theta > 0)


def zero_tile_floor(denom, smax, smin_pos, mu, sigma, binsize, n_positive=None):
    """floor [C]: a lower bound of the p-value of every EMPTY testable tile of a cohort, from the region denominators alone.  An
    empty tile below the NB mean has PVAL = P(X = 0) = (1 + theta pt)^(-alpha), which falls as pt grows, and no tile's pt exceeds
    u = min(1, binsize smax[c] / denom[c, r]): floor[c] = min over the testable regions with denom > 0 of (1 + theta u)^(-alpha);
    +inf for a cohort without such a region (it has no empty testable tile).
    denom, n_positive: host arrays or device tensors as engine.tile_census returns them (the arithmetic then runs where they lie:
    at 200 000 regions x 37 cohorts numpy took 0.2 s of a 0.27 s scan); floor comes back as a host array.
    Also returns testable [C, R] (testable_regions, on the same side as denom) and checks the other end: the smallest positive pt a region can hold,
    smin_pos[c] / denom[c, r], must still give p = 1 / (theta pt + 1) < 1 and an NB mean > 0 -- else a tile with pt > 0 would have
    a NaN p-value in the dense route (p rounds to 1) and the census could not count the testable tiles: ValueError."""
    be = backend_of(denom, n_positive)
    x = be.torch if be.is_device else np                     # (the few operations below have one spelling in both)
    denom = be.arr(denom, "f64")
    C, R = denom.shape
    mu, sigma = be.arr(mu, "f64", (C, R)), be.arr(sigma, "f64", (C, R))
    smax, smin_pos = be.arr(smax, "f64", (C, 1)), be.arr(smin_pos, "f64", (C, 1))
    with np.errstate(all="ignore"):
        alpha, theta = (mu * mu) / (sigma * sigma), (sigma * sigma) / mu
        testable = x.isfinite(alpha) & (alpha > 0) & (theta > 0)              # (testable_regions)
        ok = testable & (denom > 0)
        ratio = binsize * smax / denom
        u = x.where(ratio < 1.0, ratio, x.ones_like(ratio))
        f = x.exp(-alpha * x.log1p(theta * u))
        p_low = 1.0 / (theta * (smin_pos / denom) + 1.0)
        lost = ok & ~((p_low < 1.0) & (alpha * (1.0 - p_low) / p_low > 0))
    if n_positive is not None:
        lost = lost & (be.arr(n_positive, None, (C, R)) > 0)
    if bool(lost.any()):
        c, r = np.argwhere(lost.cpu().numpy() if be.is_device else lost)[0]
        raise ValueError("cohort %d, region %d: theta pt of the smallest tile probability is below the rounding of 1 / (theta pt + 1): "
                         "the testable tiles cannot be counted without evaluating every tile (use nb_model_hits)" % (c, r))
    if R == 0:
        return np.full(C, np.inf), testable
    floor = x.amin(x.where(ok, f, x.full_like(f, float("inf"))), 1)
    return (floor.cpu().numpy() if be.is_device else floor), testable


def nb_model_hits_sparse(d_prs, idx, mu, sigma, f_muts, f_fasta, n_up=2, n_down=2, binsize=1, collapse=False, pval_max=None, fdr=None,
                         bonferroni=None, device=0):
    """nb_model_hits over the tiles that hold a mutation row, and no other: memory and work follow the rows and C R, no [C, R, T]
    array is allocated.  Exactly one of pval_max / fdr / bonferroni (cut = bonferroni / n_testable of the cohort).  Frames as
    nb_model_hits makes them (columns, dtypes, row order, int64 index = the row number in the full dense frame; QVAL with fdr;
    attrs n_testable and n_tiles), with two more attrs:
      zero_floor  a lower bound of the p-value of every empty testable tile of the cohort (zero_tile_floor);
      complete    zero_floor (1 - 4e-6) > cut: no empty tile can be a hit, the frame is ALL of the dense hits.  When it is false the
                  frame is the dense hits with OBS >= 1 (pval_max, bonferroni).
    fdr: every cohort must be complete at cut = fdr, else ValueError (naming the cohorts, their floors and fdr) before any tile is
    tested; the frames are then exactly the dense ones: every p <= fdr belongs to a mutated tile and holds its rank, and the
    Benjamini-Hochberg pivot p_(j) <= fdr j / m <= fdr < floor is no empty tile.
    n_testable is the dense route's: the tiles with pt > 0 of the testable regions (engine.tile_census counts them), plus the
    mutated tiles outside that set whose p-value is a number (a row on a tile of windows with an N: Pi = 0, PVAL = 0)."""
    _one_cut(pval_max, fdr, bonferroni)
    if n_up != n_down or n_up not in (1, 2):
        raise NotImplementedError("the tile kernels take n_up = n_down = 1 or 2")
    import pandas as pd
    from .. import engine
    from ..data_tools import cohort_rows, genome as genome_mod
    C = len(d_prs)
    f_muts = list(f_muts)
    idx = np.asarray(idx)
    R = len(idx)
    mu, sigma = np.asarray(mu, float).reshape(C, R), np.asarray(sigma, float).reshape(C, R)
    if len(f_muts) != C:
        raise ValueError("one mutation file per cohort: %d files for %d cohorts" % (len(f_muts), C))
    s_prob = np.stack([_s_prob_table(d, n_up, collapse) for d in d_prs]) if C else np.zeros((0, 4 ** (2 * n_up + 1)))
    if (s_prob < 0).any():
        raise ValueError("S_prob: a negative entry (cohort %d)" % int(np.argwhere(s_prob < 0)[0][0]))
    starts, ends = (idx[:, 1].astype(np.int64), idx[:, 2].astype(np.int64)) if R else (np.zeros(0, np.int64),) * 2
    engine.check_tile_regions(starts, ends, n_up)
    g = f_fasta if isinstance(f_fasta, genome_mod.PackedGenome) else genome_mod.PackedGenome.from_fasta(f_fasta)
    chroms = [str(c) for c in idx[:, 0]] if R else []
    known = set(n.replace("chr", "") for n in g.names)
    rows = _cohort_rows(f_muts, known, False)
    mc, ms, me = cohort_rows.column(rows, "chrom"), cohort_rows.column(rows, "start", "i64"), cohort_rows.column(rows, "end", "i64")
    co = cohort_rows.cohort_column(rows, "start")
    first_d, nval_d, denom_d, npos_d = engine.tile_census(g, chroms, starts, ends, s_prob, binsize, device=device)
    first, nval = first_d.cpu().numpy(), np.maximum(nval_d.cpu().numpy().astype(np.int64), 0)
    smax = s_prob.max(axis=1) if C else np.zeros(0)
    smin = np.where(s_prob > 0, s_prob, np.inf).min(axis=1) if C else np.zeros(0)
    floor, testable_d = zero_tile_floor(denom_d, smax, smin, mu, sigma, binsize, npos_d)
    n_census = (npos_d.long() * testable_d).sum(dim=1).cpu().numpy() if R else np.zeros(C, np.int64)
    testable = testable_d.cpu().numpy()
    if fdr is not None:
        bad = [c for c in range(C) if not floor[c] * (1.0 - ZERO_FLOOR_MARGIN) > fdr]
        if bad:
            raise ValueError("fdr = %g: no certificate that an empty tile is no hit for cohorts %s (zero-tile floors %s): a smaller fdr, "
                             "a smaller binsize, or nb_model_hits" % (fdr, bad, ["%.3g" % floor[c] for c in bad]))
    n_tiles = int(max(1, -(-int((ends - starts).max() if R else 1) // int(binsize))))
    res = engine.sparse_tile_test(g, chroms, starts, ends, s_prob, binsize, n_tiles, first_d, nval_d, denom_d, mu, sigma, mc, ms, me, co)
    p_dev = res["pval"]
    tiles = {k: v.cpu().numpy() for k, v in res.items()}
    tc, tr = tiles["cohort"].astype(np.int64), tiles["region"].astype(np.int64)
    number = ~np.isnan(tiles["pval"])
    counted = testable[tc, tr] & (tiles["pt"] > 0) if len(tc) else np.zeros(0, bool)       # (the census has these tiles already)
    n_test = n_census + np.bincount(tc[number & ~counted], minlength=C)[:C]
    ptr = np.searchsorted(tc, np.arange(C + 1))                       # (the tiles lie cohort-major)
    if fdr is not None:
        cuts = np.full(C, -1.0)
        if number.any():
            # the mutated tiles' testable p-values, ranked in a list of n_testable: every rank up to the pivot is theirs
            import torch
            keep = torch.as_tensor(number, device=p_dev.device)
            lists, lptr = p_dev[keep].contiguous(), np.searchsorted(tc[number], np.arange(C + 1)).astype(np.int64)
            q, _ = bh_ragged(lists, lptr, n_global=np.maximum(n_test, 1).astype(np.float64))
            for c in range(C):
                cuts[c] = bh_cut(lists[lptr[c]:lptr[c + 1]], q[lptr[c]:lptr[c + 1]], fdr)
        level = np.full(C, float(fdr))
    elif bonferroni is not None:
        cuts = level = float(bonferroni) / np.maximum(n_test, 1)
    else:
        cuts = level = np.full(C, float(pval_max))
    n_pos = _region_positions(g, chroms, ends, first, n_up) if R else np.zeros(0, np.int64)
    row0 = np.cumsum(nval) - nval
    frames = []
    for c in range(C):
        sel = np.arange(ptr[c], ptr[c + 1])
        sel = sel[tiles["pval"][sel] <= cuts[c]]                       # (a NaN never passes)
        reg, t = tr[sel], tiles["tile"][sel].astype(np.int64)
        df = _tile_frame(idx, mu[c], sigma[c], first, n_pos, binsize, reg, t, tiles["k"][sel], tiles["exp"][sel], tiles["pval"][sel],
                         tiles["pt"][sel])
        if fdr is not None:
            df["QVAL"] = hits_q_values(tiles["pval"][sel], int(n_test[c]))
        df.index = pd.Index(row0[reg] + t, dtype=np.int64)
        df.attrs.update(n_testable=int(n_test[c]), n_tiles=int(nval.sum()), zero_floor=float(floor[c]),
                        complete=bool(floor[c] * (1.0 - ZERO_FLOOR_MARGIN) > level[c]))
        frames.append(df)
    return frames


def nb_model_window_hits_sparse(d_prs, idx, mu, sigma, f_muts, f_fasta, n_up=2, n_down=2, binsize=1, widths=(2,), collapse=False,
                                pval_max=None, fdr=None, bonferroni=None, device=0, chunk_windows=None):
    """nb_model_window_hits over the windows that hold a mutation row, and no other (DESIGN.md "Sparse sliding windows"): memory and
    work follow the rows, the chunk and the hits kept -- no [C, R, T] array is allocated.  Exactly one of pval_max / fdr / bonferroni
    (cut = bonferroni / n_testable of the cohort at that width).  One engine.tile_census and one engine.sparse_window_test (the join,
    the keys and their sort) for every width; per width, in the order given: engine.tile_window_census, zero_tile_floor at
    binsize * width (an empty window's pt is at most min(1, width binsize smax / denom)), then the candidate windows in chunks of at
    most chunk_windows (default engine.SPARSE_WINDOW_CHUNK).  Of a chunk only what can still be a hit is kept -- pval_max: p <= it;
    bonferroni: p <= level / max(the census' testable windows, 1), an upper bound of the final cut, filtered again with the final
    n_testable; fdr: p <= fdr (every Benjamini-Hochberg hit is, and holds its rank among them) -- and, per cohort, the windows with a
    p-value that the census does not count are counted.  With fdr the route keeps every window with p <= fdr (16 bytes each on the
    device beside the host copy): pval_max and bonferroni are the genome-scale cuts.
    Frames as nb_model_window_hits makes them (the nine columns, WIDTH, PEAK, QVAL with fdr per cohort and width; the index is the row
    number in the full frame of that width; attrs n_testable and n_windows, one entry per width), with two more attrs, one entry per
    width each: zero_floor, a lower bound of the p-value of every empty testable window, and complete, zero_floor (1 - 4e-6) > cut --
    no empty window can be a hit.  Where it is false the frame is the dense hits with OBS >= 1.  Pi and EXP agree with the dense window
    route to rounding (one division of the window's sum here, a sum of the tiles' quotients there), not in bits.
    fdr needs every cohort complete at every width, else ValueError (naming cohorts, widths and floors) before any window is tested.
    ValueError before a genome is packed: no cut or more than one, a bonferroni outside (0, 1], what _check_widths refuses, a width above
    engine.TILE_WINDOW_MAX_WIDTH, a negative S_prob entry, n_up != n_down or n_up not 1 or 2.  The sample options are no parameters."""
    _one_cut(pval_max, fdr, bonferroni)
    widths = _check_widths(widths)
    from .. import engine
    if max(widths) > engine.TILE_WINDOW_MAX_WIDTH:
        raise ValueError("widths: at most %d tiles" % engine.TILE_WINDOW_MAX_WIDTH)
    if n_up != n_down or n_up not in (1, 2):
        raise ValueError("the tile kernels take n_up = n_down = 1 or 2")
    if isinstance(binsize, (bool, np.bool_)) or int(binsize) != binsize or binsize < 1:
        raise ValueError("binsize: an integer >= 1")
    binsize = int(binsize)
    import pandas as pd
    import torch
    from ..data_tools import cohort_rows, genome as genome_mod
    C = len(d_prs)
    f_muts = list(f_muts)
    idx = np.asarray(idx)
    R = len(idx)
    mu, sigma = np.asarray(mu, float).reshape(C, R), np.asarray(sigma, float).reshape(C, R)
    if len(f_muts) != C:
        raise ValueError("one mutation file per cohort: %d files for %d cohorts" % (len(f_muts), C))
    s_prob = np.stack([_s_prob_table(d, n_up, collapse) for d in d_prs]) if C else np.zeros((0, 4 ** (2 * n_up + 1)))
    if (s_prob < 0).any():
        raise ValueError("S_prob: a negative entry (cohort %d)" % int(np.argwhere(s_prob < 0)[0][0]))
    starts, ends = (idx[:, 1].astype(np.int64), idx[:, 2].astype(np.int64)) if R else (np.zeros(0, np.int64),) * 2
    engine.check_tile_regions(starts, ends, n_up)
    g = f_fasta if isinstance(f_fasta, genome_mod.PackedGenome) else genome_mod.PackedGenome.from_fasta(f_fasta)
    chroms = [str(c) for c in idx[:, 0]] if R else []
    known = set(n.replace("chr", "") for n in g.names)
    rows = _cohort_rows(f_muts, known, False)
    mc, ms, me = cohort_rows.column(rows, "chrom"), cohort_rows.column(rows, "start", "i64"), cohort_rows.column(rows, "end", "i64")
    co = cohort_rows.cohort_column(rows, "start")
    n_tiles = int(max(1, -(-int((ends - starts).max() if R else 1) // binsize)))
    first_d, nval_d, denom_d, npos_d = engine.tile_census(g, chroms, starts, ends, s_prob, binsize, n_tiles=n_tiles, device=device)
    first, nval = first_d.cpu().numpy(), np.clip(nval_d.cpu().numpy().astype(np.int64), 0, n_tiles)
    smax = s_prob.max(axis=1) if C else np.zeros(0)
    smin = np.where(s_prob > 0, s_prob, np.inf).min(axis=1) if C else np.zeros(0)
    # per width: the windows, the testable ones the census knows, the floor -- and the certificates of fdr before any window is tested
    census = []
    for m in widths:
        nwin_d, npw_d = engine.tile_window_census(g, chroms, starts, ends, s_prob, binsize, m, n_tiles=n_tiles, n_positive=npos_d)
        floor, testable_d = zero_tile_floor(denom_d, smax, smin, mu, sigma, binsize * m, npos_d)
        n_census = (npw_d.long() * testable_d).sum(dim=1).cpu().numpy() if R else np.zeros(C, np.int64)
        census.append((nwin_d.cpu().numpy().astype(np.int64), n_census, floor))
    if fdr is not None:
        bad = [(c, m) for m, (_, _, floor) in zip(widths, census) for c in range(C) if not floor[c] * (1.0 - ZERO_FLOOR_MARGIN) > fdr]
        if bad:
            raise ValueError("fdr = %g: no certificate that an empty window is no hit for cohorts %s at widths %s (zero-window floors %s): "
                             "a smaller fdr, a smaller binsize or width, or nb_model_window_hits"
                             % (fdr, sorted(set(c for c, _ in bad)), sorted(set(m for _, m in bad)),
                                ["%.3g" % census[widths.index(m)][2][c] for c, m in bad]))
    scan = engine.sparse_window_test(g, chroms, starts, ends, s_prob, binsize, n_tiles, first_d, nval_d, denom_d, mu, sigma, mc, ms, me, co,
                                     chunk_windows=chunk_windows)
    dev = denom_d.device
    n_pos = _region_positions(g, chroms, ends, first, n_up) if R else np.zeros(0, np.int64)
    last = first + n_pos                                       # one past a region's last position
    per_width = []                     # (m, the kept windows as host arrays, their cohort_ptr, cuts [C], n_testable [C], n_windows [R], floor, level)
    for m, (nwin, n_census, floor) in zip(widths, census):
        if pval_max is not None:
            bound = np.full(C, float(pval_max))
        elif fdr is not None:
            bound = np.full(C, float(fdr))
        else:
            bound = float(bonferroni) / np.maximum(n_census, 1)
        bound_d = torch.as_tensor(bound, device=dev)
        extra = torch.zeros(C, dtype=torch.int64, device=dev)
        kept, kept_p = [], []
        for ch in scan.chunks(m):
            c, p = ch["cohort"].long(), ch["pval"]
            counted = testable_d[c, ch["region"].long()] & (ch["pt"] > 0)        # (the window census has these windows already)
            extra += torch.bincount(c[~torch.isnan(p) & ~counted], minlength=C)[:C]
            keep = p <= bound_d[c]                                             # (a NaN never passes)
            kept.append({name: v[keep].cpu().numpy() for name, v in ch.items()})
            if fdr is not None:
                kept_p.append(p[keep])
        win = {name: np.concatenate([k[name] for k in kept]) if kept else np.zeros(0, np.int32 if i < 4 else np.float64)
               for i, name in enumerate(engine.SparseWindows.NAMES)}
        n_test = n_census + extra.cpu().numpy()
        wc = win["cohort"].astype(np.int64)
        ptr = np.searchsorted(wc, np.arange(C + 1))                            # (the windows lie cohort-major)
        if fdr is not None:
            cuts = np.full(C, -1.0)
            if len(wc):
                # the mutated windows with p <= fdr, ranked in a list of n_testable: every rank up to the pivot is theirs
                lists = torch.cat(kept_p).contiguous()
                q, _ = bh_ragged(lists, ptr.astype(np.int64), n_global=np.maximum(n_test, 1).astype(np.float64))
                for c in range(C):
                    cuts[c] = bh_cut(lists[ptr[c]:ptr[c + 1]], q[ptr[c]:ptr[c + 1]], fdr)
            level = np.full(C, float(fdr))
        elif bonferroni is not None:
            cuts = level = float(bonferroni) / np.maximum(n_test, 1)
        else:
            cuts = level = np.full(C, float(pval_max))
        per_width.append((m, win, ptr, cuts, n_test, nwin, floor, level))
    frames = []
    for c in range(C):
        cols = {name: [] for name in ("reg", "t", "k", "exp", "pval", "pt", "lo", "hi", "peak", "q", "row")}
        for m, win, ptr, cuts, n_test, nwin, _, _ in per_width:
            sel = np.arange(ptr[c], ptr[c + 1])
            sel = sel[win["pval"][sel] <= cuts[c]]
            reg, t, score = win["region"][sel].astype(np.int64), win["window"][sel].astype(np.int64), win["pval"][sel]
            lo = first[reg] + t * binsize
            hi = np.minimum(lo + np.minimum(m, nval[reg] - t) * binsize, last[reg]) - 1
            cols["reg"].append(reg), cols["t"].append(t), cols["lo"].append(lo), cols["hi"].append(hi)
            cols["k"].append(win["k"][sel]), cols["exp"].append(win["exp"][sel]), cols["pt"].append(win["pt"][sel]), cols["pval"].append(score)
            cols["peak"].append(window_peaks(reg, t, score, m))
            cols["q"].append(hits_q_values(score, int(n_test[c])) if fdr is not None else score)
            cols["row"].append((np.cumsum(nwin) - nwin)[reg] + t)
        cat = {name: np.concatenate(v) for name, v in cols.items()}
        df = _tile_frame(idx, mu[c], sigma[c], first, n_pos, binsize, cat["reg"], cat["t"], cat["k"], cat["exp"], cat["pval"], cat["pt"])
        df["POS"] = (cat["lo"] + cat["hi"]) / 2.0
        df["WIDTH"], df["PEAK"] = (cat["hi"] - cat["lo"] + 1).astype(float), cat["peak"].astype(bool)
        if fdr is not None:
            df["QVAL"] = cat["q"]
        df.index = pd.Index(cat["row"], dtype=np.int64)
        df.attrs.update(n_testable=[int(w[4][c]) for w in per_width], n_windows=[int(w[5].sum()) for w in per_width],
                        zero_floor=[float(w[6][c]) for w in per_width],
                        complete=[bool(w[6][c] * (1.0 - ZERO_FLOOR_MARGIN) > w[7][c]) for w in per_width])
        frames.append(df)
    return frames


def bh_ragged(p, row_ptr, n_global=None, rank0=None, carry=None, want_q=True, want_row_min=False, sorted_out=False):
    """dig_bh_qvalues_ragged (csrc/dig_sort.hip): Benjamini-Hochberg q-values of ragged rows of one float64 device tensor -- the
    library's own batched radix sort (63-bit keys, 32-bit payload, one kernel per pass), the Benjamini-Hochberg pass and the
    way back to every p-value's place in one launch sequence.  row_ptr: host offsets (rows + 1).  n_global / rank0 / carry (host
    arrays or None): the rows are ranges of longer lists (parallel.ShardedTiles' sample sort).  Returns (q or None, row_min or None)."""
    import torch
    from .. import _lib
    p = p.contiguous()
    assert p.dtype == torch.float64 and p.is_cuda
    rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
    rows = rp.size - 1
    h = lambda a, dt: None if a is None else np.ascontiguousarray(a, dtype=dt)
    ng, r0, ca = h(n_global, np.float64), h(rank0, np.int64), h(carry, np.float64)
    q = torch.empty_like(p) if want_q else None
    rmin = torch.empty(max(rows, 1), dtype=torch.float64, device=p.device) if want_row_min else None
    wsb = int(_lib.load().dig_bh_ragged_workspace(_lib.host_ptr(rp), rows))
    ws = torch.empty(wsb, dtype=torch.uint8, device=p.device)
    with torch.cuda.device(p.device):
        _lib.call("dig_bh_qvalues_ragged", _lib.dev_ptr(p), _lib.host_ptr(rp), rows, _lib.host_ptr(ng), _lib.host_ptr(r0), _lib.host_ptr(ca),
                  _lib.dev_ptr(q) if q is not None else None, _lib.dev_ptr(rmin) if rmin is not None else None, 1 if sorted_out else 0,
                  _lib.dev_ptr(ws), wsb, _lib.stream_ptr())
    return q, (rmin[:rows] if rmin is not None else None)


def get_q_vals_rows(p_rows):
    """get_q_vals for every row of a [rows, n] device tensor at once (the cohorts of the per-base route): one call of
    dig_bh_qvalues_ragged -- the library's radix sort of all rows, the Benjamini-Hochberg pass and the scatter behind it."""
    import torch
    p = p_rows.to(torch.float64).contiguous()
    rows, n = p.shape
    if n == 0 or rows == 0:
        return p.clone()
    q, _ = bh_ragged(p.reshape(-1), np.arange(rows + 1, dtype=np.int64) * n)
    return q.reshape(rows, n)


def get_q_vals(pvals_lst):
    """nb_model.py:340-342: Benjamini-Hochberg q-values, statsmodels.stats.multitest.fdrcorrection(pvals)[1] (method
    'indep'): q_(i) = min_{j >= i} p_(j) n / j in ascending order of p, capped at 1.  NaNs propagate the way the sort
    places them (last)."""
    if type(pvals_lst).__module__.startswith("torch") and pvals_lst.is_cuda:
        # device form for whole-genome tile sets (57.6 M p-values per cohort): the same IEEE operations in the same order
        # (p / (rank / n), reverse running minimum, cap), so the same bits as the host form and as statsmodels
        return get_q_vals_rows(pvals_lst.reshape(1, -1)).reshape(pvals_lst.shape)
    p = np.asarray(pvals_lst, dtype=np.float64)
    n = p.size
    if n == 0:
        return p.copy()
    order = np.argsort(p, kind="stable")
    ps = p[order]
    q = ps / (np.arange(1, n + 1) / float(n))          # statsmodels' own operation order (p / ecdf): bit-identical
    q = np.minimum.accumulate(q[::-1])[::-1]
    q = np.minimum(q, 1.0)
    out = np.empty_like(q)
    out[order] = q
    return out
