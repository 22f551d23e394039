"""Batched, device-resident burden-test engine: all elements x all cohorts per launch.

This is the MI355X-first form of the path the reference walks one cohort and one
element at a time:

    accumulate_elements  <- genic_driver_tools.nonc_model / genic_model / tiled_nonc_model
                            (genic_driver_tools.py:300-431, 31-203, 599-690)
    element_stats        <- transfer_tools.transfer_element_model_with_indels, element_expected_muts_nb,
                            element_pvalue_burden_nb(_by_sample), element_pvalue_indel, Fisher
                            (transfer_tools.py:272-302,343-344,473-482,594-615,731-747,1086-1087)
    gather_bins          <- LazyLoadDatasetFromH5.__getitem__ (mut_dataset.py:76-81)
    tiled_nb_test        <- nb_model.apply_nb_to_region arithmetic (nb_model.py:141-178)

Every function takes either torch CUDA tensors (device entry points, enqueued on
torch's current stream, zero copies) or numpy arrays (``*_host`` twins); each is written
once on the backend pair of _marshal.py (the plans keep their cached-argument run() paths).  The two-call entry points
(counts, fill) share `_scan`, the routes that turn a refused requirement into ValueError share `_requirements_as_value_errors`, and
the callers stack their cohorts with data_tools/cohort_rows.py; nothing here imports data_tools.  PyTorch is used only for device
memory and streams.
"""
import contextlib

import numpy as np

from . import _lib
from ._marshal import backend_of, backend_on, device_backend, is_cuda

ES_PLANES = _lib.ES_PLANES
GS_PLANES = _lib.GS_PLANES
SEL_PLANES = _lib.SEL_PLANES


def _t(x, dtype, device):
    return device_backend(device).arr(x, dtype)


_WS_CACHE = {}


def _workspace(kind, E, C, dev, private=False):
    """Device scratch for one launch sequence (a torch uint8 tensor, 256-byte aligned by the caching allocator).

    The one-shot entry points share a cached buffer per (kind, device, STREAM): launches on one stream are ordered, so they
    may reuse it; two callers overlapping the same operation on two streams get two buffers.  Plan objects
    (`private=True`) own theirs for their lifetime -- their launches may be enqueued on any stream, any number of steps
    ahead."""
    import torch
    need = _lib.workspace_bytes(kind, E, C)
    if need <= 0:
        return None, 0
    if private:
        return torch.empty(need, dtype=torch.uint8, device=dev), need
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (kind, idx, torch.cuda.current_stream(idx).cuda_stream)
    ws = _WS_CACHE.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _WS_CACHE[key] = ws
    return ws, need


def _shared_workspace(be, kind, E, C, use=True):
    """The `workspace=` of be.call for a one-shot launch: the cached buffer on the device (NULL with use=False), nothing on the host."""
    return _workspace(kind, E, C, be.dev) if be.is_device and use else (None, 0)


def _scan(be, counts, groups=None):
    """The i32 counts of a two-call entry point -> (their exclusive prefix sum, i64 on the backend; the total as a host int).
    groups: the counts are that many runs of one length (tile_select's cohorts); then also, from the same transfer as the total,
    where every run starts and the last one ends: host int64 [groups + 1]."""
    n, g = counts.shape[0], 1 if groups is None else groups
    offsets, ends = be.empty(0, "i64"), np.zeros(g, np.int64)
    if n:
        incl = be.torch.cumsum(counts, 0, dtype=be.torch.int64) if be.is_device else np.cumsum(counts, dtype=np.int64)
        ends = incl[n // g - 1::n // g]                                   # the running total behind every run; the last is the total
        offsets, ends = incl - counts, ends.cpu().numpy() if be.is_device else ends
    ptr = np.concatenate([[0], ends]).astype(np.int64)
    return (offsets, int(ptr[-1])) if groups is None else (offsets, int(ptr[-1]), ptr)


@contextlib.contextmanager
def _requirements_as_value_errors():
    """A requirement the library refuses ("requirement failed" in the DigHipError) leaves as ValueError with the same text."""
    try:
        yield
    except _lib.DigHipError as exc:
        if "requirement failed" in str(exc):
            raise ValueError(str(exc)) from exc
        raise


def _cols(a):
    """A table for one cohort given as a vector -> [n, 1]."""
    return a[:, None] if a.ndim == 1 else a


def _per_cohort(be, x, C):
    """f64 [C] (None stays None); a single value stands for every cohort."""
    x = be.arr(x, "f64", (-1,))
    if x is not None and x.shape[0] == 1 and C != 1:
        x = x.repeat(C)
    assert x is None or x.shape[0] == C
    return x


def _rates(be, mu, sigma, mu_indel, sigma_indel):
    """mu, sigma (and the optional indel pair) as f64 [n, C]; returns them and (n, C)."""
    mu = _cols(be.arr(mu, "f64"))
    n, C = mu.shape
    return mu, be.arr(sigma, "f64", (n, C)), be.arr(mu_indel, "f64", (n, C)), be.arr(sigma_indel, "f64", (n, C)), n, C


# ---------------------------------------------------------------------------
def element_stats(mu, sigma, pi_sum, pi_indel, obs_snv, obs_samples, obs_indel, cj, cj_indel,
                  mu_indel=None, sigma_indel=None, device=0, out=None, use_workspace=True):
    """Seven result planes for a dense [E, C] problem.

    mu, sigma, pi_sum : f64 [E, C];  pi_indel : f64 [E] or [E, C];  obs_* : i32 [E, C];
    cj, cj_indel : f64 [C].  Returns a dict plane-name -> [E, C] array/tensor (views of one
    [7, E, C] buffer).  CUDA tensors in -> CUDA tensors out.
    """
    be = backend_of(mu, device=device)
    mu, sigma, mu_indel, sigma_indel, E, C = _rates(be, mu, sigma, mu_indel, sigma_indel)
    pi_sum = be.arr(pi_sum, "f64", (E, C))
    pi_indel = be.arr(pi_indel, "f64")
    per_cohort = int(pi_indel.ndim == 2)
    assert pi_indel.shape == ((E, C) if per_cohort else (E,))
    obs = [be.arr(v, "i32", (E, C)) for v in (obs_snv, obs_samples, obs_indel)]
    cj, cj_indel = _per_cohort(be, cj, C), _per_cohort(be, cj_indel, C)
    if out is None:
        out = be.empty((len(ES_PLANES), E, C), "f64")
    p = be.ptr
    be.call("dig_element_stats", p(mu), p(sigma), p(mu_indel), p(sigma_indel), p(pi_sum), p(pi_indel), per_cohort, p(obs[0]),
            p(obs[1]), p(obs[2]), p(cj), p(cj_indel), p(out), E, C,
            workspace=_shared_workspace(be, "element_stats", E, C, use_workspace))
    return {name: out[i] for i, name in enumerate(ES_PLANES)}


# ---------------------------------------------------------------------------
def _gene_observations(be, obs, n_samp, cj, t_indel, G, C):
    """obs i32 [G, 5, C], n_samp i32 [G, 6, C], cj and t_indel (or None) f64 [C]."""
    return be.arr(obs, "i32", (G, 5, C)), be.arr(n_samp, "i32", (G, 6, C)), _per_cohort(be, cj, C), _per_cohort(be, t_indel, C)


def gene_stats(mu, sigma, pi, pi_indel, obs, n_samp, cj, t_indel=None, mu_indel=None, sigma_indel=None, device=0, out=None):
    """The gene route's statistics block (transfer_tools.py:331-340,394-456,554-583,709-729,860-861) for G genes x C cohorts
    in ONE launch (dig_gene_stats).  mu, sigma f64 [G, C]; pi f64 [G, 6 or 4, C]; pi_indel [G] or [G, C]; obs i32 [G, 5, C]
    (SYN, MIS, NONS, SPL, INDEL); n_samp i32 [G, 6, C]; cj [C]; t_indel [C] or None (no indel block: those planes are NaN).
    Returns dict plane name -> [G, C] (views of one [22, G, C] buffer); CUDA tensors in -> CUDA tensors out."""
    be = backend_of(mu, device=device)
    mu, sigma, mu_indel, sigma_indel, G, C = _rates(be, mu, sigma, mu_indel, sigma_indel)
    pi = be.arr(pi, "f64")
    if pi.ndim == 2:
        pi = pi[:, :, None]
    n_pi = pi.shape[1]
    assert pi.shape == (G, n_pi, C) and n_pi in (4, 6)
    pi_indel = be.arr(pi_indel, "f64")
    per_cohort = int(pi_indel is not None and pi_indel.ndim == 2)
    obs, n_samp, cj, ti = _gene_observations(be, obs, n_samp, cj, t_indel, G, C)
    if out is None:
        out = be.empty((len(GS_PLANES), G, C), "f64")
    p = be.ptr
    be.call("dig_gene_stats", p(mu), p(sigma), p(mu_indel), p(sigma_indel), p(pi), n_pi, p(pi_indel), per_cohort, p(obs), p(n_samp),
            p(cj), p(ti), int(ti is not None), p(out), G, C)
    return {name: out[i] for i, name in enumerate(GS_PLANES)}


def gene_selection(alpha, theta, pi, obs, device=0, out=None):
    """The gene route's dN/dS correction and selection tests (transfer_tools.py:363-392,617-676,749-765,1172-1292) for G genes x
    C cohorts in ONE launch (dig_gene_selection).  alpha, theta f64 [G, C] (the frame's ALPHA and THETA: THETA already scaled);
    pi f64 [G, 6 or 4, C] ([G, n_pi] for one cohort); obs i32 [G, 5, C] (SYN, MIS, NONS, SPL, INDEL; INDEL unused).
    Returns dict plane name -> [G, C] (views of one [34, G, C] buffer, SEL_PLANES); CUDA tensors in -> CUDA tensors out."""
    be = backend_of(alpha, device=device)
    alpha = _cols(be.arr(alpha, "f64"))
    G, C = alpha.shape
    theta = be.arr(theta, "f64", (G, C))
    pi = be.arr(pi, "f64")
    if pi.ndim == 2:
        pi = pi[:, :, None]
    n_pi = pi.shape[1]
    assert pi.shape == (G, n_pi, C) and n_pi in (4, 6)
    obs = be.arr(obs, "i32", (G, 5, C))
    if out is None:
        out = be.empty((len(SEL_PLANES), G, C), "f64")
    p = be.ptr
    be.call("dig_gene_selection", p(alpha), p(theta), p(pi), n_pi, p(obs), p(out), G, C)
    return {name: out[i] for i, name in enumerate(SEL_PLANES)}


def join_blocks(chrom, start, end):
    """The block table of the interval join (dig_overlap_join_*) from host arrays, in any order: chromosome id, START, END.
    Returns (order, start_key, runmax_key, end_eff), host int64: `order` sorts the blocks by (chrom, start) (stably: blocks sorted
    already keep their rows), and in that order end_eff is the block's end, a zero-length block (end == start) lifted to
    start + 1, start_key = (chrom << 40) | start and runmax_key = (chrom << 40) | the largest end_eff so far on the chromosome."""
    chrom, start, end = (np.asarray(x, np.int64).ravel() for x in (chrom, start, end))
    order = np.lexsort((start, chrom))
    chrom, start, end_eff = chrom[order], start[order], np.where(end == start, start + 1, end)[order]
    runmax = np.empty_like(end_eff)
    for c in np.unique(chrom):
        sel = chrom == c
        runmax[sel] = np.maximum.accumulate(end_eff[sel])
    return order, (chrom << 40) | start, (chrom << 40) | runmax, end_eff


def _window_blocks(win_chrom, win_start, win_end):
    """Windows (chromosome id, START, END: host arrays in any order) as the one-block elements of join_blocks."""
    wc, ws, we = (np.asarray(x, np.int64).ravel() for x in (win_chrom, win_start, win_end))
    if len(wc) and (wc.min() < 0 or wc.max() >= (1 << 22) or ws.min() < 0 or max(ws.max(), we.max()) >= (1 << 40)):
        raise ValueError("windows: chromosome ids within [0, 2^22), coordinates within [0, 2^40)")
    return join_blocks(wc, ws, we)


def overlap_join(be, start_key, runmax_key, blk_end, m_chrom, m_start, m_end, max_pairs=None,
                 too_many="%d (row, block) pairs: more than max_pairs"):
    """The interval join of mutation rows (chromosome id, start, end: half-open, int64) with a block table of join_blocks:
    dig_overlap_join_count, a cumulative sum, dig_overlap_join_fill.  Returns (pair_row, pair_blk): int32, one entry per
    overlapping (row, block of the sorted table), mutation-major with the blocks ascending; ValueError, before the fill, for
    more than max_pairs of them, with the caller's text `too_many` (%d: the pair count).  CUDA tensors on the device backend,
    arrays on the host one."""
    tabs = [be.arr(x, "i64", (-1,)) for x in (start_key, runmax_key, blk_end, m_chrom, m_start, m_end)]
    n_blk, n = tabs[0].shape[0], tabs[3].shape[0]
    assert tabs[1].shape[0] == tabs[2].shape[0] == n_blk and tabs[4].shape[0] == tabs[5].shape[0] == n
    if n == 0 or n_blk == 0:
        return be.empty(0, "i32"), be.empty(0, "i32")
    p = be.ptr
    join = [p(x) for x in tabs[:3]] + [n_blk] + [p(x) for x in tabs[3:]] + [n]
    counts = be.empty(n, "i32")
    be.call("dig_overlap_join_count", *join, p(counts))
    offsets, total = _scan(be, counts)
    if max_pairs is not None and total > max_pairs:
        raise ValueError(too_many % total)
    pair_row, pair_blk = be.empty(total, "i32"), be.empty(total, "i32")
    if total:
        be.call("dig_overlap_join_fill", *join, p(offsets), *([] if be.is_device else [total]), p(pair_row), p(pair_blk))
    return pair_row, pair_blk


def _sample_offsets(x, C=None):
    """sample_offsets (a host array or a CUDA tensor) -> (host int64 [C + 1], C, the sample count S).  C: the cohort count of a
    caller that was given one (the library refuses C < 1 for it); without it C comes from the length, at least 1."""
    off = np.ascontiguousarray(np.asarray(x.cpu() if is_cuda(x) else x), dtype=np.int64).ravel()
    if (len(off) < 2 if C is None else len(off) != C + 1) or off[0] != 0 or (np.diff(off) < 0).any():
        raise ValueError("sample_offsets: C + 1 non-decreasing entries, 0 first")
    return off, len(off) - 1, int(off[-1])


def _sorted(be, keys):
    """The keys ascending: the caller of a sorted-key entry point sorts (plumbing, as for dig_bh_qvalues_sorted)."""
    return keys.sort()[0] if be.is_device else np.sort(keys)


def gene_counts(gene, sample, annot, cohort, sample_offsets, G, C, tp53, max_muts_per_sample=3e9, max_muts_per_gene_per_sample=3e9,
                device=0):
    """The gene route's integer bookkeeping for the coding rows of C cohorts against one gene index of G rows
    (filter_hypermut_samples, mutations_per_gene, the N_SAMP_* columns of transfer_gene_model and the synonymous row count of the
    scale factor; mutation_tools.py:293-304,329-361, transfer_tools.py:196-270,809-823): dig_gene_row_keys, a key sort,
    dig_gene_counts.  Rows as tabulate_gpu.encode_gene_rows gives them: gene i32 (0 .. G - 1, G = outside the model, G + 1 = TP53
    when the model has none), sample i32 (dense per cohort), annot u8 (0 SYN, 1 MIS, 2 NONS, 3 SPL, 4 INDEL, 5 other), cohort i32;
    sample_offsets [C + 1] = a cohort's first global sample; tp53: TP53's gene id.
    Returns dict(obs i32 [G, 5, C] (SYN, MIS, NONS, SPL, INDEL) and n_samp i32 [G, 6, C] as gene_stats takes them, n_syn i64 [C],
    blacklisted u8 per global sample, n_samp_indel i32 [G, C], n_pairs i32 [G, C]: (gene, sample) pairs with a row of any class).
    CUDA tensors in -> CUDA tensors out."""
    be = backend_of(gene, sample, annot, cohort, device=device)
    gene, sample, cohort = (be.arr(x, "i32", (-1,)) for x in (gene, sample, cohort))
    annot = be.arr(annot, "u8", (-1,))
    n = gene.shape[0]
    assert sample.shape[0] == annot.shape[0] == cohort.shape[0] == n
    G = int(G)
    off_host, C, S = _sample_offsets(sample_offsets, int(C))
    off = be.arr(off_host, "i64")
    if be.is_device and n:
        # (device tensors are checked here; the host twin checks its own arrays inside the library)
        per_row = (off[1:] - off[:-1])[cohort.clamp(0, C - 1).long()]
        bad = (cohort < 0) | (cohort >= C) | (gene < 0) | (gene > G + 1) | (annot > 5) | (sample < 0) | (sample >= per_row)
        if bool(bad.any()):
            raise ValueError("a row outside the tables: cohort within [0, C), gene within [0, G + 1], annot within [0, 5], sample "
                             "within its cohort")
    p = be.ptr
    keys, total = be.empty(n, "i64"), be.empty(S, "i32")
    be.call("dig_gene_row_keys", p(gene), p(sample), p(annot), p(cohort), p(off), n, G, C, S, p(keys), p(total))
    keys = _sorted(be, keys)
    obs, n_samp, extra = be.empty((G, 5, C), "i32"), be.empty((G, 6, C), "i32"), be.empty((G, 2, C), "i32")
    n_syn, black = be.empty(C, "i64"), be.empty(S, "u8")
    scratch = [p(be.empty((G, 5, C), "i32"))] if be.is_device else []      # (the host twin stages its own)
    be.call("dig_gene_counts", p(keys), n, p(total), S, float(max_muts_per_sample), float(max_muts_per_gene_per_sample), int(tp53),
            G, C, p(obs), p(n_samp), p(extra), p(n_syn), p(black), *scratch)
    return dict(obs=obs, n_samp=n_samp, n_syn=n_syn, blacklisted=black, n_samp_indel=extra[:, 0], n_pairs=extra[:, 1])


def panel_counts(label, sample, annot, cohort, sample_offsets, label_mask, P, skip=None, device=0):
    """The target route's panel bookkeeping for the rows of C cohorts and P <= 32 panels (CohortRun.panel_scale,
    transfer_tools.py:905-935; DigPretrain.py countMutations, :103-177): dig_panel_row_keys, a key sort, dig_panel_counts.  Rows as
    tabulate_gpu.encode_panel_rows gives them: label i32 (0 .. L - 1 = the place in the label table, L = in no panel), sample i32
    (dense per cohort), annot u8 (0 SYN, 1 MIS, 2 NONS, 3 SPL, 4 INDEL, 5 other, 6 Noncoding), cohort i32; sample_offsets [C + 1];
    label_mask u32 [L] (a host array): bit p set when the label is in panel p; skip u8 per global sample or None: the blacklist.
    Returns dict(n_mut, n_pairs, n_sample i64 [C, P]: counted rows, distinct (label, sample) pairs and distinct samples per cohort
    and panel; n_cds i64 [C]: rows that are not Noncoding).  CUDA tensors in -> CUDA tensors out."""
    be = backend_of(label, sample, annot, cohort, device=device)
    label, sample, cohort = (be.arr(x, "i32", (-1,)) for x in (label, sample, cohort))
    annot = be.arr(annot, "u8", (-1,))
    n = label.shape[0]
    assert sample.shape[0] == annot.shape[0] == cohort.shape[0] == n
    P = int(P)
    off_host, C, S = _sample_offsets(sample_offsets)
    mask_host = np.ascontiguousarray(np.asarray(label_mask.cpu() if is_cuda(label_mask) else label_mask)).ravel()
    if mask_host.dtype != np.uint32:
        if len(mask_host) and (mask_host.min() < 0 or mask_host.max() >= 2 ** 32):
            raise ValueError("label_mask: 32-bit masks")
        mask_host = mask_host.astype(np.uint32)
    L = len(mask_host)
    mask = be.arr(mask_host.view(np.int32), "i32")          # (the bits; the library reads them as u32)
    off = be.arr(off_host, "i64")
    skip = be.arr(skip, "u8", (-1,))
    if skip is not None and skip.shape[0] != S:
        raise ValueError("skip: one byte per global sample ({})".format(S))
    if be.is_device and n:
        # (device tensors are checked here; the host twin checks its own arrays inside the library)
        per_row = (off[1:] - off[:-1])[cohort.clamp(0, C - 1).long()]
        bad = (cohort < 0) | (cohort >= C) | (label < 0) | (label > L) | (annot > 6) | (sample < 0) | (sample >= per_row)
        if bool(bad.any()):
            raise ValueError("a row outside the tables: cohort within [0, C), label within [0, L], annot within [0, 6], sample "
                             "within its cohort")
    p = be.ptr
    keys, n_cds = be.empty(n, "i64"), be.empty(C, "i64")
    with _requirements_as_value_errors():
        be.call("dig_panel_row_keys", p(label), p(sample), p(annot), p(cohort), p(off), p(skip), p(mask), n, L, P, C, S, p(keys), p(n_cds))
        keys = _sorted(be, keys)
        n_mut, n_pairs, n_sample = (be.empty((C, P), "i64") for _ in range(3))
        be.call("dig_panel_counts", p(keys), n, p(mask), p(off), L, P, C, S, p(n_mut), p(n_pairs), p(n_sample))
    return dict(n_mut=n_mut, n_pairs=n_pairs, n_sample=n_sample, n_cds=n_cds)


def window_objectives(win_chrom, win_start, win_end, row_chrom, row_start, row_end, row_sample, row_uid, row_indel, sample_offsets,
                      n_uid, keep_from_hits=None, device=0):
    """The region model's training labels for C cohorts at once (scripts/DataExtractor.py:525-572 add_objectives without --cnv):
    dig_overlap_join_count/fill of all cohorts' rows with the N windows as one-block elements, dig_window_pair_keys, a key sort,
    dig_window_sample_hits, `keep_from_hits` on the host, dig_window_objectives.
    Windows: chromosome id i64, START, END (host arrays, any order; the rows' chromosome ids name the same chromosomes).  Rows: chrom,
    start, end i64; sample i32 = the GLOBAL sample (sample_offsets [C + 1]: a cohort's first); uid i32 = dense ids, below n_uid, of the
    cohort's distinct (CHROM, START, END, REF, ALT); indel u8.
    keep_from_hits(hits): host int32 [S], the distinct windows each sample hits -> the samples that stay, bool / u8 [S] (None: all).
    Returns dict(labels f64 [N, C]: distinct non-indel mutations of the kept samples per window and cohort; hits, keep: host arrays).
    CUDA tensors in (the row arrays) -> labels as a CUDA tensor."""
    be = backend_of(row_chrom, row_start, row_end, row_sample, row_uid, row_indel, device=device)
    off_host, C, S = _sample_offsets(sample_offsets)
    n_uid = int(n_uid)
    order, start_key, runmax_key, blk_end = _window_blocks(win_chrom, win_start, win_end)
    N = len(order)
    blk_window = be.arr(order, "i32")
    row_chrom, row_start, row_end = (be.arr(x, "i64", (-1,)) for x in (row_chrom, row_start, row_end))
    row_sample, row_uid = be.arr(row_sample, "i32", (-1,)), be.arr(row_uid, "i32", (-1,))
    row_indel = be.arr(row_indel, "u8", (-1,))
    n = row_chrom.shape[0]
    assert row_start.shape[0] == row_end.shape[0] == row_sample.shape[0] == row_uid.shape[0] == row_indel.shape[0] == n
    if be.is_device and n:
        # (device tensors are checked here; the host twin checks its own arrays inside the library)
        bad = (row_sample < 0) | (row_sample >= S) | (row_uid < 0) | (row_uid >= n_uid)
        if bool(bad.any()):
            raise ValueError("a row outside the tables: global sample within [0, S), mutation id within [0, n_uid)")
    pair_row, pair_blk = overlap_join(be, start_key, runmax_key, blk_end, row_chrom, row_start, row_end, max_pairs=2 ** 31 - 1,
                                      too_many="%d (mutation, window) pairs: the join's pair indices are 32-bit; fewer cohorts per call")
    total = pair_row.shape[0]
    p = be.ptr
    keys = be.empty(total, "i64")
    be.call("dig_window_pair_keys", p(pair_row), p(pair_blk), total, p(blk_window), N, p(row_sample), p(row_uid), p(row_indel), n,
            S, N, n_uid, p(keys))
    keys = _sorted(be, keys)
    hits = be.empty(S, "i32")
    be.call("dig_window_sample_hits", p(keys), total, S, N, n_uid, p(hits))
    hits_host = hits.cpu().numpy() if be.is_device else hits
    keep_host = np.ones(S, np.uint8) if keep_from_hits is None else np.ascontiguousarray(keep_from_hits(hits_host), dtype=np.uint8)
    if keep_host.shape != (S,):
        raise ValueError("keep_from_hits: one entry per global sample")
    labels = be.empty((N, C), "f64")
    # (named, so that every buffer of the call is alive at once: a tensor dropped here goes back to the allocator and the next one
    #  may be given its memory)
    keep, off = be.arr(keep_host, "u8"), be.arr(off_host, "i64")
    scratch = [be.empty((N, C), "i32")] if be.is_device else []            # (the host twin stages its own)
    be.call("dig_window_objectives", p(keys), total, p(keep), p(off), S, N, C, n_uid, p(labels), *[p(s) for s in scratch])
    return dict(labels=labels, hits=hits_host, keep=keep_host)


def window_cnv_means(win_chrom, win_start, W, seg_chrom, seg_start, seg_end, seg_class, seg_weight, seg_cohort, C, device=0):
    """The region model's copy-number training labels for C cohorts at once (scripts/DataExtractor.py:100-154,535-539 add_objectives
    --cnv): per window [START, START + W) the mean over its W positions of the duplication, copy-neutral / LOH and deletion tracks of
    a cohort's segments -- dig_cnv_segment_deltas (one thread per segment into a difference array), dig_cnv_window_means (its prefix
    sums / W).  No (segment, window) pair is formed.
    Windows: chromosome id, START (host arrays, any order, repeated or overlapping each other); the distinct (chrom, START) are
    sorted here and the result scattered back.  Segments: chrom (the windows' chromosome ids; another one adds nothing), start, end
    i64, half-open; class u8 (0 duplication, 1 LOH, 2 deletion); weight i32 >= 1; cohort i32 within [0, C).
    Returns labels f64 [N, 3, C], N = the windows as given; CUDA tensors in (the segment arrays) -> a CUDA tensor."""
    be = backend_of(seg_chrom, seg_start, seg_end, seg_class, seg_weight, seg_cohort, device=device)
    C, W = int(C), int(W)
    wc, ws = (np.asarray(x, np.int64).ravel() for x in (win_chrom, win_start))
    if wc.shape != ws.shape:
        raise ValueError("windows: one START per chromosome id")
    if len(wc) and (wc.min() < 0 or wc.max() >= (1 << 22) or ws.min() < 0 or ws.max() >= (1 << 40)):
        raise ValueError("windows: chromosome ids within [0, 2^22), starts within [0, 2^40)")
    key, inverse = np.unique((wc << 40) | ws, return_inverse=True)                           # the distinct windows by (chrom, START)
    inverse = np.asarray(inverse).reshape(-1)
    N = len(key)
    uniq_start = key & ((1 << 40) - 1)
    chrom_id, first = np.unique(key >> 40, return_index=True)
    chrom_off = np.concatenate([first, [N]]).astype(np.int64)
    seg_chrom, seg_start, seg_end = (be.arr(x, "i64", (-1,)) for x in (seg_chrom, seg_start, seg_end))
    seg_class, seg_weight, seg_cohort = be.arr(seg_class, "u8", (-1,)), be.arr(seg_weight, "i32", (-1,)), be.arr(seg_cohort, "i32", (-1,))
    n = seg_chrom.shape[0]
    assert seg_start.shape[0] == seg_end.shape[0] == seg_class.shape[0] == seg_weight.shape[0] == seg_cohort.shape[0] == n
    if be.is_device and n:
        # (device tensors are checked here; the host twin checks its own arrays inside the library)
        bad = (seg_start < 0) | (seg_end <= seg_start) | (seg_end > (1 << 40)) | (seg_class > 2) | (seg_weight < 1) | (seg_cohort < 0) | \
            (seg_cohort >= C)
        if bool(bad.any()):
            raise ValueError("a segment outside the tables: 0 <= start < end <= 2^40, class within [0, 2], weight >= 1, cohort within [0, C)")
    p = be.ptr
    with _requirements_as_value_errors():
        lib = _lib.load()
        delta_bytes, carry_bytes = int(lib.dig_cnv_segment_deltas_size(C, N)), int(lib.dig_cnv_window_means_size(C, N))
        if delta_bytes < 0 or carry_bytes < 0:
            raise ValueError(_lib.last_error())
        # (named, so that every buffer of the two calls is alive at once)
        starts, ids, off = be.arr(uniq_start, "i64"), be.arr(chrom_id, "i64"), be.arr(chrom_off, "i64")
        deltas, labels = be.empty(delta_bytes // 8, "i64"), be.empty((C, N, 3), "f64")
        be.call("dig_cnv_segment_deltas", p(starts), p(ids), p(off), len(chrom_id), N, W, p(seg_chrom), p(seg_start), p(seg_end), p(seg_class),
                p(seg_weight), p(seg_cohort), n, C, p(deltas))
        scratch = [be.empty(carry_bytes // 8, "i64")] if be.is_device else []              # (the host twin stages its own)
        be.call("dig_cnv_window_means", p(deltas), N, C, W, p(labels), *[p(s) for s in scratch])
    if be.is_device:
        return labels.permute(1, 2, 0)[be.arr(inverse, "i64")].contiguous()
    return np.ascontiguousarray(labels.transpose(1, 2, 0)[inverse])


def sequence_counts(win_chrom, win_start, win_end, row_chrom, row_start, row_end, row_type, row_cohort, K, C, device=0):
    """The sequence model's sufficient statistic for C cohorts at once (scripts/DigPretrain.py:179-208 sequenceModel): per cohort the
    K counts of (MUT_TYPE, CONTEXT) over the rows that lie in at least one window -- dig_overlap_join_count/fill of all cohorts' rows
    with the windows as one-block elements, then dig_sequence_counts.
    Windows: chromosome id i64, START, END (host arrays, any order, doubled or overlapping; the rows' chromosome ids name the same
    chromosomes).  Rows: chrom, start, end i64; type i32 = the row's row of mk_mutation_context, K for a label pair the table does
    not hold; cohort i32 within [0, C).  A row counts once however many windows hold it: the reference's rule for one-base rows
    (restrict_mutations_by_bed(unique=True)); the caller keeps other rows out (sequence_tools.train_sequence_models).
    Returns counts i64 [C, K]; CUDA tensors in (the row arrays) -> a CUDA tensor."""
    be = backend_of(row_chrom, row_start, row_end, row_type, row_cohort, device=device)
    K, C = int(K), int(C)
    _, start_key, runmax_key, blk_end = _window_blocks(win_chrom, win_start, win_end)
    row_chrom, row_start, row_end = (be.arr(x, "i64", (-1,)) for x in (row_chrom, row_start, row_end))
    row_type, row_cohort = be.arr(row_type, "i32", (-1,)), be.arr(row_cohort, "i32", (-1,))
    n = row_chrom.shape[0]
    assert row_start.shape[0] == row_end.shape[0] == row_type.shape[0] == row_cohort.shape[0] == n
    if be.is_device:
        # (device tensors are checked here; the host twin checks its own arrays inside the library)
        if K < 1 or C < 1:
            raise ValueError("K >= 1, C >= 1")
        if n and bool(((row_cohort < 0) | (row_cohort >= C) | (row_type < 0) | (row_type > K)).any()):
            raise ValueError("a row outside the tables: cohort within [0, C), type within [0, K]")
    pair_row, _ = overlap_join(be, start_key, runmax_key, blk_end, row_chrom, row_start, row_end, max_pairs=2 ** 31 - 1,
                               too_many="%d (row, window) pairs: the join's pair indices are 32-bit; fewer cohorts per call")
    p = be.ptr
    counts = be.empty((max(C, 0), max(K, 0)), "i64")
    with _requirements_as_value_errors():
        be.call("dig_sequence_counts", p(pair_row), pair_row.shape[0], p(row_type), p(row_cohort), n, K, C, p(counts))
    return counts


SITE_COUNT_BLOCK = 256          # csrc/dig_sitematch.hip kSiteBlock: the workgroup of dig_site_counts (the tests place runs at its edges)


def site_counts(site_pos, site_end, site_attr, site_elt, row_pos, row_end, row_attr, row_sample, row_cohort, sample_offsets, E, C,
                device=0):
    """The sites route's observed counts for C cohorts at once (mutation_tools.py:233-281 tabulate_nonc_mutations_at_sites: the inner
    merge on nine columns and the group-by per element): dig_site_match_count, a cumulative sum, dig_site_match_keys, a key sort,
    dig_site_counts.
    Sites (data_tools/sites.encode_sites_file): pos = chrom << 40 | START ascending, end, attr i64 [S]; elt i32 [S] within [0, E).
    Rows of all cohorts in any order (sites.encode_site_rows): pos, end, attr i64 [n] (attr < 0: matches nothing); sample i32 = the
    GLOBAL sample, inside its cohort's range of sample_offsets [C + 1]; cohort i32.
    Returns dict(obs_snv, obs_samples), i32 [E, C]: matched (row, site) pairs and distinct samples among them per (element, cohort).
    ValueError, before the fill, for more than 2^31 - 1 matches.  CUDA tensors in -> CUDA tensors out."""
    be = backend_of(site_pos, site_end, site_attr, site_elt, row_pos, row_end, row_attr, row_sample, row_cohort, device=device)
    E = int(E)
    off_host, C, n_samples = _sample_offsets(sample_offsets, int(C))
    site_pos, site_end, site_attr = (be.arr(x, "i64", (-1,)) for x in (site_pos, site_end, site_attr))
    site_elt = be.arr(site_elt, "i32", (-1,))
    row_pos, row_end, row_attr = (be.arr(x, "i64", (-1,)) for x in (row_pos, row_end, row_attr))
    row_sample, row_cohort = be.arr(row_sample, "i32", (-1,)), be.arr(row_cohort, "i32", (-1,))
    S, n = site_pos.shape[0], row_pos.shape[0]
    assert site_end.shape[0] == site_attr.shape[0] == site_elt.shape[0] == S
    assert row_end.shape[0] == row_attr.shape[0] == row_sample.shape[0] == row_cohort.shape[0] == n
    off = be.arr(off_host, "i64")
    if be.is_device:
        # (device tensors are checked here; the host twins check their own arrays inside the library)
        if S and (bool(((site_elt < 0) | (site_elt >= E)).any()) or bool((site_pos[1:] < site_pos[:-1]).any())):
            raise ValueError("the site table: site_pos ascending, elements within [0, E)")
        if n:
            c = row_cohort.clamp(0, C - 1).long()
            if bool(((row_cohort < 0) | (row_cohort >= C) | (row_sample < off[c]) | (row_sample >= off[c + 1])).any()):
                raise ValueError("a row outside the tables: cohort within [0, C), global sample within its cohort")
    p = be.ptr
    search = [p(site_pos), p(site_end), p(site_attr), p(site_elt), S, E, p(row_pos), p(row_end), p(row_attr), p(row_sample),
              p(row_cohort), p(off), n, C, n_samples]
    with _requirements_as_value_errors():
        counts = be.empty(n, "i32")
        be.call("dig_site_match_count", *search, p(counts))
        offsets, total = _scan(be, counts)
        if total > 2 ** 31 - 1:
            raise ValueError("%d (row, site) matches: the observed counts are 32-bit; pass fewer cohorts per call" % total)
        keys = be.empty(total, "i64")
        be.call("dig_site_match_keys", *search, p(offsets), total, p(keys))
        keys = _sorted(be, keys)
        obs_snv, obs_samples = be.empty((E, C), "i32"), be.empty((E, C), "i32")
        be.call("dig_site_counts", p(keys), total, E, C, n_samples, p(obs_snv), p(obs_samples))
    return dict(obs_snv=obs_snv, obs_samples=obs_samples)


def gene_pipeline(bin_mu, bin_std, bin_y, bin_flag, bin_ctx, ov_ptr, ov_idx, L, strand_minus, gene_length, d_pr, obs, n_samp, cj,
                  t_indel=None):
    """genic_model (genic_driver_tools.py:31-203) + the gene statistics block as one call on device tensors
    (dig_gene_pipeline): L i32 [G, 4, 192] (silent, missense, nonsense, splice columns), gene_length i32 [G].
    Returns (accumulate dict with P [G, 4, C], dict of the 22 statistics planes)."""
    be = device_backend(bin_mu.device)
    tabs, (N, G, C, n_class) = _bin_tables(be, bin_mu, bin_std, bin_y, bin_flag, bin_ctx, ov_ptr, ov_idx, L, strand_minus,
                                           gene_length, d_pr)
    assert n_class == 4
    obs, n_samp, cj, ti = _gene_observations(be, obs, n_samp, cj, t_indel, G, C)
    o = _accumulate_outputs(be, G, C, 4)
    out = be.empty((len(GS_PLANES), G, C), "f64")
    p = be.ptr
    be.call("dig_gene_pipeline", *[p(x) for x in tabs], p(obs), p(n_samp), p(cj), p(ti), int(ti is not None),
            *[p(o[k]) for k in _ACC_OUTPUTS], p(out), N, G, C, workspace=_shared_workspace(be, "accumulate", G, C))
    return o, {name: out[i] for i, name in enumerate(GS_PLANES)}


# ---------------------------------------------------------------------------
def scale_suffstats(bin_mu, bin_flag, device=0, out=None):
    """Per-cohort sum of Y_PRED over unflagged bins (transfer_tools.py:148-156): [N, C] -> [C]."""
    be = backend_of(bin_mu, device=device)
    bin_mu = _cols(be.arr(bin_mu, "f64"))
    N, C = bin_mu.shape
    bin_flag = be.arr(bin_flag, "u8", (N, C))
    if out is None:
        out = be.empty(C, "f64")
    be.call("dig_scale_suffstats", be.ptr(bin_mu), be.ptr(bin_flag), N, C, be.ptr(out), workspace=_shared_workspace(be, "suffstats", N, C))
    return out


def scale_factors_local(bin_mu, bin_flag, n_snv_obs, n_ind_obs, out=None):
    """Single-shard scale factors (transfer_tools.py:148-156): masked column sums and the two divisions in one pair of
    kernels (dig_scale_factors_local).  Returns (cj, cj_indel, exp_sum) device tensors."""
    be = device_backend(bin_mu.device)
    bin_mu, bin_flag = be.arr(bin_mu, "f64"), be.arr(bin_flag, "u8")
    N, C = bin_mu.shape
    n_snv_obs, n_ind_obs = be.arr(n_snv_obs, "f64"), be.arr(n_ind_obs, "f64")
    if out is None:
        out = tuple(be.empty(C, "f64") for _ in range(3))
    p = be.ptr
    be.call("dig_scale_factors_local", p(bin_mu), p(bin_flag), N, C, p(n_snv_obs), p(n_ind_obs), p(out[2]), p(out[0]), p(out[1]),
            workspace=_shared_workspace(be, "suffstats", N, C))
    return out


def scale_factors_from_parts(parts, out=None):
    """cj, cj_indel from the all-gathered per-shard statistics `parts` f64 [world, 3, C] on the device
    (rank-ordered sums + division in one kernel; transfer_tools.py:153-154)."""
    be = device_backend(parts.device)
    parts = be.arr(parts, "f64")
    world, three, C = parts.shape
    assert three == 3
    if out is None:
        out = (be.empty(C, "f64"), be.empty(C, "f64"))
    be.call("dig_scale_factors", be.ptr(parts), world, C, be.ptr(out[0]), be.ptr(out[1]))
    return out


# ---------------------------------------------------------------------------
def ideal_overlaps(elt_chrom, blk_ptr, blk_start, blk_end, window, bin_chrom, bin_start):
    """CSR of overlapped bin rows per element (genic_driver_tools.py:275-283), ascending rows.
    Host-side integer index construction in the C++ runtime."""
    elt_chrom = _lib.as_host(elt_chrom, np.int32)
    blk_ptr = _lib.as_host(blk_ptr, np.int64)
    blk_start = _lib.as_host(blk_start, np.int64)
    blk_end = _lib.as_host(blk_end, np.int64)
    bin_chrom = _lib.as_host(bin_chrom, np.int32)
    bin_start = _lib.as_host(bin_start, np.int64)
    E, N = len(elt_chrom), len(bin_chrom)
    ov_ptr = np.zeros(E + 1, np.int64)
    args = [_lib.host_ptr(elt_chrom), _lib.host_ptr(blk_ptr), _lib.host_ptr(blk_start), _lib.host_ptr(blk_end), E,
            int(window), _lib.host_ptr(bin_chrom), _lib.host_ptr(bin_start), N, _lib.host_ptr(ov_ptr)]
    _lib.call("dig_ideal_overlaps_host", *args, None)
    ov_idx = np.zeros(max(int(ov_ptr[E]), 1), np.int32)
    _lib.call("dig_ideal_overlaps_host", *args, _lib.host_ptr(ov_idx))
    return ov_ptr, ov_idx[:int(ov_ptr[E])]


_ACC_OUTPUTS = ("MU", "SIGMA", "R_OBS", "FLAG", "P", "R_SIZE", "ELT_SIZE", "P_INDEL")       # in the library's argument order


def _accumulate_outputs(be, E, C, n_class):
    return dict(MU=be.empty((E, C), "f64"), SIGMA=be.empty((E, C), "f64"), R_OBS=be.empty((E, C), "i32"),
                FLAG=be.empty((E, C), "i32"), P=be.empty((E, n_class, C), "f64"), R_SIZE=be.empty(E, "i32"),
                ELT_SIZE=be.empty(E, "i32"), P_INDEL=be.empty(E, "f64"))


def alloc_accumulate_outputs(E, C, n_class, dev):
    """Output tensors of accumulate_elements (reusable across calls through `out=`)."""
    return _accumulate_outputs(device_backend(dev), E, C, n_class)


def _bin_tables(be, bin_mu, bin_std, bin_y, bin_flag, bin_ctx, ov_ptr, ov_idx, L, strand_minus, gene_length, d_pr):
    """The bin tables, the overlap CSR and the element table every accumulation takes, normalised: bin_mu, bin_std f64 [N, C];
    bin_y i32 [N, C]; bin_flag u8 [N, C]; bin_ctx i32 [N, 64]; ov_ptr i64 [E + 1]; ov_idx i32; L i32 [E, n_class, 192] (an
    [E, 192] table is one class); strand_minus u8 [E]; gene_length i32 [E] or None; d_pr f64 [C, 192].
    Returns (the eleven arrays in that order, (N, E, C, n_class))."""
    bin_mu = _cols(be.arr(bin_mu, "f64"))
    N, C = bin_mu.shape
    L = be.arr(L, "i32")
    if L.ndim == 2:
        L = L[:, None, :]
    E, n_class, K = L.shape
    ov_ptr, ov_idx = be.arr(ov_ptr, "i64"), be.arr(ov_idx, "i32")
    assert K == 192 and ov_ptr.shape[0] == E + 1
    if not be.is_device and ov_idx.shape[0] == 0:               # (the staging helper of the host twins copies at least one entry)
        ov_idx = be.arr([0], "i32")
    return [bin_mu, be.arr(bin_std, "f64", (N, C)), be.arr(bin_y, "i32", (N, C)), be.arr(bin_flag, "u8", (N, C)),
            be.arr(bin_ctx, "i32", (N, 64)), ov_ptr, ov_idx, L, be.arr(strand_minus, "u8"), be.arr(gene_length, "i32"),
            be.arr(d_pr, "f64", (C, 192))], (N, E, C, n_class)


def accumulate_elements(bin_mu, bin_std, bin_y, bin_flag, bin_ctx, ov_ptr, ov_idx, L, strand_minus, d_pr,
                        gene_length=None, device=0, out=None, use_workspace=True):
    """Per-element accumulation for all cohorts (see include/dig_hip.h: dig_accumulate_elements).

    Returns dict(MU, SIGMA [E,C] f64; R_OBS, FLAG [E,C] i32; P [E,n_class,C] f64;
                 R_SIZE, ELT_SIZE [E] i32; P_INDEL [E] f64)."""
    be = backend_of(bin_mu, device=device)
    tabs, (N, E, C, n_class) = _bin_tables(be, bin_mu, bin_std, bin_y, bin_flag, bin_ctx, ov_ptr, ov_idx, L, strand_minus,
                                           gene_length, d_pr)
    o = out if out is not None else _accumulate_outputs(be, E, C, n_class)
    p = [be.ptr(x) for x in tabs]
    be.call("dig_accumulate_elements", *p[:8], n_class, *p[8:], *[be.ptr(o[k]) for k in _ACC_OUTPUTS], N, E, C,
            workspace=_shared_workspace(be, "accumulate", E, C, use_workspace))
    return o


# ---------------------------------------------------------------------------
def element_pipeline(bin_mu, bin_std, bin_y, bin_flag, bin_ctx, ov_ptr, ov_idx, L, strand_minus, d_pr, obs_snv,
                     obs_samples, obs_indel, cj, cj_indel, gene_length=None, out_acc=None, out_stats=None, stages=7, compact=False):
    """accumulate_elements (n_class = 1) + element_stats as one operation on device tensors (dig_element_pipeline):
    the rate sums are formed inside the statistics kernel.  Returns (accumulate dict, statistics tensor [7, E, C]).
    stages: bit mask 1 = context kernel, 2 = dot kernel, 4 = statistics (7 = all); separate calls must keep that order.
    compact="auto": check L for the three-fold context repetition first (one more pass over L and a stream synchronisation,
    see PipelinePlan) and run the 64-context form when it holds; a loop over the same element set should keep a PipelinePlan."""
    if compact:
        plan = PipelinePlan(bin_mu, bin_std, bin_y, bin_flag, bin_ctx, ov_ptr, ov_idx, L, strand_minus, d_pr, obs_snv, obs_samples,
                            obs_indel, out_acc=out_acc, out_stats=out_stats, gene_length=gene_length, compact=compact,
                            pack_bins=False, element_contexts=False,   # (one call: packing the tables, or summing the context rows
                            element_rates=False, element_p=False)      #  or the rates, or keeping P, in kernels of their own, would cost more than it saves)
        return plan.run(_t(cj, "f64", plan.dev), _t(cj_indel, "f64", plan.dev), stages=stages)
    be = device_backend(bin_mu.device)
    tabs, (N, E, C, n_class) = _bin_tables(be, bin_mu, bin_std, bin_y, bin_flag, bin_ctx, ov_ptr, ov_idx, L, strand_minus,
                                           gene_length, d_pr)
    assert n_class == 1
    obs = [be.arr(x, "i32") for x in (obs_snv, obs_samples, obs_indel)]
    assert all(x.shape == (E, C) for x in obs)
    cj, cj_indel = be.arr(cj, "f64"), be.arr(cj_indel, "f64")
    o = out_acc if out_acc is not None else _accumulate_outputs(be, E, C, 1)
    st = out_stats if out_stats is not None else be.empty((len(ES_PLANES), E, C), "f64")
    ws = _shared_workspace(be, "pipeline", E, C)
    if ws[0] is None:
        raise _lib.DigHipError("dig_element_pipeline: problem too large for the fused path (E * C >= 2^32 - 1)")
    p = be.ptr
    be.call("dig_element_pipeline", *[p(x) for x in tabs], *[p(x) for x in obs], p(cj), p(cj_indel), *[p(o[k]) for k in _ACC_OUTPUTS],
            p(st), N, E, C, None, int(stages), workspace=ws)
    return o, st


_RECORDS_FASTER = {}          # device index -> whether the record form of the statistics outputs is the faster one there


def records_form_is_faster(plane_plan, record_plan, cj, cj_indel, rounds=2, warm=8, launches=25):
    """Which layout of the statistics stage's outputs is the faster one on THIS card: eleven planes, or tile-blocked records
    (PipelinePlan(records_out=True))?  The pool's MI355X fall into two kinds -- on most the eleven store streams of the plane
    form cost ~ 10 us of a 180-us pass in a loop, on the others the record form does.  Developer A/B
    (`bench.py --outputs auto`): whole passes of the two plans (same inputs), best of `rounds` x `launches` behind `warm` untimed
    ones (bursts of five measure the clocks coming up, not the forms), HIP events on torch's current stream; a tie keeps the
    planes; once per process and device.  Returns (bool, {"planes": us, "records": us})."""
    import torch
    key = plane_plan.dev.index
    if key in _RECORDS_FASTER:
        return _RECORDS_FASTER[key]
    us = {}
    with torch.cuda.device(plane_plan.dev):
        for name, pl in (("planes", plane_plan), ("records", record_plan)):
            best = float("inf")
            for _ in range(rounds):
                ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                for _w in range(warm):
                    pl.run(cj, cj_indel)
                ea.record()
                for _r in range(launches):
                    pl.run(cj, cj_indel)
                eb.record()
                eb.synchronize()
                best = min(best, ea.elapsed_time(eb) / launches * 1e3)
            us[name] = best
    _RECORDS_FASTER[key] = (us["records"] < us["planes"] - 1.5, us)
    return _RECORDS_FASTER[key]


class PipelinePlan:
    """dig_element_pipeline / dig_scale_factors_local with the argument marshalling done ONCE, for loops that run
    the same tensors many times (the driver's cohort loop, bench.py): a call is then one ctypes invocation (~10 us of
    host time instead of ~60), which keeps the host ahead of a 0.3 ms GPU step.  The tensors are held by the plan."""

    _ws_owner = {}         # data_ptr of a caller-owned workspace -> weak reference to the plan that owns it

    def __init__(self, bin_mu, bin_std, bin_y, bin_flag, bin_ctx, ov_ptr, ov_idx, L, strand_minus, d_pr, obs_snv,
                 obs_samples, obs_indel, out_acc=None, out_stats=None, gene_length=None, compact="auto", workspace=None,
                 pack_bins=True, records_out=False, element_contexts=True, element_rates=True, element_p=True):
        """compact: "auto" (default) checks ONCE, here, on the device whether L repeats every context count three times
        (sequence_tools.py:560-564: true for every elementModel / tiledModel / quickDriver set) and, if so, runs the
        64-context form of the accumulation (contexts + dot in one kernel, half the matrix work); False forces the
        general 192-substitution form.  `self.compact` tells which one runs.
        pack_bins: rewrite the four bin tables ONCE, here, as the packed records the statistics stage gathers from
        (dig_bin_records_pack: 20 bytes per (bin, cohort) of plan-owned memory, two gathers per bin instead of four, same
        bits).  The plan then reads the records, not the tables: call `repack_bins()` after changing a table in place.
        Another PipelinePlan over the same tables may be given instead of True: its records are shared.
        records_out: the statistics stage writes tile-blocked records (DIG_PIPE_RECORDS: the ten outputs of a pair -- seven
        statistics, MU, SIGMA, R_OBS | FLAG -- as field f of block i / 64 at [f / 2, i % 64, f % 2]: one aligned 5 120-byte run
        per 64-pair tile instead of eleven store streams) into `self.out_records` [ceil(E C / 64), 5, 64, 2]; `self.stats` and
        MU / SIGMA / R_OBS / FLAG of `self.acc` are filled by `unpack()` (same bits).  Needs the packed bin records (pack_bins).
        element_contexts: a compact plan sums the context rows of every element's bins ONCE, here (dig_element_contexts_prepare:
        a plan-owned [E, 64] int32 table, `self.elt_ctx`, outside the workspace), and its dot kernel streams that table instead
        of walking the overlaps and gathering bin rows every call (DIG_PIPE_ELEMENT_CTX; integer sums: same bits).  The plan then
        reads the table, not bin_ctx / ov_ptr / ov_idx / strand_minus (the statistics stage reads the overlaps in its live form only: element_rates): call
        `recontext()` after changing one of them in place.  Another PipelinePlan over the same tables and element set may be
        given instead of True: its table is shared.  A plan that is not compact ignores the option.
        element_rates: a plan with packed bin records forms the rate sums of every (element, cohort) pair -- MU, SIGMA, R_OBS, FLAG --
        ONCE, here (dig_element_rates_prepare: a plan-owned table of 24 bytes per pair, `self.elt_rates`, outside the workspace),
        and its statistics kernel streams that table instead of walking the overlaps and gathering bin records every call
        (DIG_PIPE_ELEMENT_RATES; the live form's additions in its order: same bits).  The statistics stage then reads the table, not
        the records or ov_ptr / ov_idx: `repack_bins()` and `recontext()` both rebuild it, since the tables and the overlaps both
        feed it.  Another PipelinePlan over the same records and overlaps may be given instead of True: its table is shared.  A plan
        without packed records ignores the option and sums per call.  A caller that builds a plan and runs it ONCE passes False
        (engine.element_pipeline, cohort_batch._element_planes): for it the table is an extra write and read of 24 bytes per pair
        and saves nothing.
        element_p: P, R_SIZE, ELT_SIZE and P_INDEL depend on nothing a run() is given (L, the context rows, gene_length and d_pr
        all belong to the plan).  The plan runs its own accumulation stages ONCE, here, in whichever form it has (compact, planned
        contexts, general), keeps bit copies of the four outputs in a plan-owned table (dig_element_p_prepare: `self.elt_p`,
        8 bytes per pair + 16 per element, outside the workspace), and the DOT stage of every run() streams them back into the
        plan's outputs instead of forming them again (DIG_PIPE_ELEMENT_P; copies: same bits).  All four outputs are still written
        by every run.  The plan then snapshots L, d_pr, gene_length, bin_ctx, the overlaps and the strands: call `recontext()`
        after changing one of them in place.  Another PipelinePlan over the same inputs may be given instead of True: its table
        is shared.  A caller that builds a plan and runs it ONCE passes False (as for element_rates)."""
        import ctypes
        import torch
        dev = bin_mu.device
        be = device_backend(dev)
        tabs, (self.N, self.E, self.C, n_class) = _bin_tables(be, bin_mu, bin_std, bin_y, bin_flag, bin_ctx, ov_ptr, ov_idx, L,
                                                              strand_minus, gene_length, d_pr)
        assert n_class == 1
        L = tabs[7]
        self.keep = tabs + [be.arr(x, "i32") for x in (obs_snv, obs_samples, obs_indel)]
        assert all(x.shape == (self.E, self.C) for x in self.keep[11:14])
        self.dev = dev
        self.acc = out_acc if out_acc is not None else _accumulate_outputs(be, self.E, self.C, 1)
        self.stats = out_stats if out_stats is not None else be.empty((len(ES_PLANES), self.E, self.C), "f64")
        if workspace is not None:
            # A caller-owned buffer (uint8, at least dig_element_pipeline_workspace bytes).  NOT plain scratch: a compact plan
            # keeps its [E, 64] copy of L and the repetition flag in it from construction on (dig_element_pipeline_prepare), so
            # the buffer belongs to THIS plan (or to plans over the very same L tensor) for the plan's lifetime -- two live plans
            # over different element sets on one buffer would compute P from each other's L: refused below.
            self.ws, self.wsb = workspace, _lib.workspace_bytes("pipeline", self.E, self.C)
            assert workspace.numel() >= self.wsb and workspace.data_ptr() % 256 == 0
            import weakref
            owner = PipelinePlan._ws_owner.get(workspace.data_ptr())
            if owner is not None and owner[0]() is not None and owner[0]() is not self and owner[1] != (L.data_ptr(), tuple(L.shape)):
                raise ValueError("this workspace buffer already belongs to a live PipelinePlan over ANOTHER element set (a compact "
                                 "plan keeps its copy of L in it): give every plan its own workspace")
            PipelinePlan._ws_owner[workspace.data_ptr()] = (weakref.ref(self), (L.data_ptr(), tuple(L.shape)))
        else:
            self.ws, self.wsb = _workspace("pipeline", self.E, self.C, dev, private=True)
        if self.ws is None:
            raise _lib.DigHipError("dig_element_pipeline: problem too large for the fused path (E * C >= 2^32 - 1)")
        p = _lib.dev_ptr
        o = self.acc
        self._head = [p(x) for x in self.keep]
        self.records = None
        if isinstance(pack_bins, PipelinePlan):              # several plans over the SAME bin tables share one set of records
            assert pack_bins.keep[0].data_ptr() == self.keep[0].data_ptr() and (pack_bins.N, pack_bins.C) == (self.N, self.C)
            self.records = pack_bins.records
        elif pack_bins and self.N >= 1:
            nb = int(_lib.load().dig_bin_records_bytes(self.N, self.C))
            self.records = torch.empty(nb, dtype=torch.uint8, device=dev)
            self.repack_bins()
        self.records_out = bool(records_out)
        self.out_records = None
        if self.records_out:
            if self.records is None:
                raise ValueError("records_out needs the packed bin records (pack_bins)")
            nrec = (self.E * self.C + 63) // 64 * 64
            self.out_records = torch.empty((nrec // 64, _lib.DIG_REC_DOUBLES // 2, 64, 2), dtype=torch.float64, device=dev)
            assert self.out_records.data_ptr() % 256 == 0
        self._tail = [p(o["MU"]), p(o["SIGMA"]), p(o["R_OBS"]), p(o["FLAG"]), p(o["P"]), p(o["R_SIZE"]), p(o["ELT_SIZE"]),
                      p(o["P_INDEL"]), p(self.out_records if self.records_out else self.stats), self.N, self.E, self.C,
                      p(self.records)]
        self._ws = p(self.ws)
        self._fn = getattr(_lib.load(), "dig_element_pipeline")
        self.compact = False
        if compact and self.N >= 1:
            ok = ctypes.c_int(0)
            with torch.cuda.device(dev):
                _lib.call("dig_element_pipeline_prepare", p(L), self.E, self.C, self._ws, self.wsb, ctypes.byref(ok),
                          _lib.stream_ptr())
            self.compact = bool(ok.value)
        self._flags = (_lib.DIG_PIPE_COMPACT_L if self.compact else 0) | (_lib.DIG_PIPE_RECORDS if self.records_out else 0)
        self.elt_ctx = None
        if self.compact and element_contexts:
            if isinstance(element_contexts, PipelinePlan):    # several plans over the SAME bins and element set share one table
                other = element_contexts
                assert other.elt_ctx is not None and (other.N, other.E) == (self.N, self.E)
                assert all(other.keep[i].data_ptr() == self.keep[i].data_ptr() for i in (4, 5, 6, 8))
                self.elt_ctx = other.elt_ctx
            else:
                self.elt_ctx = torch.empty((self.E, 64), dtype=torch.int32, device=dev)
                assert self.elt_ctx.data_ptr() % 256 == 0
                self.recontext()
            self._head[4] = p(self.elt_ctx)                   # the `bin_ctx` slot (self.keep still holds the bin table)
            self._flags |= _lib.DIG_PIPE_ELEMENT_CTX
        self.elt_rates = None
        if self.records is not None and element_rates:
            if isinstance(element_rates, PipelinePlan):       # several plans over the SAME records and overlaps share one table
                other = element_rates
                assert other.elt_rates is not None and (other.N, other.E, other.C) == (self.N, self.E, self.C)
                assert other.records.data_ptr() == self.records.data_ptr()
                assert all(other.keep[i].data_ptr() == self.keep[i].data_ptr() for i in (5, 6))
                self.elt_rates = other.elt_rates
            else:
                self.elt_rates = torch.empty(int(_lib.load().dig_element_rates_bytes(self.E, self.C)), dtype=torch.uint8, device=dev)
                assert self.elt_rates.data_ptr() % 256 == 0
                self._rerate()
            self._head[0] = p(self.elt_rates)                 # the `bin_mu` slot (self.keep still holds the bin table)
            self._flags |= _lib.DIG_PIPE_ELEMENT_RATES
        self.elt_p = None
        self._live_flags, self._live_d_pr = self._flags, self._head[10]     # the accumulation form that fills the table
        if element_p:
            if isinstance(element_p, PipelinePlan):           # several plans over the SAME accumulation inputs share one table
                other = element_p
                assert other.elt_p is not None and (other.N, other.E, other.C, other.compact) == (self.N, self.E, self.C, self.compact)
                assert all(other.keep[i].data_ptr() == self.keep[i].data_ptr() for i in (4, 5, 6, 7, 8, 10))
                assert (other.keep[9] is None) == (self.keep[9] is None)
                assert self.keep[9] is None or other.keep[9].data_ptr() == self.keep[9].data_ptr()
                self.elt_p = other.elt_p
            else:
                self.elt_p = torch.empty(int(_lib.load().dig_element_p_bytes(self.E, self.C)), dtype=torch.uint8, device=dev)
                assert self.elt_p.data_ptr() % 256 == 0
                self._reform_p(recompact=False)               # (L was compacted just above)
            self._head[10] = p(self.elt_p)                    # the `d_pr` slot (self.keep still holds the parameters)
            self._flags |= _lib.DIG_PIPE_ELEMENT_P

    def unpack(self, cohort_major=False, stream=None, stats=None, rates=None):
        """records_out plans: out_records -> the plane form (self.stats [7, E, C] and MU, SIGMA, R_OBS, FLAG of self.acc) on
        `stream`; cohort_major=True writes every plane as [C, E] instead (a result frame's column is then one contiguous row)
        into `stats` [7, C, E] (required then) and, when given, `rates` = dict(MU, SIGMA: float64 [C, E]; R_OBS, FLAG: int32
        [C, E]); self.acc is left alone."""
        import torch
        assert self.records_out
        p = _lib.dev_ptr
        o = self.acc
        with torch.cuda.device(self.dev):
            if cohort_major:
                assert stats is not None and tuple(stats.shape) == (len(ES_PLANES), self.C, self.E)
                r = rates or {}
                assert all(tuple(v.shape) == (self.C, self.E) and v.is_contiguous() for v in r.values())
                assert all(r[k].dtype == (torch.float64 if k in ("MU", "SIGMA") else torch.int32) for k in r)
                _lib.call("dig_element_records_unpack", p(self.out_records), self.E, self.C, p(stats), p(r.get("MU")), p(r.get("SIGMA")),
                          p(r.get("R_OBS")), p(r.get("FLAG")), 1, _lib.stream_ptr(stream))
                return stats
            st = self.stats if stats is None else stats
            _lib.call("dig_element_records_unpack", p(self.out_records), self.E, self.C, p(st), p(o["MU"]), p(o["SIGMA"]),
                      p(o["R_OBS"]), p(o["FLAG"]), 0, _lib.stream_ptr(stream))
        return o, st

    def repack_bins(self):
        """(Re)build the packed bin records from the plan's bin tables on torch's current stream (waits for it), and the table of
        the pairs' rate sums from them (enqueued behind it)."""
        import torch
        if self.records is None:
            return
        k = self.keep
        with torch.cuda.device(self.dev):
            _lib.call("dig_bin_records_pack", _lib.dev_ptr(k[0]), _lib.dev_ptr(k[1]), _lib.dev_ptr(k[2]), _lib.dev_ptr(k[3]),
                      self.N, self.C, _lib.dev_ptr(self.records), self.records.numel(), _lib.stream_ptr())
        self._rerate()

    def _rerate(self):
        """(Re)build the table of the pairs' rate sums from the packed bin records and the overlaps on torch's current stream
        (enqueued, not waited for)."""
        import torch
        if getattr(self, "elt_rates", None) is None:
            return
        k = self.keep
        with torch.cuda.device(self.dev):
            _lib.call("dig_element_rates_prepare", _lib.dev_ptr(self.records), _lib.dev_ptr(k[5]), _lib.dev_ptr(k[6]), self.N, self.E,
                      self.C, _lib.dev_ptr(self.elt_rates), self.elt_rates.numel(), _lib.stream_ptr())

    def _reform_p(self, recompact=True):
        """(Re)build the table of P, P_INDEL, R_SIZE and ELT_SIZE on torch's current stream (enqueued, not waited for): the plan's
        own accumulation stages (CONTEXTS | DOT in its live form, with its context table when it has one) into its outputs, then
        bit copies of the four into the table.  recompact: a compact plan compacts L into its workspace again first (L may have
        changed in place; checks the repetition and waits for the stream)."""
        import torch
        if getattr(self, "elt_p", None) is None:
            return
        o = self.acc
        head = list(self._head)
        head[10] = self._live_d_pr
        with torch.cuda.device(self.dev):
            if self.compact and recompact:
                import ctypes
                ok = ctypes.c_int(0)
                _lib.call("dig_element_pipeline_prepare", _lib.dev_ptr(self.keep[7]), self.E, self.C, self._ws, self.wsb, ctypes.byref(ok),
                          _lib.stream_ptr())
                if not ok.value:
                    raise ValueError("L no longer repeats every context count three times: a compact plan cannot take it (build a new plan)")
            # (cj / cj_indel are statistics arguments: checked for NULL, not read by these stages -- any device pointer serves)
            rc = self._fn(*head, self._tail[8], self._tail[8], *self._tail, _lib.DIG_PIPE_CONTEXTS | _lib.DIG_PIPE_DOT | self._live_flags,
                          self._ws, self.wsb, _lib.stream_ptr())
            _lib.check("dig_element_pipeline", rc)
            _lib.call("dig_element_p_prepare", _lib.dev_ptr(o["P"]), _lib.dev_ptr(o["R_SIZE"]), _lib.dev_ptr(o["ELT_SIZE"]),
                      _lib.dev_ptr(o["P_INDEL"]), self.E, self.C, _lib.dev_ptr(self.elt_p), self.elt_p.numel(), _lib.stream_ptr())

    def recontext(self):
        """(Re)build what the plan snapshots of L, d_pr, gene_length, bin_ctx, the overlaps (ov_ptr, ov_idx) and the strands, on
        torch's current stream: the table of the elements' summed context rows (bin_ctx, overlaps, strands), the table of the
        pairs' rate sums (packed bin records, overlaps) and, after the context table, the table of P, P_INDEL, R_SIZE and ELT_SIZE
        (all six; a compact plan compacts L again, which waits for the stream).  The tables are enqueued, not waited for."""
        import torch
        self._rerate()
        if self.elt_ctx is not None:
            k = self.keep
            with torch.cuda.device(self.dev):
                _lib.call("dig_element_contexts_prepare", _lib.dev_ptr(k[4]), _lib.dev_ptr(k[5]), _lib.dev_ptr(k[6]), _lib.dev_ptr(k[8]),
                          self.N, self.E, _lib.dev_ptr(self.elt_ctx), _lib.stream_ptr())
        self._reform_p()

    def run(self, cj, cj_indel, stages=7, stream=None):
        """Enqueue the pipeline (or one of its stages) on `stream` (default: torch's current stream)."""
        rc = self._fn(*self._head, _lib.dev_ptr(cj), _lib.dev_ptr(cj_indel), *self._tail, int(stages) | self._flags, self._ws,
                      self.wsb, _lib.stream_ptr(stream))
        _lib.check("dig_element_pipeline", rc)
        return self.acc, self.stats


class PlanRing:
    """Several PipelinePlans -- one per batch in flight, each with its own outputs and workspace -- taking turns on as
    many streams.  A pass is a chain of dependent kernels (contexts -> dot -> statistics) and each of them leaves part of
    the chip idle while it ramps up and while its last waves finish; with two passes over different batches in flight
    the kernels of one fill those gaps of the other: 188 us per pass against 193 us one after the other on an MI355X at
    the whole-genome x 37-cohort size (tools/overlap_probe.py; 186 against 207 while the pass still had a fourth kernel).  The caller keeps the
    order of the passes on ONE plan (they share a stream); passes on different plans are independent."""

    def __init__(self, plans, streams=None):
        import torch
        self.plans = list(plans)
        assert self.plans, "at least one plan"
        dev = self.plans[0].dev
        self.streams = list(streams) if streams is not None else [torch.cuda.Stream(device=dev) for _ in self.plans]
        assert len(self.streams) == len(self.plans)

    def run(self, k, cj, cj_indel):
        """Enqueue pass k on plan k mod len(plans); returns that plan's (accumulation outputs, statistics planes), valid
        once the plan's stream has been synchronised."""
        j = k % len(self.plans)
        return self.plans[j].run(cj, cj_indel, stream=self.streams[j])

    def synchronize(self):
        for s in self.streams:
            s.synchronize()


class ScaleFactorPlan:
    """dig_scale_factors_local with cached arguments (see PipelinePlan)."""

    def __init__(self, bin_mu, bin_flag, n_snv_obs, n_ind_obs):
        import torch
        dev = bin_mu.device
        self.keep = [_t(bin_mu, "f64", dev), _t(bin_flag, "u8", dev), _t(n_snv_obs, "f64", dev),
                     _t(n_ind_obs, "f64", dev)]
        self.N, self.C = self.keep[0].shape
        self.ws, self.wsb = _workspace("suffstats", self.N, self.C, dev, private=True)
        p = _lib.dev_ptr
        self._args = [p(self.keep[0]), p(self.keep[1]), self.N, self.C, p(self.keep[2]), p(self.keep[3])]
        self._ws = p(self.ws)
        self._fn = getattr(_lib.load(), "dig_scale_factors_local")

    def run(self, out_sum, cj, cj_indel, stream=None):
        rc = self._fn(*self._args, _lib.dev_ptr(out_sum), _lib.dev_ptr(cj), _lib.dev_ptr(cj_indel), self._ws, self.wsb,
                      _lib.stream_ptr(stream))
        _lib.check("dig_scale_factors_local", rc)

    def run_sharded(self, part, cj, cj_indel, group=None):
        """Bins sharded over ranks: this shard's sums into part[0] (dig_scale_suffstats), all-gather of the [3, C]
        parts over the process group, rank-ordered sum + division (dig_scale_factors).  Runs on torch's CURRENT stream
        (the collective follows it)."""
        import torch
        import torch.distributed as dist
        lib = _lib.load()
        sp = _lib.stream_ptr()
        rc = lib.dig_scale_suffstats(self._args[0], self._args[1], self.N, self.C, _lib.dev_ptr(part[0]), self._ws, self.wsb, sp)
        _lib.check("dig_scale_suffstats", rc)
        from . import parallel
        world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        parts = part
        if parallel.collectives_on(group):
            if getattr(self, "_parts", None) is None or self._parts.shape[0] != world:
                self._parts = torch.empty((world, 3, self.C), dtype=torch.float64, device=part.device)
            dist.all_gather_into_tensor(self._parts, part, group=group)
            parts = self._parts
        rc = lib.dig_scale_factors(_lib.dev_ptr(parts), world, self.C, _lib.dev_ptr(cj), _lib.dev_ptr(cj_indel), sp)
        _lib.check("dig_scale_factors", rc)


_DIG_SRC = {"float32": _lib.DIG_F32, "float64": _lib.DIG_F64, "int16": _lib.DIG_I16}         # by numpy's and torch's dtype name
_DIG_DST = {"f32": _lib.DIG_F32, "bf16": _lib.DIG_BF16}


def gather_bins(x_data, bin_rows, tracks=None, out_dtype="f32", transpose=False, device=0):
    """x_data[bin_rows, :, tracks] as float32 (or bf16) -- mut_dataset.py:76-81 for a batch.
    transpose=True returns channels-first [B, T_sel, L] (cnn_predictors.py:131)."""
    be = backend_of(x_data, device=device)
    x = be.arr(x_data)
    src = str(x.dtype).rpartition(".")[2]                                 # "float32" of numpy's float32 and of torch.float32
    assert src in _DIG_SRC and x.ndim == 3
    N, L, T = x.shape
    rows = be.arr(bin_rows, "i64", (-1,))
    tr = be.arr(tracks, "i32", (-1,))                                     # NULL = all tracks (contiguous block copy)
    B, Ts = rows.shape[0], T if tr is None else tr.shape[0]
    if out_dtype != "f32" and not be.is_device:
        raise ValueError("host path returns float32 only")
    dst = "f32" if out_dtype == "f32" else "bf16"
    out = be.empty((B, Ts, L) if transpose else (B, L, Ts), dst)
    be.call("dig_gather_bins", be.ptr(x), _DIG_SRC[src], N, L, T, be.ptr(rows), B, be.ptr(tr), Ts, be.ptr(out), _DIG_DST[dst],
            int(transpose))
    return out


def count_contexts(genome, chroms, starts, ends, minus=None, device=0, on_device=True, form="2bit", n_up=1, n_down=1):
    """Context counts of regions of a PackedGenome (sequence_tools.py:65-99,527-566): [R, 64] trinucleotide counts for
    (n_up, n_down) = (1, 1), [R, 1024] penta-nucleotide counts for (2, 2) (dig_count_contexts5; columns in
    mk_context_sequences(2, 2) order; a START of 1 raises ValueError, the reference's fetch would start at -1).
    on_device=True keeps the genome resident in HBM (uploaded on first use) and returns a device tensor; False goes
    through the host twin (uploads the genome for this call; small genomes / tests).
    form (trinucleotides only): "2bit" (dig_count_contexts2: the genome at 2 bits per base + the list of non-ACGT runs;
    what everything uses) or "4bit" (dig_count_contexts, the first form; kept as a cross-check) -- the same counts."""
    if (n_up, n_down) not in ((1, 1), (2, 2)):
        raise NotImplementedError("context counting handles (n_up, n_down) = (1, 1) (trinucleotides) and (2, 2) "
                                  "(penta-nucleotides); got (%s, %s)" % (n_up, n_down))
    penta = (n_up, n_down) == (2, 2)
    ci = genome.chrom_index(chroms)
    R = len(ci)
    st, en = _lib.as_host(starts, np.int64).ravel(), _lib.as_host(ends, np.int64).ravel()
    mi = np.zeros(R, np.uint8) if minus is None else _lib.as_host(np.asarray(minus).astype(np.uint8), np.uint8).ravel()
    assert len(st) == len(en) == len(mi) == R and form in ("2bit", "4bit")
    if (st < 0).any() or (en < 0).any():
        raise ValueError("negative region coordinates")
    if penta:
        if form != "2bit":
            raise ValueError("penta-nucleotide counts come from the 2-bit form only")
        if ((st > 0) & (st < n_up)).any():
            bad = int(np.flatnonzero((st > 0) & (st < n_up))[0])
            raise ValueError("START %d of region %d: the reference fetches from START - %d, before the chromosome start"
                             % (st[bad], bad, n_up))
    be = backend_on(device, on_device)
    p = be.ptr
    out = be.empty((R, 1024 if penta else 64), "i32")
    regions = [be.arr(a) for a in (ci, st, en, mi)]
    if form == "2bit":
        name, head = "dig_count_contexts5" if penta else "dig_count_contexts2", genome.genome2_args(be.dev)
    else:
        words, off, ln = genome.on_device(be.dev) if be.is_device else (genome.words, genome.offsets, genome.lengths)
        name, head = "dig_count_contexts", [p(words), words.shape[0], p(off), p(ln), len(genome.names)]
    be.call(name, *head, *[p(a) for a in regions], R, p(out))
    return out


def element_context_counts(genome, elt_chrom, elt_minus, blk_ptr, blk_start, blk_end, device=0, on_device=None):
    """Strand-aware trinucleotide counts of bed12 elements straight from a PackedGenome (dig_element_context_counts): i32 [E, 64],
    row e = the sum over the blocks blk_ptr[e] .. blk_ptr[e + 1] - 1 of the count_contexts row of (elt_chrom[e], blk_start, blk_end,
    elt_minus[e]) -- the L of quickDriver's elements (onthefly_tools.py: one count_contexts row per block, summed on the host).
    elt_chrom: chromosome labels, resolved against the genome as count_contexts resolves them (a CUDA tensor: the genome's i32
    chromosome indices); elt_minus: non-zero for a '-' element.  Host arrays go through the `_host` twin (no torch) and give a
    numpy array, CUDA tensors go to the device entry point on torch's current stream and give a tensor; on_device=True / False
    places host arrays on `device` (the genome stays resident in HBM) / copies tensors back first.  What the library would refuse
    -- a blk_ptr that does not run from 0 to the block count without decreasing, a chromosome outside the genome, negative
    coordinates, 2^31 elements or blocks -- is a ValueError here, before any device work."""
    tensors = [x for x in (elt_chrom, elt_minus, blk_ptr, blk_start, blk_end) if is_cuda(x)]
    if on_device is None:
        on_device = bool(tensors)
    be = device_backend(tensors[0].device) if on_device and tensors else backend_on(device, on_device)
    if is_cuda(elt_chrom):
        ci = be.arr(elt_chrom, "i32", (-1,)) if be.is_device else _lib.as_host(elt_chrom.cpu().numpy(), np.int32).ravel()
    else:
        try:
            ci = be.arr(genome.chrom_index(list(np.asarray(elt_chrom).ravel())), "i32")
        except KeyError as exc:
            raise ValueError("element_context_counts: %s" % exc.args[0]) from exc
    host = lambda x: x.cpu().numpy() if is_cuda(x) else np.asarray(x)
    place = lambda x, dt: be.arr(x if be.is_device else host(x), dt, (-1,))
    mi = place(elt_minus if is_cuda(elt_minus) else np.asarray(elt_minus).astype(np.uint8), "u8")
    ptr, bs, en = place(blk_ptr, "i64"), place(blk_start, "i64"), place(blk_end, "i64")
    E, n_blocks = int(ci.shape[0]), int(bs.shape[0])
    if not (mi.shape[0] == E and ptr.shape[0] == E + 1 and en.shape[0] == n_blocks):
        raise ValueError("element_context_counts: elt_chrom, elt_minus [E], blk_ptr [E + 1] and blk_start, blk_end [blk_ptr[E]] disagree")
    if E >= 2 ** 31 or n_blocks >= 2 ** 31:
        raise ValueError("element_context_counts: %d elements, %d blocks: both must stay below 2^31" % (E, n_blocks))
    true = lambda x: bool(x.all())                                    # (numpy and torch alike)
    if not (int(ptr[0]) == 0 and int(ptr[E]) == n_blocks and true(ptr[1:] >= ptr[:-1])):
        raise ValueError("element_context_counts: blk_ptr must run from 0 to the block count without decreasing")
    if E and not true((ci >= 0) & (ci < len(genome.names))):
        raise ValueError("element_context_counts: element chromosome index outside [0, %d)" % len(genome.names))
    if n_blocks and not true((bs >= 0) & (en >= 0)):
        raise ValueError("element_context_counts: negative block coordinates")
    out = be.empty((E, 64), "i32")
    if E == 0:
        return out
    n_ws = int(_lib.load().dig_element_context_counts_workspace(n_blocks)) if be.is_device else 0
    p = be.ptr
    be.call("dig_element_context_counts", *genome.genome2_args(be.dev), p(ci), p(mi), p(ptr), p(bs), p(en), E, n_blocks, p(out),
            workspace=(be.empty(n_ws, "u8") if be.is_device else None, n_ws))
    return out


MC_KEPT, MC_MISMATCH, MC_DROPPED, MC_HOST = 0, 1, 2, 3          # include/dig_hip.h DIG_MC_*
_REF_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def mutation_contexts(genome, chroms, starts, refs, n_up=2, n_down=2, collapse=False, device=0, on_device=True):
    """Per-row match test, run rule and context window of mutation_contexts_by_chrom (sequence_tools.py:130-177) over a
    PackedGenome, rows in group order (dig_mutation_contexts).  refs: the REF values (anything but one upper-case ACGT letter
    never matches).  Returns (status u8 [R] -- MC_KEPT / MC_MISMATCH / MC_DROPPED / MC_HOST --, context [R]: the window at 2 bits
    per base, base k in bits 2 k, 2 k + 1; int32 bits on the device, uint32 on the host).  on_device=True keeps the genome
    resident in HBM and returns device tensors; False goes through the host twin.  A START outside its chromosome raises
    ValueError (the reference indexes past the end of the chromosome string)."""
    import pandas as pd
    codes, uniq = pd.factorize(np.asarray(chroms))                # (one lookup per distinct label)
    ci = genome.chrom_index(list(uniq))[codes] if len(codes) else np.zeros(0, np.int32)
    R = len(ci)
    st = _lib.as_host(starts, np.int64).ravel()
    if isinstance(refs, np.ndarray) and refs.dtype == np.uint8:   # codes already (0-3, a single other letter as its byte, 255)
        rc = _lib.as_host(refs, np.uint8).copy().ravel()
    else:
        one = pd.Series(np.asarray(refs, dtype=object))
        one = one.where(one.map(lambda r: isinstance(r, str) and len(r) == 1 and 4 < ord(r) < 255), "")
        rc = one.map(_REF_CODE).fillna(one.map(lambda r: ord(r) if r else 255)).to_numpy(np.uint8)
    # a REF of one letter other than ACGT matches where the genome holds that letter (an N, an IUPAC code): the match is
    # decided here from the letter table (the 2-bit form does not know it) and passed on as code 4
    other = np.flatnonzero((rc > 3) & (rc < 255))
    for k in other:
        hit = 0 <= st[k] < genome.lengths[ci[k]] and genome.letters(ci[k], st[k], st[k] + 1) == bytes([rc[k]])
        rc[k] = 4 if hit else 255
    assert len(st) == len(rc) == R
    n_up, n_down = int(n_up), int(n_down)
    if n_up < 0 or n_down < 0 or n_up + n_down + 1 > 16:
        raise ValueError("n_up, n_down >= 0 and n_up + n_down + 1 <= 16 (a context of at most 16 bases)")
    if R and ((st < 0).any() or (st >= genome.lengths[ci]).any()):
        bad = int(np.flatnonzero((st < 0) | (st >= genome.lengths[ci]))[0])
        raise ValueError("START %d is outside chromosome %s (length %d)" % (st[bad], genome.names[ci[bad]], genome.lengths[ci[bad]]))
    be = backend_on(device, on_device)
    p = be.ptr
    status, context = be.empty(R, "u8"), be.empty(R, "i32" if be.is_device else "u32")
    n_ws = max(int(_lib.load().dig_mutation_contexts_workspace(R)), 1) if be.is_device else 0
    rows = [be.arr(a) for a in (ci, st, rc)]
    be.call("dig_mutation_contexts", *genome.genome2_args(be.dev), *[p(a) for a in rows], R, n_up, n_down, int(bool(collapse)),
            p(status), p(context), workspace=(be.empty(n_ws, "u8") if be.is_device else None, n_ws))
    return status, context


MF_KIND_SNV, MF_KIND_INS, MF_KIND_OTHER = 0, 1, 2               # include/dig_hip.h DIG_MF_*
MF_SYN, MF_MIS, MF_NONS, MF_STOP_LOSS, MF_SPLICE, MF_NONE = 0, 1, 2, 3, 4, 255
MF_OK, MF_WRONG_REF, MF_HOST, MF_OUTSIDE = 0, 1, 2, 3


def gene_table(be, genome, genes, gene_chrom):
    """The gene-table arguments of dig_mutation_function / dig_gene_site_counts on backend `be`: checks the GeneSet against the
    genome (ValueError) and returns (the eight arrays gene_chrom i32, minus u8, blk_ptr, blk_start, blk_end, cds_off, spl_ptr,
    spl_pos i64 in the library's order, gene_chrom as a host array)."""
    G = len(genes)
    gch = _lib.as_host(gene_chrom, np.int32).ravel()
    assert len(gch) == G
    if G and ((gch < 0).any() or (gch >= len(genome.names)).any()):
        raise ValueError("gene chromosome index outside the genome")
    last = genes.blk_end[genes.blk_ptr[1:] - 1] if G else np.zeros(0, np.int64)
    if G and ((genes.blk_start < 1).any() or (last > genome.lengths[gch]).any()):
        raise ValueError("a gene's CDS blocks reach outside its chromosome")
    if G and (genes.cds_len % 3).any():
        raise ValueError("a gene's CDS length is not a multiple of 3")
    table = (gch, genes.minus, genes.blk_ptr, genes.blk_start, genes.blk_end, genes.cds_off, genes.spl_ptr, genes.spl_pos)
    return [be.arr(a, dt) for a, dt in zip(table, ("i32", "u8", "i64", "i64", "i64", "i64", "i64", "i64"))], gch


def mutation_function(genome, genes, gene_chrom, pair_gene, pair_start, pair_end, pair_kind, pair_ref, pair_alt, device=0,
                      on_device=True):
    """Genic function of (mutation, gene) pairs (scripts/mutationFunction.R; dig_mutation_function) over a PackedGenome.
    genes: a gene_annotation.GeneSet; gene_chrom: the genome's chromosome index of every gene (GeneSet.on_genome).  Pairs: gene
    index, 1-based closed start / end, kind (MF_KIND_*), REF / ALT codes 0-3 on the + strand (SNVs; ignored otherwise).
    Returns (impact u8, status u8, n_cds i32, cds_min i32, cds_max i32): MF_SYN ... MF_SPLICE / MF_NONE and MF_OK / MF_WRONG_REF /
    MF_HOST / MF_OUTSIDE as include/dig_hip.h describes them.  on_device=True takes numpy arrays or tensors, keeps the genome
    resident in HBM and returns device tensors; False goes through the host twin on numpy arrays."""
    be = backend_on(device, on_device)
    G = len(genes)
    tab, _ = gene_table(be, genome, genes, gene_chrom)
    pairs = [be.arr(a, dt, (-1,)) for a, dt in zip((pair_gene, pair_start, pair_end, pair_kind, pair_ref, pair_alt),
                                                   ("i32", "i64", "i64", "u8", "u8", "u8"))]
    n = pairs[0].shape[0]
    assert all(a.shape[0] == n for a in pairs)
    # (device tensors are checked here; the host twin checks its own arrays inside the library)
    if be.is_device and n and (int(pairs[0].min()) < 0 or int(pairs[0].max()) >= G):
        raise ValueError("pair gene index outside the gene table")
    outs = [be.empty(n, dt) for dt in ("u8", "u8", "i32", "i32", "i32")]           # impact, status, n_cds, cds_min, cds_max
    p = be.ptr
    be.call("dig_mutation_function", *genome.genome2_args(be.dev), *[p(a) for a in tab], G, *[p(a) for a in pairs], n,
            *[p(a) for a in outs])
    return tuple(outs)


GS_OK, GS_HOST = 0, 1                                            # include/dig_hip.h DIG_GS_*
_GS_CODE = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"      # codon 16 b0 + 4 b1 + b2, A C G T = 0 .. 3
_GS_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _gene_sites_from_letters(genome, genes, gene_chrom, g):
    """(L [4, 192], n_stop_loss) of one gene the kernel left to the host (DIG_GS_HOST), from PackedGenome's letters: a site whose
    trinucleotide holds a letter other than ACGT (or is cut off by the chromosome end) is skipped, as seq_to_context returning
    nothing skips it in si_by_regions (sequence_tools.py:416-417); a codon with such a letter translates to X, as for
    addMutationFunction."""
    ci, minus = int(gene_chrom[g]), bool(genes.minus[g])
    clen = int(genome.lengths[ci])
    b0, b1 = int(genes.blk_ptr[g]), int(genes.blk_ptr[g + 1])
    pos = np.concatenate([np.arange(s, e + 1) for s, e in zip(genes.blk_start[b0:b1], genes.blk_end[b0:b1])] or [np.zeros(0, np.int64)])
    if minus:
        pos = pos[::-1]
    spl = genes.spl_pos[genes.spl_ptr[g]:genes.spl_ptr[g + 1]]
    L, n_stop_loss = np.zeros((4, 192), np.int32), 0
    code = {c: i for i, c in enumerate(b"ACGT")}

    def context(p):                                                  # (X, Y, Z) in transcript direction, or None
        if p - 1 < 1 or p + 1 > clen:
            return None
        w = genome.letters(ci, p - 2, p + 1)
        w = w[::-1].translate(_GS_COMP) if minus else w
        return tuple(code[c] for c in w) if all(c in code for c in w) else None

    def amino(codon):
        return _GS_CODE[16 * codon[0] + 4 * codon[1] + codon[2]] if None not in codon else 'X'

    for k in range(len(pos) // 3):
        letters = [genome.letters(ci, int(p) - 1, int(p)) for p in pos[3 * k:3 * k + 3]]
        codon = [code.get((c.translate(_GS_COMP) if minus else c)[0]) for c in letters]
        for at in range(3):
            ctx = context(int(pos[3 * k + at]))
            if ctx is None:
                continue
            for a in range(4):
                if a == ctx[1]:
                    continue
                changed = codon[:at] + [a] + codon[at + 1:]
                old_aa, new_aa = amino(codon), amino(changed)
                col = 3 * (16 * ctx[0] + 4 * ctx[1] + ctx[2]) + a - (a > ctx[1])
                if new_aa == old_aa:
                    L[0, col] += 1
                elif new_aa == '*':
                    L[2, col] += 1
                elif old_aa != '*':
                    L[1, col] += 1
                else:
                    n_stop_loss += 1
    for p in spl:
        ctx = context(int(p))
        if ctx is not None:
            c0 = 3 * (16 * ctx[0] + 4 * ctx[1] + ctx[2])
            L[3, c0:c0 + 3] += 1
    return L, n_stop_loss


def gene_site_counts(genome, genes, gene_chrom, device=0, on_device=True, return_status=False):
    """The possible single-base substitutions of every gene by effect class and substitution type (dig_gene_site_counts; the L of
    the gene container) over a PackedGenome.  genes: a gene_annotation.GeneSet; gene_chrom: the genome's chromosome index of every
    gene (GeneSet.on_genome).  Returns host arrays (L i32 [G, 4, 192] -- classes silent, missense, nonsense, essential splice;
    columns in the order of the sorted substitution index --, n_stop_loss i32 [G]); the genes the kernel left to the host (a letter
    other than ACGT in their CDS, splice positions or flanks) are finished from the genome's letters.  on_device=True keeps the
    genome resident in HBM; False goes through the host twin and needs no torch.  return_status: also the kernel's status per gene
    (GS_OK / GS_HOST)."""
    be = backend_on(device, on_device)
    G = len(genes)
    tab, gch = gene_table(be, genome, genes, gene_chrom)
    outs = [be.empty((G, 4, 192), "i32"), be.empty(G, "i32"), be.empty(G, "u8")]
    p = be.ptr
    be.call("dig_gene_site_counts", *genome.genome2_args(be.dev), *[p(a) for a in tab], G, *[p(a) for a in outs])
    L, nsl, status = (a.cpu().numpy() if be.is_device else a for a in outs)
    for g in np.flatnonzero(status == GS_HOST):
        L[g], nsl[g] = _gene_sites_from_letters(genome, genes, gch, int(g))
    return (L, nsl, status) if return_status else (L, nsl)


def tiled_nb_test(pt, k, mu, sigma, device=0):
    """Per-tile exact NB test (nb_model.py:141-178).  pt f64 [n_bins, n_tiles] or [C, n_bins, n_tiles];
    k i32 [C, n_bins, n_tiles]; mu, sigma f64 [C, n_bins].  Returns (pval, exp) [C, n_bins, n_tiles]."""
    be = backend_of(k, device=device)
    k = be.arr(k, "i32")
    C, nb, nt = k.shape
    pt = be.arr(pt, "f64")
    mu, sigma = be.arr(mu, "f64", (C, nb)), be.arr(sigma, "f64", (C, nb))
    pval, ex = be.empty((C, nb, nt), "f64"), be.empty((C, nb, nt), "f64")
    p = be.ptr
    be.call("dig_tiled_nb_test", p(pt), int(pt.ndim == 3), p(k), p(mu), p(sigma), p(pval), p(ex), C, nb, nt)
    return pval, ex


# ---------------------------------------------------------------------------
# per-base / tiled route: front half (dig_base_tile_probs + dig_tile_mut_counts) and the whole chain
# ---------------------------------------------------------------------------
TILE_CTX_MAX_POSITIONS = 16384      # positions of the longest penta-nucleotide region the tile kernels evaluate (kCtxMaxPos, dig_tiles.hpp)


def check_tile_regions(starts, ends, n_up):
    """What every caller of dig_base_tile_probs_ctx with host-side coordinates must check (the device entry point sees
    device pointers only): a region that starts inside (0, n_up) would fetch from a negative position -- the reference's
    pysam fetch fails there too (sequence_tools.py:21-29)."""
    st, en = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    if st.size and n_up > 1 and int((en - st).max()) > TILE_CTX_MAX_POSITIONS:
        raise ValueError("penta-nucleotide regions may hold at most %d positions" % TILE_CTX_MAX_POSITIONS)
    if st.size and n_up > 1 and ((st > 0) & (st < n_up)).any():
        raise ValueError("a region that starts at 1 would fetch from a negative position (the reference's pysam fetch fails too)")


def _tile_genome(be, genome, chroms, starts, ends, s_prob, binsize, n_tiles, dense=False):
    """The 14 arguments dig_base_tile_probs_ctx, dig_tile_census and dig_sparse_tile_test begin with, checked: (the pointers and sizes
    up to n_tiles in the entry points' order, the arrays behind them, C, R, n_tiles, n_up, binsize).  dense: base_tile_probs, which
    leaves binsize to the library and asserts the table's shape."""
    ci = genome.chrom_index(chroms)
    R = len(ci)
    st, en = _lib.as_host(starts, np.int64).ravel(), _lib.as_host(ends, np.int64).ravel()
    if (st < 0).any() or (en < 0).any():
        raise ValueError("negative region coordinates")
    binsize = int(binsize)
    if binsize < 1 and not dense:
        raise ValueError("binsize >= 1")
    if n_tiles is None:
        n_tiles = int(max(1, -(-int((en - st).max() if R else 1) // binsize)))
    s_prob = be.arr(s_prob, "f64")
    if s_prob.ndim != 2 or s_prob.shape[1] not in (64, 1024):
        raise (AssertionError if dense else ValueError)("s_prob must be [C, 64] (trinucleotide) or [C, 1024] (penta-nucleotide)")
    C = s_prob.shape[0]
    n_up = 1 if s_prob.shape[1] == 64 else 2
    check_tile_regions(st, en, n_up)
    words, off, ln = genome.on_device(be.dev) if be.is_device else (genome.words, genome.offsets, genome.lengths)
    held = [words, off, ln] + [be.arr(a) for a in (ci, st, en)] + [s_prob]
    p = be.ptr
    args = [p(words), words.shape[0], p(off), p(ln), len(genome.names), p(held[3]), p(held[4]), p(held[5]), R, p(s_prob), C, n_up, binsize,
            int(n_tiles)]
    return args, held, C, R, int(n_tiles), n_up, binsize


def base_tile_probs(genome, chroms, starts, ends, s_prob, binsize, n_tiles=None, device=0, on_device=True):
    """Tile probabilities of regions of a PackedGenome for C cohorts at once (sequence_tools.py:292-317 + the tiling of
    nb_model.py:126-186).  s_prob: f64 [C, 64] (trinucleotide contexts, index 16 b0 + 4 b1 + b2) or [C, 1024]
    (penta-nucleotide: the reference's default n_up = n_down = 2; index in itertools.product('ACGT', repeat=5) order).
    Returns (pt [C, R, n_tiles], first_pos [R], n_valid [R]); n_tiles defaults to what the longest region needs.
    on_device=True keeps the genome resident in HBM and returns device tensors; False goes through the host twin and returns
    arrays."""
    be = backend_on(device, on_device)
    args, held, C, R, n_tiles, _, _ = _tile_genome(be, genome, chroms, starts, ends, s_prob, binsize, n_tiles, dense=True)
    pt, first, nval = be.empty((C, R, n_tiles), "f64"), be.empty(R, "i64"), be.empty(R, "i32")
    p = be.ptr
    be.call("dig_base_tile_probs_ctx", *args, p(pt), p(first), p(nval))
    return pt, first, nval


def tile_mut_counts(genome, chroms, starts, ends, first_pos, n_valid, mut_chrom, mut_start, mut_end, mut_cohort, C, binsize,
                    n_tiles):
    """k i32 [C, R, n_tiles]: mutation rows per tile and cohort (nb_model.py:133-136,160-163).  Regions and mutations
    are joined with the interval-join kernels (a tabix fetch returns the rows overlapping the region); a row counts in
    the tile that holds its START.  first_pos, n_valid as base_tile_probs returns them: device tensors -> a device tensor, arrays
    -> the host twins.  mut_*: device tensors or host arrays (chromosome labels as in `chroms`)."""
    be = backend_of(first_pos, n_valid)
    first_pos, n_valid, pm, pr, ms, co = _tile_rows(be, genome, chroms, starts, ends, first_pos, n_valid, mut_chrom, mut_start, mut_end,
                                                    mut_cohort)
    R = first_pos.shape[0]
    k = be.empty((int(C), R, int(n_tiles)), "i32")
    p = be.ptr
    be.call("dig_tile_mut_counts", p(pm), p(pr), pm.shape[0], p(ms), *([] if be.is_device else [ms.shape[0]]), p(co), p(first_pos),
            p(n_valid), int(binsize), int(n_tiles), R, int(C), p(k))
    return k


def _tile_rows(be, genome, chroms, starts, ends, first_pos, n_valid, mut_chrom, mut_start, mut_end, mut_cohort, R=-1,
               what="mut_cohort"):
    """What the three row-counting routes hand their entry points, checked: (first_pos i64 [R], n_valid i32 [R], pair_mut, pair_reg,
    mut_start, mut_cohort i32 -- one entry per mutation row, or ValueError in the name of `what`)."""
    first_pos, n_valid = be.arr(first_pos, "i64", (R,)), be.arr(n_valid, "i32", (R,))
    pm, pr, ms = _tile_pairs(be, genome, chroms, starts, ends, mut_chrom, mut_start, mut_end)
    co = be.arr(mut_cohort, "i32", (-1,))
    if ms.shape[0] != co.shape[0]:
        raise ValueError(what + ": one entry per mutation row")
    return first_pos, n_valid, pm, pr, ms, co


def _tile_pairs(be, genome, chroms, starts, ends, mut_chrom, mut_start, mut_end):
    """The interval join of the per-base route: (pair_mut, pair_reg) i32, one entry per (mutation row, region) that overlap, and the
    rows' START as the counting entry points read it."""
    order, start_key, runmax_key, blk_end = join_blocks(genome.chrom_index(chroms), _lib.as_host(starts, np.int64),
                                                        _lib.as_host(ends, np.int64))
    mc = be.arr(mut_chrom if is_cuda(mut_chrom) else genome.chrom_index(list(np.asarray(mut_chrom).astype(str))), "i64")
    ms, me = be.arr(mut_start, "i64"), be.arr(mut_end, "i64")
    pm, pb = overlap_join(be, start_key, runmax_key, blk_end, mc, ms, me)
    pr = be.arr(order, "i32")[pb.long() if be.is_device else pb]      # block of the sorted table -> region
    return pm, pr, ms


def tile_sample_counts(genome, chroms, starts, ends, first_pos, n_valid, mut_chrom, mut_start, mut_end, mut_cohort, mut_sample,
                       sample_offsets, keep, cap, C, binsize, n_tiles, return_keys=False):
    """(k_cap, k_samples) i32 [C, R, n_tiles]: tile_mut_counts by sample -- with n the rows of one sample that tile_mut_counts counts
    in a tile, k_cap = the sum over the kept samples of min(n, cap) and k_samples = the kept samples with n > 0: the same join,
    dig_tile_sample_keys, a key sort, dig_tile_sample_counts.  mut_sample i32: the row's GLOBAL sample, inside its cohort's range of
    sample_offsets [C + 1] (a cohort's first global sample; equal labels in two cohorts are two samples); keep u8 per global sample
    or None: a sample with keep == 0 counts nowhere; cap: an integer >= 1, or None for no cap.  Everything else, and the choice of
    the backend, as tile_mut_counts.  ValueError for a row whose sample is outside its cohort and for a key (cohort, region, tile,
    sample) that does not fit 63 bits.  return_keys: (k_cap, k_samples, keys) -- the sorted keys of dig_tile_sample_keys, i64, one
    per pair of the join, for tile_window_sample_keys: the join and the key kernel then run once."""
    be = backend_of(first_pos, n_valid)
    C, T = int(C), int(n_tiles)
    off_host, _, S = _sample_offsets(sample_offsets, C)
    if cap is not None and (int(cap) != cap or cap < 1):
        raise ValueError("cap: an integer >= 1 (None: no cap)")
    co, sa = be.arr(mut_cohort, "i32", (-1,)), be.arr(mut_sample, "i32", (-1,))
    keep = be.arr(keep, "u8", (-1,))
    if keep is not None and keep.shape[0] != S:
        raise ValueError("keep: one byte per global sample ({})".format(S))
    if sa.shape[0] != co.shape[0]:
        raise ValueError("mut_sample: one entry per mutation row")
    if co.shape[0]:
        # (a row of a cohort outside [0, C) counts nowhere, as in tile_mut_counts; every other row must name a sample of its cohort)
        off, c = be.arr(off_host, "i64"), be.arr(co.clip(0, C - 1), "i64")
        if bool(((co >= 0) & (co < C) & ((sa < off[c]) | (sa >= off[c + 1]))).any()):
            raise ValueError("a row outside the tables: global sample within its cohort's range of sample_offsets")
    first_pos, n_valid, pm, pr, ms, co = _tile_rows(be, genome, chroms, starts, ends, first_pos, n_valid, mut_chrom, mut_start, mut_end, co,
                                                    what="mut_cohort, mut_sample")
    p = be.ptr
    n, R = pm.shape[0], first_pos.shape[0]
    keys = be.empty(n, "i64")
    k_cap, k_samples = be.empty((C, R, T), "i32"), be.empty((C, R, T), "i32")
    with _requirements_as_value_errors():
        be.call("dig_tile_sample_keys", p(pm), p(pr), n, p(ms), ms.shape[0], p(co), p(sa), p(keep), p(first_pos), p(n_valid),
                int(binsize), T, R, C, S, p(keys))
        keys = _sorted(be, keys)
        be.call("dig_tile_sample_counts", p(keys), n, C, R, T, S, 0 if cap is None else int(cap), p(k_cap), p(k_samples))
    return (k_cap, k_samples, keys) if return_keys else (k_cap, k_samples)


def tiled_nb_model(genome, chroms, starts, ends, s_prob, mu, sigma, mut_chrom, mut_start, mut_end, mut_cohort, binsize=50,
                   device=0, on_device=True, mut_sample=None, sample_offsets=None, keep=None, cap=None, by_sample=False):
    """nb_model (nb_model.py:188-234) for C cohorts x R regions in three launches + the interval join:
    base_tile_probs -> tile_mut_counts -> tiled_nb_test.  mu, sigma: [C, R].  Returns a dict of device tensors (arrays with
    on_device=False) pval, exp, pt [C, R, n_tiles], k i32 [C, R, n_tiles], first_pos [R], n_valid [R].
    mut_sample (with sample_offsets; keep, cap as tile_sample_counts takes them): the counts by sample -- k is then k_cap, and with
    by_sample the dict also holds k_samples and pval_sample, the same test on k_samples."""
    pt, first, nval = base_tile_probs(genome, chroms, starts, ends, s_prob, binsize, device=device, on_device=on_device)
    C, R, n_tiles = pt.shape
    rows = (genome, chroms, starts, ends, first, nval, mut_chrom, mut_start, mut_end, mut_cohort)
    if mut_sample is None:
        if sample_offsets is not None or keep is not None or cap is not None or by_sample:
            raise ValueError("sample_offsets, keep, cap and by_sample need mut_sample")
        k = tile_mut_counts(*rows, C, binsize, n_tiles)
    else:
        k, k_samples = tile_sample_counts(*rows, mut_sample, sample_offsets, keep, cap, C, binsize, n_tiles)
    pval, ex = tiled_nb_test(pt, k, mu, sigma, device=device)
    res = dict(pval=pval, exp=ex, pt=pt, k=k, first_pos=first, n_valid=nval)
    if by_sample:
        res["k_samples"], res["pval_sample"] = k_samples, tiled_nb_test(pt, k_samples, mu, sigma, device=device)[0]
    return res


TILE_WINDOW_MAX_WIDTH = 2048        # DIG_TILE_WINDOW_MAX_WIDTH (include/dig_hip.h)


def tile_window_test(pt, k, mu, sigma, n_valid, width, device=0, out=None):
    """The NB test of every window of `width` consecutive tiles (dig_tile_window_test): pt f64, k i32 [C, R, T] and n_valid i32 [R] as
    base_tile_probs and tile_mut_counts / tile_sample_counts leave them, mu, sigma f64 [C, R].  Returns dict(pt, exp, pval f64, k i32
    [C, R, T]; n_windows i32 [R]): window t of region r covers the tiles t .. min(t + width, n_valid[r]) - 1; n_windows[r] is
    max(n_valid[r] - width + 1, 1), or 0 for a region without tiles; pt is the window's sum added left to right, k the integer sum,
    pval and exp the test of tiled_nb_test on them (the same bits); behind the last window pt, exp, pval are NaN and k is 0.
    Device tensors in -> device tensors out; arrays go through the host twin.  out: a dict a former call returned, for the same
    shapes: its planes are written again (nb_model_window_hits keeps one set for all its widths).  ValueError for what the library
    refuses: a width outside [1, TILE_WINDOW_MAX_WIDTH], C R or T at or above 2^31."""
    if isinstance(width, bool) or int(width) != width:
        raise ValueError("width: an integer >= 1")
    width = int(width)
    be = backend_of(pt, k, n_valid, device=device)
    pt, k = be.arr(pt, "f64"), be.arr(k, "i32")
    if pt.ndim != 3 or tuple(k.shape) != tuple(pt.shape):
        raise ValueError("pt and k must be [C, R, T]")
    C, R, T = (int(s) for s in pt.shape)
    mu, sigma, n_valid = be.arr(mu, "f64", (C, R)), be.arr(sigma, "f64", (C, R)), be.arr(n_valid, "i32", (R,))
    if out is None:
        out = dict(pt=be.empty((C, R, T), "f64"), k=be.empty((C, R, T), "i32"), exp=be.empty((C, R, T), "f64"),
                   pval=be.empty((C, R, T), "f64"), n_windows=be.empty(R, "i32"))
    p = be.ptr
    with _requirements_as_value_errors():
        be.call("dig_tile_window_test", p(pt), p(k), p(mu), p(sigma), p(n_valid), C, R, T, width, p(out["pt"]), p(out["k"]), p(out["exp"]),
                p(out["pval"]), p(out["n_windows"]))
    if C * R * T == 0 and R:
        # (nothing was launched: the region table from n_valid alone)
        nv = n_valid.clip(0, T)
        out["n_windows"][:] = (nv > 0) * (nv - width + 1).clip(1)
    return out


def tile_window_sample_keys(keys, C, R, T, n_samples, device=0):
    """The keys of tile_sample_counts(return_keys=True), ((row T + tile) << sb) | sample, re-keyed sample-major (((row << sb) | sample)
    T + tile: dig_tile_window_sample_keys) and sorted ascending: what tile_window_samples takes, once for every width.  i64 [n]; a
    device tensor in -> a device tensor out, an array goes through the host twin.  ValueError for what the library refuses."""
    be = backend_of(keys, device=device)
    keys = be.arr(keys, "i64", (-1,))
    out = be.empty(keys.shape[0], "i64")
    p = be.ptr
    with _requirements_as_value_errors():
        be.call("dig_tile_window_sample_keys", p(keys), keys.shape[0], int(C), int(R), int(T), int(n_samples), p(out))
    return _sorted(be, out)


def tile_window_samples(keys_sm, n_valid, C, R, T, n_samples, width, device=0, out=None):
    """s_w i32 [C, R, T]: the distinct kept samples with a counted row in window t of `width` consecutive tiles
    (dig_tile_window_samples), 0 behind the last window; the windows are those of tile_window_test.  keys_sm: what
    tile_window_sample_keys returns; n_valid i32 [R] as base_tile_probs leaves it.  Device tensors in -> a device tensor out; arrays go
    through the host twin.  out: a plane a former call returned, for the same shape: it is written again.  ValueError for what the
    library refuses: a width outside [1, TILE_WINDOW_MAX_WIDTH], C R, T or the key count at or above 2^31, a key that does not fit."""
    if isinstance(width, bool) or int(width) != width:
        raise ValueError("width: an integer >= 1")
    C, R, T = int(C), int(R), int(T)
    be = backend_of(keys_sm, n_valid, device=device)
    keys_sm, n_valid = be.arr(keys_sm, "i64", (-1,)), be.arr(n_valid, "i32", (R,))
    if out is None:
        out = be.empty((C, R, T), "i32")
    elif tuple(out.shape) != (C, R, T):
        raise ValueError("out must be [C, R, T]")
    p = be.ptr
    with _requirements_as_value_errors():
        be.call("dig_tile_window_samples", p(keys_sm), keys_sm.shape[0], p(n_valid), C, R, T, int(n_samples), int(width), p(out))
    return out


# ---------------------------------------------------------------------------
# per-base route for the mutated tiles only (dig_tilesparse.hip): nothing here is [C, R, T]
# ---------------------------------------------------------------------------
def tile_census(genome, chroms, starts, ends, s_prob, binsize, n_tiles=None, device=0, on_device=True):
    """What the sparse per-base scan knows of the regions without a [C, R, T] plane (dig_tile_census): first_pos i64 [R], n_valid i32
    [R] -- the bits base_tile_probs returns --, denom f64 [C, R], the region's sum of s_prob over its positions (what the dense route
    divides by), and n_positive i32 [C, R], the tiles below n_valid whose dense pt is > 0.  Arguments as base_tile_probs; returns
    (first_pos, n_valid, denom, n_positive), device tensors or (on_device=False, the host twin) arrays."""
    be = backend_on(device, on_device)
    args, held, C, R, _, n_up, _ = _tile_genome(be, genome, chroms, starts, ends, s_prob, binsize, n_tiles)
    first, nval = be.empty(R, "i64"), be.empty(R, "i32")
    denom, npos = be.empty((C, R), "f64"), be.empty((C, R), "i32")
    wsb = int(_lib.load().dig_tile_census_workspace(C, n_up))
    p = be.ptr
    with _requirements_as_value_errors():
        be.call("dig_tile_census", *args, p(first), p(nval), p(denom), p(npos), workspace=(be.empty(wsb, "u8"), wsb) if be.is_device else None)
    return first, nval, denom, npos


def sparse_tile_test(genome, chroms, starts, ends, s_prob, binsize, n_tiles, first_pos, n_valid, denom, mu, sigma, mut_chrom, mut_start,
                     mut_end, mut_cohort):
    """The NB test of the tiles that hold a row, and of no other: the join of tile_mut_counts, dig_sparse_tile_keys, a key sort,
    dig_sparse_tile_test, and the runs' heads kept.  first_pos, n_valid, denom as tile_census returns them (device tensors -> device
    tensors, arrays -> the host twins); mu, sigma [C, R]; mut_*: as tile_mut_counts takes them.  Returns dict(cohort, region, tile, k
    i32, pt, exp, pval f64): one entry per mutated tile, cohort-major, then by region, then by tile -- the order of the dense frame.
    k is dig_tile_mut_counts' count, pt / exp / pval what the dense route has there (pt to rounding: another order of additions)."""
    be = backend_of(first_pos, n_valid, denom)
    args, held, C, R, T, _, binsize = _tile_genome(be, genome, chroms, starts, ends, s_prob, binsize, n_tiles)
    denom, mu, sigma = (be.arr(x, "f64", (C, R)) for x in (denom, mu, sigma))
    first_pos, n_valid, pm, pr, ms, co = _tile_rows(be, genome, chroms, starts, ends, first_pos, n_valid, mut_chrom, mut_start, mut_end,
                                                    mut_cohort, R)
    p = be.ptr
    n = pm.shape[0]
    keys = be.empty(n, "i64")
    names = ("cohort", "region", "tile", "k", "pt", "exp", "pval")
    with _requirements_as_value_errors():
        be.call("dig_sparse_tile_keys", p(pm), p(pr), n, p(ms), ms.shape[0], p(co), p(first_pos), p(n_valid), binsize, T, R, C, p(keys))
        keys = _sorted(be, keys)
        out = {k: be.empty(n, "i32" if i < 4 else "f64") for i, k in enumerate(names)}
        be.call("dig_sparse_tile_test", *args, p(denom), p(mu), p(sigma), p(keys), n, *[p(out[k]) for k in names])
    head = out["k"] > 0
    return {k: v[head] for k, v in out.items()}


# ---------------------------------------------------------------------------
# sliding windows over the mutated tiles only (dig_tilesparsewindows.hip): nothing here is [C, R, T] either
# ---------------------------------------------------------------------------
SPARSE_WINDOW_CHUNK = 1 << 24       # candidate windows per call of dig_sparse_window_test: 40 bytes of outputs each


def _window_width(width):
    if isinstance(width, (bool, np.bool_)) or int(width) != width:
        raise ValueError("width: an integer >= 1")
    return int(width)


def tile_window_census(genome, chroms, starts, ends, s_prob, binsize, width, n_tiles=None, n_positive=None, device=0, on_device=True):
    """What the sparse window scan knows of the windows of `width` consecutive tiles without a [C, R, T] plane (dig_tile_window_census):
    n_windows i32 [R], the bits of tile_window_test, and n_positive_w i32 [C, R], the windows below n_windows that cover a tile whose
    dense pt is > 0 -- the windows whose dense pt is > 0.  Arguments as tile_census; n_positive: what tile_census returned for the same
    binsize and n_tiles, or None -- with it a region whose tiles are all positive, or all not, is answered without a walk (a device
    tensor there keeps the call on the device, an array sends it through the host twin).  Returns (n_windows, n_positive_w), device
    tensors or (on_device=False) arrays.  ValueError for what the library refuses: a width outside [1, TILE_WINDOW_MAX_WIDTH], C R at or
    above 2^31."""
    width = _window_width(width)
    be = backend_on(device, on_device) if n_positive is None else backend_of(n_positive, device=device)
    args, held, C, R, _, n_up, _ = _tile_genome(be, genome, chroms, starts, ends, s_prob, binsize, n_tiles)
    npos = be.arr(n_positive, "i32", (C, R))
    nwin, npw = be.empty(R, "i32"), be.empty((C, R), "i32")
    wsb = int(_lib.load().dig_tile_census_workspace(C, n_up))
    p = be.ptr
    with _requirements_as_value_errors():
        be.call("dig_tile_window_census", *args, width, p(npos), p(nwin), p(npw), workspace=(be.empty(wsb, "u8"), wsb) if be.is_device else None)
    return nwin, npw


class SparseWindows:
    """The sorted keys of one sparse scan, from which the windows of every width are served (sparse_window_test makes it)."""
    NAMES = ("cohort", "region", "window", "k", "pt", "exp", "pval")

    def __init__(self, be, args, held, C, R, T, n_valid, denom, mu, sigma, keys, chunk_windows):
        self.be, self.args, self.held, self.C, self.R, self.T = be, args, held, C, R, T
        self.n_valid, self.denom, self.mu, self.sigma, self.keys = n_valid, denom, mu, sigma, keys
        self.chunk_windows = SPARSE_WINDOW_CHUNK if chunk_windows is None else int(chunk_windows)
        if self.chunk_windows < 1 or self.chunk_windows > 2 ** 31 - 1:
            raise ValueError("chunk_windows: an integer within [1, 2^31)")

    def offsets(self, width):
        """(offsets i64 [n + 1], total): where the candidate windows of every key start in the flat list of this width (the windows
        whose first mutated tile is the key's; only a run's head has any), and how many there are -- the total may exceed 2^31."""
        be, p, n = self.be, self.be.ptr, self.keys.shape[0]
        counts = be.empty(n, "i64")
        with _requirements_as_value_errors():
            be.call("dig_sparse_window_count", p(self.keys), n, p(self.n_valid), self.C, self.R, self.T, _window_width(width), p(counts))
        excl, total = _scan(be, counts)
        return be.cat([excl, be.arr(np.array([total], np.int64))], "i64"), total

    def chunks(self, width, chunk_windows=None):
        """The mutated windows of `width` tiles, dig_sparse_window_test on at most chunk_windows candidates at a time: yields
        dict(cohort, region, window, k i32, pt, exp, pval f64), one entry per mutated window, cohort-major, then by region, then by
        window, each window once; the chunks one after the other are the whole list."""
        be, p = self.be, self.be.ptr
        width = _window_width(width)
        step = self.chunk_windows if chunk_windows is None else int(chunk_windows)
        if step < 1 or step > 2 ** 31 - 1:
            raise ValueError("chunk_windows: an integer within [1, 2^31)")
        offsets, total = self.offsets(width)
        for begin in range(0, total, step):
            count = min(step, total - begin)
            out = {k: be.empty(count, "i32" if i < 4 else "f64") for i, k in enumerate(self.NAMES)}
            with _requirements_as_value_errors():
                be.call("dig_sparse_window_test", *self.args, p(self.denom), p(self.mu), p(self.sigma), p(self.keys), self.keys.shape[0],
                        p(offsets), width, begin, count, *[p(out[k]) for k in self.NAMES])
            yield out

    def windows(self, width, chunk_windows=None):
        """All chunks of `width` as one dict."""
        got = list(self.chunks(width, chunk_windows))
        return {k: self.be.cat([g[k] for g in got], "i32" if i < 4 else "f64") for i, k in enumerate(self.NAMES)}


def sparse_window_test(genome, chroms, starts, ends, s_prob, binsize, n_tiles, first_pos, n_valid, denom, mu, sigma, mut_chrom, mut_start,
                       mut_end, mut_cohort, chunk_windows=None):
    """The NB test of the windows of consecutive tiles that hold a row, and of no other: the join, dig_sparse_tile_keys and the key sort
    of sparse_tile_test, once; the SparseWindows it returns then serves every width -- per width dig_sparse_window_count, a prefix sum,
    and dig_sparse_window_test in chunks of at most chunk_windows candidate windows (default SPARSE_WINDOW_CHUNK).  Arguments as
    sparse_tile_test (device tensors -> device tensors, arrays -> the host twins).  .windows(width) is dict(cohort, region, window, k
    i32, pt, exp, pval f64): one entry per mutated window, in the order of the dense window frame; width 1 is sparse_tile_test bit for
    bit (with `window` for `tile`); against tile_window_test k is exact, pt and exp agree to rounding (one division here, a sum of
    quotients there).  ValueError for what the library refuses."""
    be = backend_of(first_pos, n_valid, denom)
    args, held, C, R, T, _, binsize = _tile_genome(be, genome, chroms, starts, ends, s_prob, binsize, n_tiles)
    denom, mu, sigma = (be.arr(x, "f64", (C, R)) for x in (denom, mu, sigma))
    first_pos, n_valid, pm, pr, ms, co = _tile_rows(be, genome, chroms, starts, ends, first_pos, n_valid, mut_chrom, mut_start, mut_end,
                                                    mut_cohort, R)
    p = be.ptr
    n = pm.shape[0]
    keys = be.empty(n, "i64")
    with _requirements_as_value_errors():
        be.call("dig_sparse_tile_keys", p(pm), p(pr), n, p(ms), ms.shape[0], p(co), p(first_pos), p(n_valid), binsize, T, R, C, p(keys))
        keys = _sorted(be, keys)
    return SparseWindows(be, args, held, C, R, T, n_valid, denom, mu, sigma, keys, chunk_windows)


def _tile_counts(be, score, n_valid, cut):
    """dig_tile_select_count on the backend's arrays: (the six leading arguments both entry points take, counts i32 [C R], C, R, T)."""
    score = be.arr(score, "f64")
    assert score.ndim == 3, "score must be [C, R, T]"
    C, R, T = (int(s) for s in score.shape)
    n_valid, cut = be.arr(n_valid, "i32", (R,)), _per_cohort(be, cut, C)
    plane = [score, n_valid, cut, C, R, T]
    counts = be.empty(C * R, "i32")
    with _requirements_as_value_errors():
        be.call("dig_tile_select_count", *[be.ptr(x) for x in plane[:3]], C, R, T, be.ptr(counts))
    return plane, counts, C, R, T


def tile_select_counts(score, n_valid, cut, device=0):
    """counts i32 [C, R]: the hits of every (cohort, region) row of a score plane -- the first call of tile_select alone."""
    be = backend_of(score, n_valid, device=device)
    _, counts, C, R, _ = _tile_counts(be, score, n_valid, cut)
    return counts.reshape(C, R)


def tile_select(score, n_valid, cut, pt=None, exp=None, k=None, device=0, index=True):
    """The hits of a score plane of the per-base route, in the row order of the reference's frame: dig_tile_select_count, a
    cumulative sum, dig_tile_select_fill.  score f64 [C, R, T]; n_valid i32 [R] as base_tile_probs returns it; cut f64 [C] (a
    single value stands for every cohort).  Tile (c, r, t) is a hit when t < n_valid[r] and score[c, r, t] <= cut[c]; a NaN on
    either side never hits, cut = +inf takes every existing tile with a non-NaN score.  pt, exp f64 and k i32 [C, R, T]: planes
    gathered at the hits when given.
    Returns dict(region i32, tile i32, score f64 [hits], cohort-major, then by region, then by tile; pt / exp / k [hits] for the
    planes given; cohort_ptr host int64 [C + 1]: where a cohort's hits start); index=False leaves region and tile out (the
    ragged score lists of a Benjamini-Hochberg pass).  ValueError, before the fill, for more than 2^31 - 1 hits.  CUDA tensors
    in -> CUDA tensors out."""
    be = backend_of(score, n_valid, pt, exp, k, device=device)
    held, counts, C, R, T = _tile_counts(be, score, n_valid, cut)        # (held: the arrays behind the pointers stay alive)
    planes = dict(pt=be.arr(pt, "f64", (C, R, T)), exp=be.arr(exp, "f64", (C, R, T)), k=be.arr(k, "i32", (C, R, T)))
    p = be.ptr
    plane = [p(x) for x in held[:3]] + [C, R, T]
    with _requirements_as_value_errors():
        offsets, total, cohort_ptr = _scan(be, counts, groups=C)
        if total > 2 ** 31 - 1:
            raise ValueError("%d hits: a smaller cut or fewer cohorts per call" % total)
        res = dict(region=be.empty(total, "i32"), tile=be.empty(total, "i32")) if index else {}
        res["score"] = be.empty(total, "f64")
        for name, x in planes.items():
            if x is not None:
                res[name] = be.empty(total, "i32" if name == "k" else "f64")
        be.call("dig_tile_select_fill", *plane, p(offsets), total, p(planes["pt"]), p(planes["exp"]), p(planes["k"]),
                p(res.get("region")), p(res.get("tile")), p(res["score"]), p(res.get("pt")), p(res.get("exp")), p(res.get("k")))
    res["cohort_ptr"] = cohort_ptr
    return res


def row_select_chunk():
    """The elements of a chunk of dig_row_select_* (a wave's share of a row): dig_row_select_chunk."""
    return int(_lib.load().dig_row_select_chunk())


def _row_counts(be, score, cut):
    """dig_row_select_count on the backend's arrays: ((score [rows, n], cut [rows]), counts i32 [rows * chunks], rows, n)."""
    score = be.arr(score, "f64")
    assert score.ndim == 2, "score must be [rows, n]"
    rows, n = (int(s) for s in score.shape)
    # (a Python number is made a float64 array first: as a tensor it would be rounded to float32, and the rule is inclusive)
    cut = _per_cohort(be, cut if is_cuda(cut) else np.asarray(cut, np.float64), rows)
    with _requirements_as_value_errors():
        size = int(_lib.load().dig_row_select_counts_size(rows, n))
        if size < 0:
            raise ValueError(_lib.last_error())
        counts = be.empty(size, "i32")
        be.call("dig_row_select_count", be.ptr(score), be.ptr(cut), rows, n, be.ptr(counts))
    return (score, cut), counts, rows, n


def row_select_counts(score, cut, device=0):
    """counts i32 [rows, chunks]: the selected elements of every chunk (row_select_chunk() elements) of every row of a score plane
    -- the first call of row_select alone."""
    be = backend_of(score, device=device)
    _, counts, rows, _ = _row_counts(be, score, cut)
    return counts.reshape(rows, int(counts.shape[0]) // rows if rows else 0)


def row_select(score, cut, device=0, index=True):
    """The elements of a score plane f64 [rows, n] that pass their row's cut, as ragged lists: dig_row_select_count, a cumulative
    sum, dig_row_select_fill.  cut f64 [rows] (a single value stands for every row).  Element (r, e) is selected when
    score[r, e] <= cut[r]; a NaN on either side never is, cut = +inf takes every score that is a number.
    Returns dict(index i32, score f64 [selected], row-major and ascending in e within a row; row_ptr host int64 [rows + 1]: where
    a row's list starts); index=False leaves the index out (the lists of a Benjamini-Hochberg pass).  ValueError, before the fill,
    for more than 2^31 - 1 selected elements.  CUDA tensors in -> CUDA tensors out."""
    be = backend_of(score, device=device)
    held, counts, rows, n = _row_counts(be, score, cut)                  # (held: the arrays behind the pointers stay alive)
    p = be.ptr
    with _requirements_as_value_errors():
        offsets, total, row_ptr = _scan(be, counts, groups=rows)
        if total > 2 ** 31 - 1:
            raise ValueError("%d selected elements: a smaller cut or fewer rows per call" % total)
        res = dict(index=be.empty(total, "i32")) if index else {}
        res["score"] = be.empty(total, "f64")
        be.call("dig_row_select_fill", p(held[0]), p(held[1]), rows, n, p(offsets), total, p(res.get("index")), p(res["score"]))
    res["row_ptr"] = row_ptr
    return res


def row_scatter(score, cut, values, fill=float("nan"), device=0):
    """The inverse of row_select: out f64 [rows, n] with values[slot] where (r, e) is selected -- values f64 [selected], in the order
    of row_select's lists -- and `fill` elsewhere (dig_row_select_count, a cumulative sum, dig_row_scatter).  Every element of out
    is written.  CUDA tensors in -> CUDA tensors out."""
    be = backend_of(score, values, device=device)
    held, counts, rows, n = _row_counts(be, score, cut)
    values = be.arr(values, "f64", (-1,))
    p = be.ptr
    with _requirements_as_value_errors():
        offsets, total = _scan(be, counts)
        if int(values.shape[0]) != total:
            raise ValueError("%d values for %d selected elements" % (int(values.shape[0]), total))
        out = be.empty((rows, n), "f64")
        be.call("dig_row_scatter", p(held[0]), p(held[1]), rows, n, p(offsets), total, p(values), float(fill), p(out))
    return out


GROUPS_PER_LAUNCH = 32                                   # include/dig_hip.h: M <= 32 per call of dig_group_fisher / dig_group_sums


def _group_planes(be, x, member, what):
    """(x f64 [R, C, E] -- a [C, E] plane is R = 1 --, member u8 [M, C] as 0 / 1, whether x came as 2-D, R, C, E, M)."""
    x = be.arr(x, "f64")
    if x.ndim not in (2, 3):
        raise ValueError("%s must be [C, E] or [R, C, E]" % what)
    flat = x.ndim == 2
    if flat:
        x = x.reshape((1,) + tuple(x.shape))
    R, C, E = (int(s) for s in x.shape)
    member = be.arr(member)
    if member.ndim != 2 or int(member.shape[1]) != C:
        raise ValueError("member must be [M, C] with C = %d cohorts, not %s" % (C, tuple(member.shape)))
    member = be.arr(member != 0, "u8")
    return x, member, flat, R, C, E, int(member.shape[0])


def _group_launches(be, M, R, E, flat, dtypes, call):
    """The outputs [R, M, E] of `dtypes`, filled by call(first group, groups, the outputs' slices) per slice of GROUPS_PER_LAUNCH groups
    (a slice of the groups is written into an array of its own and copied in: the entry point's output is [R, groups, E])."""
    outs = [be.empty((R, M, E), d) for d in dtypes]
    with _requirements_as_value_errors():
        for g0 in range(0, max(M, 1), GROUPS_PER_LAUNCH):
            n = min(GROUPS_PER_LAUNCH, M - g0)
            part = outs if n == M else [be.empty((R, n, E), d) for d in dtypes]
            call(g0, n, part)
            if part is not outs:
                for o, q in zip(outs, part):
                    o[:, g0:g0 + n] = q
    return [o.reshape(M, E) if flat else o for o in outs]


def group_fisher(p, member, device=0, counts=True):
    """Fisher's method over groups of cohorts, per element (dig_group_fisher): p f64 [R, C, E] or [C, E] (R stacked p-value columns, C
    <= 64 cohorts, E elements), member [M, C] (non-zero: cohort c belongs to group g).  A NaN p is not testable: it adds nothing and is
    not counted.  Returns dict(pval f64 [R, M, E], n_used i32 [R, M, E] (None with counts=False)) -- [M, E] for a 2-D p: with m = n_used
    the testable members, pval is NaN for m = 0, the member's p for m = 1, fisher_combine of the pair for m = 2 and
    chi2.sf(-2 sum ln p, 2 m) for m >= 3.  More than 32 groups run as several launches.  CUDA tensors in -> CUDA tensors out."""
    be = backend_of(p, member, device=device)
    p, member, flat, R, C, E, M = _group_planes(be, p, member, "p")

    def call(g0, n, part):
        be.call("dig_group_fisher", be.ptr(p), be.ptr(member[g0:g0 + n]), R, C, E, n, be.ptr(part[0]), be.ptr(part[1]) if counts else None)
    pval, n_used = _group_launches(be, M, R, E, flat, ("f64", "i32") if counts else ("f64",), call) + ([] if counts else [None])
    return dict(pval=pval, n_used=n_used)


def group_sums(x, member, gate=None, device=0):
    """The sums of x f64 [R, C, E] (or [C, E]) over the members of every group, in ascending cohort order, one addition per member
    (dig_group_sums): f64 [R, M, E] ([M, E]).  gate f64 of x's shape: only the members whose gate is not NaN are added.  A group with
    nothing to add gives 0.0.  More than 32 groups run as several launches.  CUDA tensors in -> CUDA tensors out."""
    be = backend_of(x, member, gate, device=device)
    x, member, flat, R, C, E, M = _group_planes(be, x, member, "x")
    if gate is not None:
        gate = be.arr(gate, "f64")
        if tuple(gate.shape) != ((C, E) if flat else (R, C, E)):
            raise ValueError("gate must have the shape of x")

    def call(g0, n, part):
        be.call("dig_group_sums", be.ptr(x), be.ptr(gate), be.ptr(member[g0:g0 + n]), R, C, E, n, be.ptr(part[0]))
    return _group_launches(be, M, R, E, flat, ("f64",), call)[0]


NB_POWER_MAX_FOLDS = 8                                   # DIG_NB_POWER_MAX_FOLDS (include/dig_hip.h)


def nb_power(alpha, theta, pi, level, scale=None, folds=(), k_max=1 << 20, device=0):
    """Critical counts of the upper mid-p burden test and the power at them (dig_nb_power): alpha, theta, pi f64 [R, n] (R rows =
    cohorts; a [n] input is R = 1), level f64 [R] and scale f64 [R] or None (a single value stands for every row), folds: at most 8
    finite numbers > 0.  With theta' = theta * scale and p(f) = 1 / ((theta' * pi) * f + 1), k_crit is the smallest k in [0, k_max]
    with nb_pvalue_greater_midp(k, alpha, p(1)) <= level -- -1 where none reaches it, the statistic is NaN or the level is not inside
    (0, 1) -- and power[j] = nb_pvalue_greater(k_crit, alpha, p(folds[j])): 0.0 where the level is out of reach, NaN for the other
    two.  Returns dict(k_crit i32 [R, n], power f64 [F, R, n], None without folds) -- [n] and [F, n] for 1-D planes.  ValueError for
    a refused requirement.  CUDA tensors in -> CUDA tensors out."""
    be = backend_of(alpha, theta, pi, level, scale, device=device)
    alpha = be.arr(alpha, "f64")
    if alpha.ndim not in (1, 2):
        raise ValueError("alpha must be [n] or [R, n]")
    flat = alpha.ndim == 1
    R, n = (1, int(alpha.shape[0])) if flat else (int(s) for s in alpha.shape)
    alpha, theta, pi = (be.arr(x, "f64").reshape((R, n)) for x in (alpha, theta, pi))
    folds = np.ascontiguousarray(np.atleast_1d(np.asarray(folds, np.float64)))
    if folds.ndim != 1 or folds.shape[0] > NB_POWER_MAX_FOLDS or not (np.isfinite(folds) & (folds > 0)).all():
        raise ValueError("folds: at most %d finite numbers > 0, not %r" % (NB_POWER_MAX_FOLDS, folds.tolist()))
    if int(k_max) != k_max or not 0 <= k_max <= 1 << 30:
        raise ValueError("k_max must be an integer in [0, 2^30], not %r" % (k_max,))
    F = int(folds.shape[0])
    # (a Python number is made a float64 array first: as a tensor it would be rounded to float32)
    level, scale = (_per_cohort(be, x if x is None or is_cuda(x) else np.asarray(x, np.float64), R) for x in (level, scale))
    k_crit, power, folds = be.empty((R, n), "i32"), be.empty((F, R, n), "f64") if F else None, be.arr(folds, "f64") if F else None
    with _requirements_as_value_errors():
        if R * n:                                            # (an empty tensor has no address, and a NULL power with folds is refused)
            be.call("dig_nb_power", be.ptr(alpha), be.ptr(theta), be.ptr(pi), be.ptr(scale), be.ptr(level), R, n, be.ptr(folds), F,
                    int(k_max), be.ptr(k_crit), be.ptr(power))
    if flat:
        k_crit, power = k_crit.reshape(n), power.reshape(F, n) if F else None
    return dict(k_crit=k_crit, power=power)


# ---------------------------------------------------------------------------
# pairs of rows of a bit matrix: intersection counts and the two one-sided Fisher exact tests (dig_pair_bits, dig_pair_fisher)
# ---------------------------------------------------------------------------
PAIR_MAX_SAMPLES, PAIR_MAX_ROWS, PAIR_TILE, PAIR_CHUNK_BITS = 65536, 8192, 64, 2048      # DIG_PAIR_* (include/dig_hip.h)


def pair_words(n_max):
    """The u64 words of a bit row that holds n_max samples: even (16-byte rows), at least 2."""
    return max(2, 2 * ((int(n_max) + 127) // 128))


def pair_index(i, j, H):
    """The slot of pair (i, j), i < j < H, in the row-major upper triangle of one cohort (numbers or arrays)."""
    return i * (2 * H - i - 1) // 2 + (j - i - 1)


def pair_plan(rows, n_samples):
    """The plan-time arrays of dig_pair_fisher, on the host: rows[c] entering rows and n_samples[c] samples per cohort ->
    dict(C, H_total, n_pairs, n_max, h_max, W, row_ptr i64 [C + 1], pair_ptr i64 [C + 1], n_samples i32 [C], tiles i32 [n_tiles, 3]).
    ValueError for what the library would refuse: more than 65 536 samples or 8 192 rows in a cohort, 2^31 pairs or more."""
    rows, n_samples = np.atleast_1d(np.asarray(rows, np.int64)), np.atleast_1d(np.asarray(n_samples, np.int64))
    if rows.ndim != 1 or rows.shape != n_samples.shape or (rows < 0).any() or (n_samples < 0).any():
        raise ValueError("rows and n_samples: one number >= 0 per cohort")
    C = int(rows.shape[0])
    n_max, h_max = (int(x.max()) if C else 0 for x in (n_samples, rows))
    if n_max > PAIR_MAX_SAMPLES:
        raise ValueError("pair_fisher: requirement failed: n_max <= 65 536 samples per cohort (got %d)" % n_max)
    if h_max > PAIR_MAX_ROWS:
        raise ValueError("pair_fisher: requirement failed: h_max <= 8 192 rows per cohort: a higher min_samples or a stricter cut "
                         "(got %d)" % h_max)
    row_ptr, pair_ptr = (np.concatenate([[0], np.cumsum(x)]).astype(np.int64) for x in (rows, rows * (rows - 1) // 2))
    if pair_ptr[-1] >= 1 << 31:
        raise ValueError("pair_fisher: requirement failed: fewer than 2^31 pairs per call: fewer cohorts per call (got %d)" % pair_ptr[-1])
    tiles = [np.zeros((0, 3), np.int32)]
    for c in range(C):
        bi, bj = np.triu_indices((int(rows[c]) + PAIR_TILE - 1) // PAIR_TILE if rows[c] > 1 else 0)
        tiles.append(np.stack([np.full(bi.shape, c), bi, bj], 1).astype(np.int32))
    return dict(C=C, H_total=int(row_ptr[-1]), n_pairs=int(pair_ptr[-1]), n_max=n_max, h_max=h_max, W=pair_words(n_max), row_ptr=row_ptr,
                pair_ptr=pair_ptr, n_samples=n_samples.astype(np.int32), tiles=np.ascontiguousarray(np.concatenate(tiles)))


def _pair_bits_arg(be, bits, H_total, W):
    """bits as the backend's i64 [H_total, W] (a numpy uint64 array is viewed, not converted)."""
    if isinstance(bits, np.ndarray) and bits.dtype == np.uint64:
        bits = np.ascontiguousarray(bits).view(np.int64)
    bits = be.arr(bits, "i64")
    if tuple(bits.shape) != (H_total, W):
        raise ValueError("bits must be [%d, %d] (rows, pair_words(max n_samples)), not %r" % (H_total, W, tuple(bits.shape)))
    return bits


def pair_bits(row, sample, H_total, W, device=0):
    """The stacked bit matrix of distinct (row, sample) keys (dig_pair_bits): row i32 [K] -- a row of the matrix, -1 where the key's
    element does not enter --, sample i32 [K] the cohort-local sample index.  Returns bits i64 [H_total, W] (the bytes of u64 words:
    sample s is bit s % 64 of word s / 64), W = pair_words(the largest n_samples).  Repeated keys are harmless.  ValueError for a
    refused requirement.  CUDA tensors in -> a CUDA tensor out."""
    be = backend_of(row, sample, device=device)
    row, sample = be.arr(row, "i32", (-1,)), be.arr(sample, "i32", (-1,))
    if row.shape != sample.shape:
        raise ValueError("row and sample: one of each per key")
    H_total, W, K = int(H_total), int(W), int(row.shape[0])
    if H_total < 0 or W < 2 or W % 2 or W > PAIR_MAX_SAMPLES // 64:
        raise ValueError("pair_bits: requirement failed: H_total >= 0, W even, 2 <= W <= 1024 (got %d, %d)" % (H_total, W))
    bits = be.empty((H_total, W), "i64")
    with _requirements_as_value_errors():
        if H_total:
            be.call("dig_pair_bits", be.ptr(row) if K else None, be.ptr(sample) if K else None, K, H_total, W, be.ptr(bits))
    return bits


def pair_fisher(bits, rows, n_samples, device=0, tails=True):
    """Per pair of rows of each cohort the size of the intersection and the two one-sided Fisher exact p-values (dig_pair_fisher;
    include/dig_hip.h states the rule): bits i64 / u64 [H_total, W] from pair_bits, rows[c] the rows of cohort c (stacked in cohort
    order), n_samples[c] its samples -- host numbers, the plan (pair_plan).  Returns dict(n_row i32 [H_total], n_both i32 [n_pairs],
    pval_cooccur, pval_exclusive f64 [n_pairs] (None with tails=False: dig_pair_counts), pair_ptr: host i64 [C + 1], plan); pair
    (i, j) of cohort c is at pair_ptr[c] + pair_index(i, j, rows[c]).  ValueError for a refused requirement.  CUDA tensors in -> CUDA
    tensors out."""
    be = backend_of(bits, device=device)
    plan = pair_plan(rows, n_samples)
    H_total, P, W = plan["H_total"], plan["n_pairs"], plan["W"]
    bits = _pair_bits_arg(be, bits, H_total, W)
    n_row, n_both = be.empty(H_total, "i32"), be.empty(P, "i32")
    p_co, p_ex = (be.empty(P, "f64"), be.empty(P, "f64")) if tails else (None, None)
    if H_total:
        dev = {k: be.arr(plan[k]) for k in ("row_ptr", "n_samples", "pair_ptr", "tiles")}
        head = (be.ptr(bits), H_total, W, be.ptr(dev["row_ptr"]), be.ptr(dev["n_samples"]), be.ptr(dev["pair_ptr"]), plan["C"],
                be.ptr(dev["tiles"]) if len(plan["tiles"]) else None, len(plan["tiles"]), P, plan["n_max"], plan["h_max"])
        ptr = lambda x: be.ptr(x) if x is not None and P else None                 # (an empty tensor has no address)
        with _requirements_as_value_errors():
            if tails:
                lnfact = be.empty(plan["n_max"] + 1, "f64")
                be.call("dig_pair_fisher", *head, be.ptr(lnfact), be.ptr(n_row), ptr(n_both), ptr(p_co), ptr(p_ex))
            else:
                be.call("dig_pair_counts", *head, be.ptr(n_row), ptr(n_both))
    return dict(n_row=n_row, n_both=n_both, pval_cooccur=p_co, pval_exclusive=p_ex, pair_ptr=plan["pair_ptr"], plan=plan)


MAP_TAILS ={"upper": 0, "side": 1}                      # `tail` of dig_map_windows (include/dig_hip.h)
MAP_LEVELS = (0.05, 0.01, 0.001, 0.0001)                 # the levels of N_BELOW (gp_tools.py:117-121)
MAP_COUNTS = ("N_WINDOWS", "N_TESTED", "OBS_TOTAL") + tuple("N_BELOW_%g" % a for a in MAP_LEVELS)
MAP_SUMS = ("EXP_TOTAL", "SXX", "SYY", "SXY")


def map_windows(mu_cm, std_cm, y_cm, flag_cm, run_ptr, drop_flagged=False, tail="upper", device=0):
    """A map's bins merged into larger windows with the region test per window (dig_map_windows; gp_tools.merge_windows,
    gp_tools.py:125-160): mu_cm, std_cm f64, y_cm i32, flag_cm u8 (None without drop_flagged) [C, N] cohort-major (a [N] input is
    C = 1), run_ptr i64 [M + 1]: window m = bins run_ptr[m] .. run_ptr[m + 1] - 1.  tail: 'upper' (nb_pvalue_greater_midp, the burden
    test) or 'side' (nb_pvalue_midp).  Returns dict(n_bins i32, y_true i64, y_pred f64, std f64, pval f64), each [C, M]: the sums of
    the bins that are not gated out (a flagged bin with drop_flagged), the float sums sequential in ascending bin order, pval NaN for
    a window without a bin left.  ValueError for a refused requirement.  CUDA tensors in -> CUDA tensors out."""
    if tail not in MAP_TAILS:
        raise ValueError("tail must be 'upper' or 'side', not %r" % (tail,))
    be = backend_of(mu_cm, std_cm, y_cm, flag_cm, run_ptr, device=device)
    mu_cm = be.arr(mu_cm, "f64")
    if mu_cm.ndim not in (1, 2):
        raise ValueError("mu_cm must be [N] or [C, N]")
    C, N = (1, int(mu_cm.shape[0])) if mu_cm.ndim == 1 else (int(s) for s in mu_cm.shape)
    std_cm, y_cm, flag_cm = be.arr(std_cm, "f64", (C, N)), be.arr(y_cm, "i32", (C, N)), be.arr(flag_cm, "u8", (C, N))
    if drop_flagged and flag_cm is None:
        raise ValueError("drop_flagged needs flag_cm")
    run_ptr = be.arr(run_ptr, "i64", (-1,))
    M = int(run_ptr.shape[0]) - 1
    if M < 0:
        raise ValueError("run_ptr must hold at least one offset")
    out = dict(n_bins=be.empty((C, M), "i32"), y_true=be.empty((C, M), "i64"), y_pred=be.empty((C, M), "f64"),
               std=be.empty((C, M), "f64"), pval=be.empty((C, M), "f64"))
    p = be.ptr
    with _requirements_as_value_errors():
        if C * M:                                            # (an empty tensor has no address)
            be.call("dig_map_windows", p(mu_cm), p(std_cm), p(y_cm), p(flag_cm) if drop_flagged else None, C, N, p(run_ptr), M,
                    int(bool(drop_flagged)), MAP_TAILS[tail], p(out["n_bins"]), p(out["y_true"]), p(out["y_pred"]), p(out["std"]),
                    p(out["pval"]))
    return out


def map_scores(n_bins, y_true, y_pred, pval, device=0):
    """The per-cohort scores of merged planes [C, M] (dig_map_scores), over the windows with n_bins > 0: dict(counts i64 [C, 7]:
    MAP_COUNTS -- N_WINDOWS, N_TESTED (pval not NaN), OBS_TOTAL, the windows with pval < 0.05, 0.01, 0.001, 0.0001 --, sums f64
    [C, 4]: MAP_SUMS -- EXP_TOTAL and the sums of squares and products centred on the two means).  The float sums are taken in an
    order fixed by (M, C): the same bits on any stream and through the host twin.  CUDA tensors in -> CUDA tensors out."""
    be = backend_of(n_bins, y_true, y_pred, pval, device=device)
    n_bins = be.arr(n_bins, "i32")
    if n_bins.ndim != 2:
        raise ValueError("n_bins must be [C, M]")
    C, M = (int(s) for s in n_bins.shape)
    y_true, y_pred, pval = be.arr(y_true, "i64", (C, M)), be.arr(y_pred, "f64", (C, M)), be.arr(pval, "f64", (C, M))
    out = dict(counts=be.empty((C, len(MAP_COUNTS)), "i64"), sums=be.empty((C, len(MAP_SUMS)), "f64"))
    p = be.ptr
    with _requirements_as_value_errors():
        if C:
            be.call("dig_map_scores", p(n_bins), p(y_true), p(y_pred), p(pval), C, M, p(out["counts"]), p(out["sums"]),
                    workspace=_shared_workspace(be, "map_scores", C, M))
    return out


# ---------------------------------------------------------------------------
# scale factors in canonical chunks: identical bits for any sharding of the bins (dig_scale_suffstats_chunked)
# ---------------------------------------------------------------------------
class ChunkedScaleFactorPlan:
    """Scale factors of one shard of the bin grid (transfer_tools.py:148-156) with cached arguments.

    bin_mu / bin_flag: this rank's rows (device tensors, halo included); chunk_rows: first row, in THIS table, of every
    canonical chunk the rank owns (+ end) -- parallel.canonical_chunks / parallel.plan_shards give them; n_snv_obs,
    n_ind_obs: this rank's observed counts per cohort (integers).  run():
        own chunk sums (dig_scale_suffstats_chunked) -> all-gather of [chunk sums ; observed counts] over the process group
        -> every rank adds the K chunk sums first to last and divides (dig_scale_factors_chunked).
    Without a process group the all-gather is skipped: same kernels, same bits."""

    def __init__(self, bin_mu, bin_flag, n_snv_obs, n_ind_obs, chunk_rows, n_chunks_total, group=None, world=None, premask=True):
        """premask: keep a plan-time copy of bin_mu with +0.0 in the flagged entries and sum THAT every step (8 instead of 9
        bytes per (bin, cohort) and step, the same additions and bits); call `remask()` after changing a table in place."""
        import torch
        import torch.distributed as dist
        dev = bin_mu.device
        self.mu, self.flag = _t(bin_mu, "f64", dev), _t(bin_flag, "u8", dev)
        self.masked = None
        if premask:
            self.masked = torch.empty_like(self.mu)
            self.remask()
        self.C = int(self.mu.shape[1])
        self.chunk_rows = np.ascontiguousarray(chunk_rows, np.int64)
        self.n_own, self.n_total, self.group = len(self.chunk_rows) - 1, int(n_chunks_total), group
        self.dist_world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        # (world may be given explicitly to walk the ranks of a plan one after the other on one device:
        #  enqueue_part() per rank, then finish() on the stacked parts -- tests/test_gpu_sharded.py)
        self.world = int(world) if world is not None else self.dist_world
        assert self.n_own * self.world == self.n_total, "every rank owns n_chunks_total / world canonical chunks"
        lib = _lib.load()
        self.wsb = int(lib.dig_scale_suffstats_chunked_workspace(_lib.host_ptr(self.chunk_rows), self.n_own, self.C))
        self.ws = torch.empty(max(self.wsb, 8), dtype=torch.uint8, device=dev)
        # what a rank contributes: its chunk sums [n_own, C] followed by its observed counts [2, C]
        self.part = torch.zeros((self.n_own + 2, self.C), dtype=torch.float64, device=dev)
        self.part[self.n_own] = _t(n_snv_obs, "f64", dev)
        self.part[self.n_own + 1] = _t(n_ind_obs, "f64", dev)
        # the exchange step: with more than one rank, or when parallel.FORCE_COLLECTIVES sends a world of one through RCCL too
        from . import parallel
        self.exchange = self.world == self.dist_world and parallel.collectives_on(group)
        self.all = torch.empty((self.world, self.n_own + 2, self.C), dtype=torch.float64, device=dev) \
            if (self.world > 1 or self.exchange) else None
        self.sums = torch.empty((self.n_total, self.C), dtype=torch.float64, device=dev)
        self.obs = torch.empty((self.world, 2, self.C), dtype=torch.float64, device=dev)
        self._lib = lib

    def remask(self):
        """(Re)build the masked copy of the rate table on torch's current stream."""
        import torch
        if self.masked is not None:
            torch.where(self.flag != 0, torch.zeros((), dtype=torch.float64, device=self.mu.device), self.mu, out=self.masked)

    def enqueue_part(self, stream=None):
        """This rank's contribution [n_own + 2, C]: chunk sums of its own chunks, then its observed counts."""
        p = _lib.dev_ptr
        mu, flag = (self.masked, None) if self.masked is not None else (self.mu, self.flag)
        rc = self._lib.dig_scale_suffstats_chunked(p(mu), p(flag), self.C, _lib.host_ptr(self.chunk_rows), self.n_own,
                                                   p(self.part), p(self.ws), self.wsb, _lib.stream_ptr(stream))
        _lib.check("dig_scale_suffstats_chunked", rc)
        return self.part

    def _on(self, stream):
        """Context in which torch's own work (copies, the collective) lands on `stream` -- the kernels of this plan take the
        stream as an argument, torch's operations take the CURRENT stream, and the two must be the same queue."""
        import contextlib
        import torch
        return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()

    def finish(self, all_parts, cj, cj_indel, out_sum=None, stream=None):
        """all_parts [world, n_own + 2, C] (rank order = chunk order) -> scale factors on this rank."""
        p = _lib.dev_ptr
        if self.world > 1:
            with self._on(stream):
                self.sums.view(self.world, self.n_own, self.C).copy_(all_parts[:, :self.n_own])
                self.obs.copy_(all_parts[:, self.n_own:])
            sums, obs = self.sums, self.obs
        else:
            sums, obs = all_parts[0, :self.n_own], all_parts[0, self.n_own:]
        rc = self._lib.dig_scale_factors_chunked(p(sums), self.n_total, p(obs), self.world, self.C,
                                                 p(out_sum) if out_sum is not None else None, p(cj), p(cj_indel),
                                                 _lib.stream_ptr(stream))
        _lib.check("dig_scale_factors_chunked", rc)

    def run(self, cj, cj_indel, out_sum=None, stream=None):
        """Enqueue on `stream` (default: torch's current stream).  With a process group the all-gather and the copies that
        unpack it are issued with `stream` made current, so they are ordered with the two kernels around them."""
        import torch.distributed as dist
        assert self.world in (1, self.dist_world), "run() needs the process group the plan was built for"
        part = self.enqueue_part(stream)
        if self.exchange:
            with self._on(stream):
                dist.all_gather_into_tensor(self.all, part, group=self.group)
            self.finish(self.all, cj, cj_indel, out_sum, stream)
        else:
            self.finish(part.unsqueeze(0), cj, cj_indel, out_sum, stream)


class StageTimer:
    """How long did the dot kernel / the statistics kernel of a dig_element_pipeline call run?  (dig_stage_timer_*, include/dig_hip.h:
    the kernel's own begin and end, taken from its dispatch -- nothing is added to the stream.)

        tm = StageTimer(); tm.arm(_lib.DIG_PIPE_STATISTICS); plan.run(...); ms = tm.read_ms(); tm.close()
    """

    def __init__(self):
        import ctypes
        self._h = ctypes.c_void_p()
        _lib.call("dig_stage_timer_create", ctypes.byref(self._h))

    def arm(self, stage):
        _lib.call("dig_stage_timer_arm", self._h, int(stage))

    def read_ms(self):
        import ctypes
        ms = ctypes.c_double()
        _lib.call("dig_stage_timer_read", self._h, ctypes.byref(ms))
        return float(ms.value)

    def selftest(self, stream=None):
        """Time a kernel that does nothing (then read_ms()): what of a reading is dispatch, not kernel."""
        _lib.call("dig_stage_timer_selftest", self._h, _lib.stream_ptr(stream))

    def close(self):
        if self._h:
            _lib.call("dig_stage_timer_destroy", self._h)
            import ctypes
            self._h = ctypes.c_void_p()
