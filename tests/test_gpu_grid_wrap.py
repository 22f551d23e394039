"""Every kernel whose grid is capped by the CU count, run past its cap: two full passes of the grid and a ragged third, against
the references the other test modules already state (the numpy hit rule, the context oracle, the gene statement, numpy indexing,
the per-row rule of the mutation contexts).  The loops over gridDim carry state from pass to pass -- LDS histograms that are
re-zeroed, counters that are never cleared, a position stepped by a precomputed stride, prefetched pairs -- and the shapes of
the other modules end inside the first pass.  Sizes come from CAPS below and the CU count of the card; a reference is computed
once on a small set of unique cases and the large input draws from it by index, so that what a block, wave or lane sees differs
from one pass to the next and a stale histogram shows as a wrong row.  Everything is compared exactly.

The last test is of the same nature without a grid cap: mutctx_resolve_kernel carries a run of rows over waves through
wave_last, 64 waves per step of its look-back; runs of up to 8 300 rows take it through three steps."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# Items per pass of the grid as a function of the CU count, one entry per kernel, each with the launch it mirrors.
CAPS = {
    # dig_tilehits.hip, dig_tile_select_count: grid_for((n - lead) >> 1, kTileHitBlock = 256) blocks, default 8 per CU, a pair
    # of elements per lane; a trip of the kernel's loop is two such blocks of pairs.  In elements per block of pairs:
    "tile_count": lambda cus: 2 * 8 * cus * 256,
    # dig_context.hip, dig_count_contexts2: grid_for(R, kC2Block = 256, 1), one lane per region
    "context_count2": lambda cus: cus * 256,
    # dig_context.hip, dig_count_contexts: grid_for(R * 64, kCtxBlock = 256, DIG_CTX_PER_CU = 6), one wave per region
    # (csrc/Makefile passes no -D: the value is the source's default)
    "context_count": lambda cus: cus * 6 * 4,
    # dig_genesites.hip, dig_gene_site_counts: cap = cu_count() * 64 workgroups, one gene each
    "gene_site_counts": lambda cus: cus * 64,
    # dig_gather.hip, launch_gather: min(B, cu_count() * 8) workgroups, one bin each (gather_rows_kernel, gather_rows_subset_kernel)
    "gather_rows": lambda cus: cus * 8,
    "gather_subset": lambda cus: cus * 8,
    # ... min((n_groups + 3) / 4, cu_count() * 4) workgroups of four waves, one row group per wave (gather_rows_subset_wide_kernel)
    "gather_wide": lambda cus: cus * 4 * 4,
    # ... gy = min(B, max(1, cu_count() * 8 / tiles)) bins (gather_transpose_kernel), cu_count() * 16 / tiles (gather_transpose_all_kernel)
    "gather_transpose": lambda cus, tiles: max(1, cus * 8 // tiles),
    "gather_transpose_all": lambda cus, tiles: max(1, cus * 16 // tiles),
    # ... gather_block_kernel: gy = min(B, 65535) bins; min(.., 64) chunks of kGatherBlock * kBlockUnroll = 1024 four-value vectors
    "gather_block_y": lambda cus: 65535,
    "gather_block_x": lambda cus: 64 * 256 * 4,
}


def past(cap):
    """Two full passes and a ragged third."""
    return 2 * cap + cap // 8 + 37


@pytest.fixture(scope="module")
def cus():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


# ---- 1. dig_tile_select_count / fill past one trip ----------------------------------------------------------------------------------
TILE_CUT = 0.003            # a wave looks at 128 scores per half trip: at 0.3 % of them below the cut two waves in three leave early
TILE_PLANES = [             # (R, T, blocks of pairs, lead, kinds of cut): C is sized from the cap
    # stride of a block at 256 CUs (c, r, t) = (0, 684, 1372): t carries on most steps
    (1151, 1531, 5, 0, "finite inf -1"), (1151, 1531, 5, 0, "nan finite inf"),
    (1151, 1531, 5, 1, "finite inf -1"),                                   # the plane at 8 (mod 16): every pair one element on
    (3, 251, 5, 0, "mixed"),                                               # (1392, 1, 149): carries through t, r and c
    (3, 251, 4, 0, "mixed"),                                               # four blocks and a rest: a last trip with part of A and no B
    (2500, 1, 5, 0, "mixed"),                                              # (419, 1076, 0): the element before is always in another row
]


def tile_plane(R, T, n_blocks, kinds, cus, seed):
    """(score [C, R, T], n_valid, cut [C], k): at least n_blocks blocks of pairs and a rest.  The planes of test_gpu_tile_hits.py
    hold 2 % of -inf and a last row below every cut, which leaves no wave without a hit; here 0.02 % are -inf and a finite cut
    takes 0.3 %.  Around every block boundary (of the plane at 0 and at 8 (mod 16)) three scores are -inf, in a row that exists
    whole.  At 256 CUs the last wave holds 7, 47, 63 and 52 pairs in the four shapes, and the first shape ends in a single element."""
    block = CAPS["tile_count"](cus)
    C = -(-(n_blocks * block + block // 50) // (R * T))
    rng = np.random.default_rng(seed)
    shape = (C, R, T)
    score = rng.uniform(size=shape)
    u = rng.uniform(size=shape)
    score[u < 0.1] = np.nan
    score[u > 0.98] = np.inf
    score[(u > 0.5) & (u < 0.5002)] = -np.inf
    nv = rng.integers(-1, T + 1, R).astype(np.int32)
    nv[rng.uniform(size=R) < 0.5] = T
    nv[:3] = [T, 0, -1][:min(R, 3)]
    nv[R - 1] = T
    flat = score.reshape(-1)
    for b in range(block, flat.size - 1, block):
        rows = {(b // T) % R, ((b + 1) // T) % R}
        if R > 16:
            nv[list(rows)] = T                                              # (plenty of other rows stay short)
        if all(nv[r] == T for r in rows):
            flat[b - 1:b + 2] = -np.inf
    assert (nv < T).any() and (nv <= 0).any()
    if kinds == "mixed":
        c = np.arange(C)
        cut = np.where(c % 7 == 3, -1.0, np.where(c % 11 == 5, np.nan, np.where(c % 997 == 1, np.inf, TILE_CUT)))
    else:
        kinds = [dict(finite=TILE_CUT, inf=np.inf, nan=np.nan)[w] if w != "-1" else -1.0 for w in kinds.split()]
        cut = np.array([kinds[c % len(kinds)] for c in range(C)])
    return score, nv, cut, rng.integers(0, 7, shape).astype(np.int32)


def tile_blocks(n, lead, cus):
    """The kernel's split of a plane of n elements: (elements of a block of pairs, the block of every element; -1 for the one or
    two elements outside the pairs)."""
    n_pairs = (n - lead) >> 1
    stride = min(-(-n_pairs // 256), 8 * cus) * 256
    blk = np.full(n, -1, np.int64)
    blk[lead:lead + 2 * n_pairs] = (np.arange(2 * n_pairs) // 2) // stride
    return 2 * stride, blk


def tile_reference_checks(score, nv, cut, lead, cus, n_blocks, every_block):
    """What the reference alone must show before the kernel runs: more than two trips, hits in every
    block of pairs of every trip (A and B halves are the even and the odd blocks), a (c, r) row across a block boundary with hits
    on both sides, and -- at the finite cut -- waves with and without a score below the cut."""
    C, R, T = score.shape
    n = score.size
    block, blk = tile_blocks(n, lead, cus)
    assert block == CAPS["tile_count"](cus) and n > 2 * (2 * block), "more than two trips of two blocks of pairs"
    n_pairs = (n - lead) >> 1
    assert blk.max() >= n_blocks
    with np.errstate(invalid="ignore"):
        below = (score <= cut.reshape(C, 1, 1)).reshape(-1)
        hit = ((np.arange(T)[None, None, :] < nv[None, :, None]) & (score <= cut.reshape(C, 1, 1))).reshape(-1)
    per_block = np.bincount(blk[hit & (blk >= 0)], minlength=blk.max() + 1)
    if every_block:
        assert (per_block > 0).all(), per_block
    both = 0
    for b in range(lead + block, n, block):
        row = b // T
        if b > row * T:
            both += hit[row * T:b].any() and hit[b:(row + 1) * T].any()
    assert both > 0 or T == 1                                              # (T = 1: no row has two sides)
    pairs = below[lead:lead + 2 * (n_pairs // 64) * 64].reshape(-1, 128).any(axis=1)     # a wave's 64 pairs of a half trip
    assert 0.05 < pairs.mean() < 0.95 or not every_block
    return per_block


@pytest.mark.parametrize("R,T,n_blocks,lead,kinds", TILE_PLANES, ids=lambda v: str(v).replace(" ", "_"))
def test_tile_select_past_one_trip_of_the_grid(cus, R, T, n_blocks, lead, kinds):
    """engine.tile_select / tile_select_counts on planes of four or five blocks of pairs and an odd rest (the second half of a
    trip, step / step2 / tile_pos_advance with every kind of carry, a second and a third trip), against the numpy hit rule."""
    import torch
    from digdriver_amd import engine
    from test_gpu_tile_hits import _expected
    score, nv, cut, k = tile_plane(R, T, n_blocks, kinds, cus, seed=R + T + n_blocks)
    C = score.shape[0]
    tile_reference_checks(score, nv, cut, lead, cus, n_blocks, every_block="nan" not in kinds)
    want, want_counts = _expected(score, nv, cut, dict(k=k))
    assert len(want["tile"]) > 1000
    dev = torch.device("cuda:0")
    if lead:
        room = torch.empty(score.size + 1, dtype=torch.float64, device=dev)
        d_score = room[1:].view(C, R, T)
        d_score.copy_(torch.as_tensor(score))
    else:
        d_score = torch.as_tensor(score, device=dev)
    assert d_score.is_contiguous() and (d_score.data_ptr() >> 3) & 1 == lead
    d_nv, d_k = torch.as_tensor(nv, device=dev), torch.as_tensor(k, device=dev)
    counts = engine.tile_select_counts(d_score, d_nv, cut).cpu().numpy()
    assert counts.shape == (C, R)
    bad = np.flatnonzero(counts.reshape(-1) != want_counts)
    assert bad.size == 0, (bad.size, bad[:5], counts.reshape(-1)[bad[:5]], want_counts[bad[:5]])
    got = engine.tile_select(d_score, d_nv, cut, k=d_k)
    assert np.array_equal(got["cohort_ptr"], want["cohort_ptr"])
    for name in ("region", "tile", "score", "k"):
        g = got[name].cpu().numpy()
        assert g.dtype == want[name].dtype and g.tobytes() == want[name].tobytes(), name


# ---- 2. trinucleotide context counts, both forms, past one pass ---------------------------------------------------------------------
def context_cases(p_n, seed):
    """The genome and regions of test_context_counting_2bit_form_on_letter_runs_and_every_alignment (test_gpu_parity.py):
    (seqs, chroms, starts, ends)."""
    rng = np.random.default_rng(seed)
    seqs = {"chr1": "".join(rng.choice(list("ACGTN"), 30_011, p=[(1 - p_n) / 4] * 4 + [p_n])),
            "chr2": "".join(rng.choice(list("ACGT"), 5_003)),
            "chr3": "N" * 10 + "".join(rng.choice(list("ACGT"), 300)) + "N" * 700 + "ACGNAC" + "".join(rng.choice(list("ACGT"), 4000))}
    names = list(seqs)
    regs = []
    for _ in range(6000):
        c = names[int(rng.integers(0, 3))]
        n = len(seqs[c])
        a = int(rng.integers(0, n))
        e = a + int(rng.integers(0, (5, 70, 300, 3000)[int(rng.integers(0, 4))]))
        u = rng.uniform()
        regs.append((c, 0 if u < 0.03 else a, n + 5 if u > 0.95 else e))
    regs += [("chr3", 300 + k, 1020 + k) for k in range(70)] + [("chr3", k, k + 1) for k in range(40)]
    chroms, starts, ends = (np.array(x) for x in zip(*regs))
    assert (starts == 0).sum() > 50 and sum(e > len(seqs[c]) for c, _, e in regs) > 50
    return seqs, chroms, starts, ends


@pytest.fixture(scope="module", params=[0.0, 0.2], ids=["N-free", "a fifth N"])
def context_oracle(request):
    """The oracle's rows of the unique regions, computed once on the plus strand; a minus-strand row is the oracle's own gather of
    it (count_contexts_regions: out[ctx] = plus[revcomp(ctx)])."""
    from digdriver_amd.data_tools.genome import PackedGenome
    from oracle import dig_oracle as O
    seqs, chroms, starts, ends = context_cases(request.param, seed=43)
    plus = O.count_contexts_regions(seqs, list(chroms), list(starts), list(ends))
    assert plus.shape == (len(chroms), 64) and plus.sum() > 0
    return dict(genome=PackedGenome.from_sequences(seqs), chroms=chroms, starts=starts, ends=ends, plus=plus,
                minus=plus[:, O.minus_strand_gather64()])


@pytest.mark.parametrize("form", ["2bit", "4bit"])
def test_context_counts_past_one_pass_of_the_grid(cus, context_oracle, form):
    """context_count2_kernel (a lane per region: its counters are never cleared, its totals run on from region to region) and
    context_count_kernel (a wave per region: its LDS histogram is zeroed per region) on more than two passes of regions drawn
    by index from the oracle's rows, on either strand."""
    from digdriver_amd import engine
    cap = CAPS["context_count2" if form == "2bit" else "context_count"](cus)
    R = past(cap)
    assert R > 2 * cap
    c = context_oracle
    rng = np.random.default_rng(cap)
    idx, minus = rng.integers(0, len(c["chroms"]), R), rng.uniform(size=R) < 0.5
    assert (idx[:cap] != idx[cap:2 * cap]).mean() > 0.99                   # what a lane / wave sees changes from pass to pass
    assert (c["plus"] != c["minus"]).any(axis=1).mean() > 0.5
    got = engine.count_contexts(c["genome"], c["chroms"][idx], c["starts"][idx], c["ends"][idx], minus, device=0, form=form).cpu().numpy()
    want = np.where(minus[:, None], c["minus"][idx], c["plus"][idx])
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (form, bad.size, bad[:5], idx[bad[:5]], minus[bad[:5]])


# ---- 3. dig_gene_site_counts past one pass -------------------------------------------------------------------------------------------
from test_gpu_gene_site_counts import fuzz  # noqa: E402,F401  (the 304 fuzz genes and their statement rows, as a fixture of this module too)


def repeat_ragged(ptr, idx, *arrays):
    """The ragged rows idx of (ptr, arrays) one after the other: (their ptr, the arrays)."""
    n = np.diff(ptr)[idx]
    new_ptr = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    src = np.repeat(ptr[idx] - new_ptr[:-1], n) + np.arange(new_ptr[-1])
    return new_ptr, [np.ascontiguousarray(a[src]) for a in arrays]


def test_gene_site_counts_past_one_pass_of_the_grid(cus, fuzz):  # noqa: F811
    """The device entry point itself on a table of genes drawn by index from the fuzz genes: a workgroup's LDS counters and
    its `other` flag are reset per gene, so a gene after one left to the host comes out whole, and the other way round.  The
    genes left to the host stay as zero rows with GS_HOST: nothing is finished from letters."""
    import torch
    from digdriver_amd import _lib, engine
    cap = CAPS["gene_site_counts"](cus)
    G = past(cap)
    assert G > 2 * cap
    genes, other = fuzz["genes"], fuzz["other"]
    idx = np.random.default_rng(5).integers(0, len(genes), G)
    # a workgroup takes the genes b, b + cap, b + 2 cap: both orders of (left to the host, whole) occur in consecutive passes
    a, b = other[idx[:G - cap]], other[idx[cap:]]
    assert (a & ~b).sum() > 100 and (~a & b).sum() > 100 and (idx[:G - cap] != idx[cap:]).mean() > 0.99
    blk_ptr, (blk_start, blk_end, cds_off) = repeat_ragged(genes.blk_ptr, idx, genes.blk_start, genes.blk_end, genes.cds_off)
    spl_ptr, (spl_pos,) = repeat_ragged(genes.spl_ptr, idx, genes.spl_pos)
    assert blk_ptr[-1] == len(blk_start) > G and spl_ptr[-1] == len(spl_pos) > 0
    dev = torch.device("cuda:0")
    table = [torch.as_tensor(np.ascontiguousarray(x), device=dev) for x in
             (fuzz["gch"][idx].astype(np.int32), genes.minus[idx].astype(np.uint8), blk_ptr, blk_start.astype(np.int64),
              blk_end.astype(np.int64), cds_off.astype(np.int64), spl_ptr, spl_pos.astype(np.int64))]
    L = torch.full((G, 4, 192), -1, dtype=torch.int32, device=dev)
    nsl = torch.full((G,), -1, dtype=torch.int32, device=dev)
    status = torch.full((G,), 9, dtype=torch.uint8, device=dev)
    p = _lib.dev_ptr
    _lib.call("dig_gene_site_counts", *fuzz["g"].genome2_args(dev), *[p(t) for t in table], G, p(L), p(nsl), p(status), _lib.stream_ptr())
    torch.cuda.synchronize()
    whole = ~other[idx]
    assert np.array_equal(status.cpu().numpy(), np.where(whole, engine.GS_OK, engine.GS_HOST).astype(np.uint8))
    assert np.array_equal(nsl.cpu().numpy(), np.where(whole, fuzz["nsl"][idx], 0))
    got = L.cpu().numpy()
    bad = np.flatnonzero((got != np.where(whole[:, None, None], fuzz["L"][idx], 0)).any(axis=(1, 2)))
    assert bad.size == 0, (bad.size, bad[:5], idx[bad[:5]], whole[bad[:5]])


# ---- 4. dig_gather_bins, all six kernels past their caps -----------------------------------------------------------------------------
_NP = {"i16": np.int16, "f32": np.float32, "f64": np.float64}
_OUT_BYTES = {"f32": 4, "bf16": 2}


def gather_values(rng, src, shape):
    return (rng.integers(-1200, 12000, shape) / (1 if src == "i16" else 4)).astype(_NP[src])       # (exact in float32)


def gather_and_compare(x, xd, rows, tracks, dst, transpose):
    """engine.gather_bins on device tensors against numpy indexing, bit for bit; returns the kernel launch_gather chose."""
    import torch
    from digdriver_amd import engine
    from test_gpu_guarded_calls import gather_kernel
    N, L, T = x.shape
    d_tracks = None if tracks is None else torch.as_tensor(tracks.astype(np.int32), device=xd.device)
    got = engine.gather_bins(xd, torch.as_tensor(rows, device=xd.device), d_tracks, out_dtype=dst, transpose=transpose)
    want = x[rows].astype(np.float32) if tracks is None else x[rows][:, :, tracks].astype(np.float32)
    want = torch.from_numpy(np.ascontiguousarray(want.transpose(0, 2, 1)) if transpose else want)
    if dst == "bf16":
        assert got.dtype == torch.bfloat16
        same = torch.equal(got.cpu().view(torch.int16), want.to(torch.bfloat16).view(torch.int16))
    else:
        assert got.dtype == torch.float32
        same = torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))
    T_sel = T if tracks is None else len(tracks)
    which = gather_kernel(x.itemsize, _OUT_BYTES[dst], L, T, T_sel, tracks is not None, transpose, xd.data_ptr(), got.data_ptr(),
                          0 if d_tracks is None else d_tracks.data_ptr())
    assert same, (which, x.dtype, dst, x.shape, transpose)
    return which


@pytest.mark.parametrize("src", ["i16", "f32", "f64"])
def test_gather_bins_past_one_pass_of_every_capped_grid(cus, src):
    """rows, subset, wide, transpose and transpose_all with more than two passes of bins (of row groups for the wide kernel),
    drawn with repeats from 50 source bins; gather_kernel() of test_gpu_guarded_calls.py says which kernel a call reached."""
    import torch
    rng = np.random.default_rng(_NP[src]().itemsize)
    dev = torch.device("cuda:0")
    N, S = 50, _NP[src]().itemsize
    group = 8 // S                                                          # positions per row group of the wide kernel
    sel44 = np.concatenate([np.arange(3, 43), [1, 70, 76, 5]])
    sel41 = sel44[:41]
    seen = {}
    # (L, T, tracks, transpose, dst, the kernel it must reach, that kernel's bins per pass)
    cases = [(12, 77, sel44, False, "f32", "wide", -(-CAPS["gather_wide"](cus) // (12 // group))),
             (12, 77, sel44, False, "bf16", "subset", CAPS["gather_subset"](cus)),        # 88 bytes per output row: not the wide kernel's
             (13, 77, sel41, False, "f32", "rows", CAPS["gather_rows"](cus)),
             (13, 77, sel41, False, "bf16", "rows", CAPS["gather_rows"](cus)),
             (13, 64, None, True, "f32", "transpose", CAPS["gather_transpose"](cus, 1)),
             (12, 77, sel44, True, "bf16", "transpose", CAPS["gather_transpose"](cus, 1)),
             (12, 77, None, True, "f32", "transpose_all", CAPS["gather_transpose_all"](cus, 2)),
             (12, 77, None, True, "bf16", "transpose_all", CAPS["gather_transpose_all"](cus, 2))]
    if src != "f64":
        cases.append((13, 64, np.arange(3, 43)[::-1], False, "f32", "subset", CAPS["gather_subset"](cus)))      # L no multiple of the group
    xs = {}
    for L, T, tracks, transpose, dst, kernel, cap in cases:
        if (L, T) not in xs:
            x = gather_values(rng, src, (N, L, T))
            xs[(L, T)] = (x, torch.as_tensor(x, device=dev))
        x, xd = xs[(L, T)]
        B = past(cap)
        assert B > 2 * cap
        if kernel == "wide":
            assert B * (L // group) > 2 * CAPS["gather_wide"](cus)
        rows = rng.integers(0, N, B)
        rows[:2] = [0, N - 1]
        assert (rows[:cap] != rows[cap:2 * cap]).mean() > 0.9
        which = gather_and_compare(x, xd, rows, tracks, dst, transpose)
        assert which == kernel, (L, T, transpose, dst, which)
        seen[which] = seen.get(which, 0) + 1
    assert set(seen) == {"rows", "subset", "wide", "transpose", "transpose_all"}


@pytest.mark.parametrize("src", ["i16", "f32", "f64"])
def test_gather_block_kernel_past_its_grid_in_y_and_in_x(cus, src):
    """gather_block_kernel: more than two passes of 65 535 bins in y (bins of 32 values), and bins of more than two passes of the
    64 chunks in x (135 000 four-value vectors per bin)."""
    import torch
    rng = np.random.default_rng(10 + _NP[src]().itemsize)
    dev = torch.device("cuda:0")
    cap_y, cap_x = CAPS["gather_block_y"](cus), CAPS["gather_block_x"](cus)
    for N, L, T, B in ((50, 4, 8, past(cap_y)), (4, 300, 1800, 3)):
        x = gather_values(rng, src, (N, L, T))
        rows = rng.integers(0, N, B)
        if B == 3:
            rows[:] = [N - 1, 0, 2]
            assert L * T // 4 > 2 * cap_x and (L * T // 4) % 1024 != 0
        else:
            assert B > 2 * cap_y and (rows[:cap_y] != rows[cap_y:2 * cap_y]).mean() > 0.9
        xd = torch.as_tensor(x, device=dev)
        for dst in ("f32", "bf16"):
            assert gather_and_compare(x, xd, rows, None, dst, False) == "block"


# ---- 5. dig_mutation_contexts: runs that span many waves -----------------------------------------------------------------------------
LONG_RUNS = [63, 64, 65, 127, 128, 129, 200, 4095, 4096, 4097, 8300]
VARIANTS = ["all match", "first", "last of the first wave", "middle wave", "last", "before the head"]


def long_run_rows(seqs, rng):
    """Rows in group order (chr1, then chr2): every length of LONG_RUNS in every variant of VARIANTS, at a START whose windows are
    ACGT, between short runs of 1 ... 49 rows anywhere on the chromosome (N runs, other letters, chromosome ends; a fifth of their
    REFs wrong).  Returns (chrom name per row, starts, refs, a list of (first row, length, variant) of the long runs)."""
    plan = [(n, v) for n in LONG_RUNS for v in VARIANTS]
    plan = [plan[i] for i in rng.permutation(len(plan))]
    names = ["chr1", "chr2"]
    chrom, starts, refs, runs = [], [], [], []

    def other_letter(base):
        return "ACGT"[("ACGT".index(base) + int(rng.integers(1, 4))) % 4]

    for j, (n, variant) in enumerate(plan):
        c = names[j >= len(plan) // 2]
        seq = seqs[c].upper()
        for q in range(int(rng.integers(1, 6))):                            # the short runs in front
            while True:
                s = int(rng.choice([rng.integers(3, len(seq)), rng.integers(3, 12), rng.integers(len(seq) - 10, len(seq))], p=[0.9, 0.05, 0.05]))
                if not starts or s != starts[-1]:
                    break
            for _ in range(int(rng.integers(1, 50))):
                base = seq[s]
                chrom.append(c), starts.append(s)
                refs.append(base if rng.random() < 0.8 or base not in "ACGT" else other_letter(base))
        while True:                                                         # the long run: a START whose windows hold ACGT only
            s = int(rng.integers(10, len(seq) - 10))
            if set(seq[s - 3:s + 2]) <= set("ACGT") and s != starts[-1]:
                break
        prev = seq[starts[-1]]
        if prev in "ACGT":                                                  # the row in front of the head: wrong or right by the variant
            refs[-1] = other_letter(prev) if variant == "before the head" else prev
        elif variant == "before the head":
            refs[-1] = "A"                                                  # (an N or another letter in the genome: 'A' does not match it)
        first = len(starts)
        k = {"all match": None, "before the head": None, "first": 0, "last of the first wave": min(first | 63, first + n - 1) - first,
             "middle wave": n // 2, "last": n - 1}[variant]
        for i in range(n):
            chrom.append(c), starts.append(s)
            refs.append(other_letter(seq[s]) if i == k else seq[s])
        runs.append((first, n, variant))
    return np.array(chrom, dtype=object), np.array(starts, np.int64), np.array(refs, dtype=object), runs


def run_rule_statuses(seqs, chrom, starts, refs):
    """The run rule on its own: a row that does not match is a mismatch; one that matches is dropped when a row of its run in front
    of it did not match; every other row is kept (True in the third array: by the device, or by the host for a window it cannot
    read).  Returns (mismatch, dropped, kept)."""
    n = len(starts)
    mismatch, dropped = np.zeros(n, bool), np.zeros(n, bool)
    run_bad = False
    for i in range(n):
        if i == 0 or chrom[i] != chrom[i - 1] or starts[i] != starts[i - 1]:
            run_bad = False
        match = seqs[chrom[i]][starts[i]].upper() == refs[i]
        mismatch[i], dropped[i] = not match, match and run_bad
        run_bad |= not match
    return mismatch, dropped, ~(mismatch | dropped)


@pytest.fixture(scope="module")
def long_runs():
    from digdriver_amd.data_tools.genome import PackedGenome
    from test_gpu_mutation_context import _fuzz_genome
    rng = np.random.default_rng(17)
    seqs = _fuzz_genome(rng)
    chrom, starts, refs, runs = long_run_rows(seqs, rng)
    return dict(seqs=seqs, g=PackedGenome.from_sequences(seqs), chrom=chrom, starts=starts, refs=refs, runs=runs)


@pytest.mark.parametrize("n_up,n_down,collapse", [(1, 1, False), (3, 1, True)])
def test_mutation_context_runs_that_span_many_waves(cus, long_runs, n_up, n_down, collapse):
    """mutctx_resolve_kernel's look-back over wave_last: runs of up to 8 300 rows (130 waves: three steps of 64 waves, head-less
    waves between the head and the last wave), a mismatch in the first row, at the end of the head's wave, in a middle wave, in
    the last row, and in the row in front of the head, which belongs to the run before and must not leak."""
    from digdriver_amd import engine
    from digdriver_amd.sequence_model import sequence_tools as st
    from test_mutation_context_host import rule3
    f = long_runs
    seqs, chrom, starts, refs, runs = f["seqs"], f["chrom"], f["starts"], f["refs"], f["runs"]
    n = len(starts)
    assert n > 60000 and sorted(set((r[1], r[2]) for r in runs)) == sorted((a, v) for a in LONG_RUNS for v in VARIANTS)
    assert len({first % 64 for first, _, _ in runs}) > 32                  # the long runs start at varied lanes
    mismatch, dropped, kept = run_rule_statuses(seqs, chrom, starts, refs)
    # from the rule alone: all three outcomes inside the long runs, and in front of and behind wave 64 of the 8 300-row runs
    inside = np.zeros(n, bool)
    early, late = np.zeros(n, bool), np.zeros(n, bool)
    for first, length, variant in runs:
        inside[first:first + length] = True
        if length == 8300:
            early[first:first + 64 * 64], late[first + 64 * 64:first + length] = True, True
        if variant in ("all match", "before the head"):
            assert kept[first:first + length].all() and (mismatch[first - 1] or variant == "all match")
    for where in (inside, early, late):
        assert mismatch[where].any() and dropped[where].any() and kept[where].any()
    want = []
    for c in ("chr1", "chr2"):
        sel = chrom == c
        want += rule3(seqs[c], starts[sel].tolist(), refs[sel].tolist(), n_up, n_down, collapse)
    want = np.array(want, dtype=object)
    assert ((want != "") <= kept).all() and (want[inside & kept] != "").all()
    status, got = st._row_contexts(f["g"], chrom, starts, refs, n_up, n_down, collapse, True)
    assert np.array_equal(status == engine.MC_MISMATCH, mismatch) and np.array_equal(status == engine.MC_DROPPED, dropped)
    assert np.array_equal((status == engine.MC_KEPT) | (status == engine.MC_HOST), kept) and (status[inside & kept] == engine.MC_KEPT).all()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, bad[:5], got[bad[:5]], want[bad[:5]])
    s_h, c_h = engine.mutation_contexts(f["g"], chrom, starts, refs, n_up, n_down, collapse, on_device=False)
    s_d, c_d = engine.mutation_contexts(f["g"], chrom, starts, refs, n_up, n_down, collapse, on_device=True)
    assert np.array_equal(s_h, s_d.cpu().numpy()) and np.array_equal(s_h, status) and np.array_equal(c_h, c_d.cpu().numpy().view(np.uint32))
