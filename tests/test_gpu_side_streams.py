"""Every public route of engine.py and nb_model on a side stream while the default stream is busy.

On the null stream a kernel, memset, copy or host wait issued on the wrong queue still gives the right answer, and the suite's
calls almost all run there.  tests/guarded_arena.py now runs every guarded device entry point a fourth time on a side stream; this
file does the same one level up, where the package mixes kernels that take a stream argument with torch operations that take the
current stream, through the same helper (guarded_arena.side_stream_call):

    the reference is the same call on the default stream, compared bit for bit;
    a delay (torch.cuda._sleep, calibrated once per process) is enqueued on the default stream;
    the route runs on the side stream; the side stream alone is synchronised; the results are read with copies issued on it (R1);
    the default stream must still be busy then -- otherwise the case FAILS as inconclusive;
    the device is synchronised and the results are read again (R2).

R1 catches a producer left on the default stream (the outputs of the reference run are overwritten before the side run, so a
result that was not produced holds poison or another block's contents, never the right values), R2 a memset or copy left there,
the busy check a wait for the default stream or the device.

  1  the helper's teeth on the GPU: three stand-in "entry points" built from torch operations, each reported under its name
  2  current-stream form: every route inside torch.cuda.stream(side)
  3  explicit-stream form: the plans with stream=side while the busy default stream is current
  4  two calls at once on two side streams: the workspace cache holds one buffer per stream
"""
import contextlib
import functools

import numpy as np
import pytest

import guarded_arena as GA
from guarded_arena import SideStreamViolation, guarded_runs, inp, out, side_stream_call

pytestmark = pytest.mark.gpu

E33 = 33


@pytest.fixture(scope="module")
def dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# =====================================================================================================================================
# 1  stand-ins: no library code and no wrong kernel, only torch operations issued where a defective entry point would issue its own
# =====================================================================================================================================
N = 4096


def _stand_in_bufs():
    rng = np.random.default_rng(3)
    return {"x": inp("f64", rng.uniform(1.0, 2.0, N)), "y": out("f64", N), "n": out("i32", 3)}


def _correct(a):
    a.window("n").zero_()
    a.window("y").copy_(a.window("x") * 2.0 + 1.0)
    a.window("n").add_(7)


def _producer_on_the_default_stream(a):
    import torch
    a.window("n").zero_()
    with torch.cuda.stream(torch.cuda.default_stream()):
        a.window("y").copy_(a.window("x") * 2.0 + 1.0)
    a.window("n").add_(7)


def _zeroing_on_the_default_stream(a):
    import torch
    with torch.cuda.stream(torch.cuda.default_stream()):
        a.window("y").zero_()                                     # (what a hipMemsetAsync on the wrong queue does: it runs late)
    a.window("n").zero_()
    a.window("y").copy_(a.window("x") * 2.0 + 1.0)
    a.window("n").add_(7)


def _waits_for_the_default_stream(a):
    import torch
    torch.cuda.default_stream().synchronize()
    _correct(a)


def test_a_correct_stand_in_passes_its_side_stream_run(dev):
    before = GA.SIDE["runs"]
    got = guarded_runs(_stand_in_bufs(), _correct, device=dev, what="correct stand-in", plain=True)
    assert GA.SIDE["runs"] == before + 1 and len(GA.SIDE["streams"]) >= 1
    assert GA.SIDE["cycles_per_ms"] or GA.SIDE["muls_per_ms"]
    assert np.array_equal(got["n"], [7, 7, 7]) and np.array_equal(got["y"], _stand_in_bufs()["x"].data * 2.0 + 1.0)


def test_a_producer_on_the_default_stream_is_a_late_producer(dev):
    """Also the proof that side and default stream are not implicitly ordered here: the side stream's synchronisation returned
    while the producer, behind the delay on the default stream, had not run -- `y` still held its poison."""
    with pytest.raises(SideStreamViolation, match=r"stand-in \(side stream\): late producer: output `y` .* reading R1 .* element 0$"):
        guarded_runs(_stand_in_bufs(), _producer_on_the_default_stream, device=dev, what="stand-in", plain=True)


def test_a_zeroing_on_the_default_stream_is_a_late_clobber(dev):
    with pytest.raises(SideStreamViolation, match=r"stand-in \(side stream\): late clobber: output `y` .* reading R2 .* element 0$"):
        guarded_runs(_stand_in_bufs(), _zeroing_on_the_default_stream, device=dev, what="stand-in", plain=True)


def test_a_wait_for_the_default_stream_is_inconclusive_and_fails(dev):
    with pytest.raises(SideStreamViolation, match=r"stand-in \(side stream\): inconclusive: the default stream was idle"):
        guarded_runs(_stand_in_bufs(), _waits_for_the_default_stream, device=dev, what="stand-in", plain=True)


def test_the_same_three_through_the_route_helper(dev):
    """side_stream_call, both forms, on stand-in routes that return fresh tensors."""
    import torch
    x = torch.arange(float(N), dtype=torch.float64, device=dev)
    on = lambda s: torch.cuda.stream(s) if s is not None else contextlib.nullcontext()

    def correct(stream):
        with on(stream):
            return {"y": x * 2.0 + 1.0}

    def producer_elsewhere(stream):
        with torch.cuda.stream(torch.cuda.default_stream()):
            return {"y": x * 2.0 + 1.0}

    def clobber_elsewhere(stream):
        with on(stream):
            y = torch.empty_like(x)
        with torch.cuda.stream(torch.cuda.default_stream()):
            y.zero_()
        with on(stream):
            y.copy_(x * 2.0 + 1.0)
        return {"y": y}

    def waits(stream):
        torch.cuda.synchronize()
        return correct(stream)

    mid = torch.empty_like(x)                                     # what a plan keeps between its kernels: it outlives the call

    def intermediate_elsewhere(stream):
        with torch.cuda.stream(torch.cuda.default_stream()):
            mid.copy_(x * 2.0)                                    # (a plan's copy_ left on the current stream)
        with on(stream):
            return {"y": mid + 1.0}

    for explicit in (False, True):
        ref = side_stream_call(correct, dev, "stand-in route", explicit=explicit)
        assert np.array_equal(ref["y"], np.arange(float(N)) * 2.0 + 1.0)
        for fn, name in ((producer_elsewhere, "late producer"), (clobber_elsewhere, "late clobber"), (waits, "inconclusive")):
            with pytest.raises(SideStreamViolation, match=r"stand-in route \(%s\): %s" % ("stream=side" if explicit else "side stream current", name)):
                side_stream_call(fn, dev, "stand-in route", explicit=explicit)
        # an intermediate that persists holds the reference run's equal values and hides its late producer, unless it is named as scratch
        side_stream_call(intermediate_elsewhere, dev, "stand-in plan", explicit=explicit)
        with pytest.raises(SideStreamViolation, match=r"stand-in plan \(.*\): late producer: output `y`"):
            side_stream_call(intermediate_elsewhere, dev, "stand-in plan", explicit=explicit, scratch=[mid])


# =====================================================================================================================================
# inputs: the smallest existing cases, uploaded once on the default stream
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def workload(C, seed=None):
    """make_workload(900, 33, C) as tests/test_gpu_guarded_calls.py builds it: (host arrays, the same as device tensors)."""
    import torch
    from bench import make_workload
    w = make_workload(n_bins=900, n_elements=E33, n_cohorts=C, seed=11 + C if seed is None else seed)
    return w, {k: torch.as_tensor(v, device="cuda:0") for k, v in w.items() if isinstance(v, np.ndarray)}


_TABLES = ("bin_mu", "bin_std", "bin_y", "bin_flag", "bin_ctx", "ov_ptr", "ov_idx", "L", "strand_minus", "d_pr")
_OBS = ("obs_snv", "obs_samples", "obs_indel", "cj", "cj_indel")


def _accumulate(t):
    from digdriver_amd import engine
    return engine.accumulate_elements(*[t[k] for k in _TABLES])


def _element_stats(t, acc):
    from digdriver_amd import engine
    return engine.element_stats(acc["MU"], acc["SIGMA"], acc["P"][:, 0, :], acc["P_INDEL"], *[t[k] for k in _OBS])


def _element_pipeline(t, compact=False):
    from digdriver_amd import engine
    return engine.element_pipeline(*[t[k] for k in _TABLES], *[t[k] for k in _OBS], compact=compact)


def _scale_suffstats(t):
    from digdriver_amd import engine
    return engine.scale_suffstats(t["bin_mu"], t["bin_flag"])


@functools.lru_cache(maxsize=None)
def accumulated(C, seed=None):
    """The accumulation of workload(C) from the default stream: the input of the statistics routes."""
    import torch
    acc = _accumulate(workload(C, seed)[1])
    torch.cuda.synchronize()
    return acc


@functools.lru_cache(maxsize=None)
def gene_inputs():
    """G = 33, C = 5 with the inputs of tests/test_gpu_guarded_calls.py test_gene_pipeline, the rates from the device accumulation."""
    import torch
    from bench import make_workload
    from digdriver_amd import engine
    G, C, n_bins = 33, 5, 900
    w = make_workload(n_bins=n_bins, n_elements=G, n_cohorts=C, seed=41, max_blocks=8)
    rng = np.random.default_rng(42)
    L = np.repeat(rng.poisson(6.0, (G, 4, 64)), 3, axis=2).astype(np.int32)
    L[:, :, ::7] += rng.integers(0, 3, (G, 4, 28))
    gene_length = rng.integers(300, 9000, G).astype(np.int32)
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")
    tabs = [up(w[k]) for k in _TABLES[:7]] + [up(L), up(w["strand_minus"]), up(gene_length), up(w["d_pr"])]
    acc = engine.accumulate_elements(*tabs[:9], tabs[10], gene_length=tabs[9])
    torch.cuda.synchronize()
    mu, sigma, P, p_indel = (acc[k].cpu().numpy() for k in ("MU", "SIGMA", "P", "P_INDEL"))
    alpha, theta = mu ** 2 / sigma ** 2, sigma ** 2 / mu * w["cj"][None, :]
    obs5 = np.stack([rng.poisson(alpha * theta * P[:, j] * 1.2) for j in range(4)] + [rng.poisson(alpha * theta * p_indel[:, None] * 0.1)],
                    axis=1).astype(np.int32)
    obs5[::10, 1] += 400
    cls = [obs5[:, 0], obs5[:, 1], obs5[:, 2], obs5[:, 3], obs5[:, 2] + obs5[:, 3], obs5[:, 1] + obs5[:, 2] + obs5[:, 3]]
    n_samp = np.stack([rng.binomial(x, 0.9) for x in cls], axis=1).astype(np.int32)
    t_indel = rng.uniform(0.05, 0.3, C)
    return dict(tabs=tabs, acc=acc, obs=up(obs5), n_samp=up(n_samp), cj=up(w["cj"]), t_indel=up(t_indel), alpha=up(alpha), theta=up(theta))


@functools.lru_cache(maxsize=None)
def tile_problem():
    """The regions, rows and tables of tests/tile_samples_cases.py (C = 3, R = 6; bin size 1: T = 400)."""
    import tile_samples_cases as K
    from digdriver_amd.data_tools.genome import PackedGenome
    from digdriver_amd.sequence_model import nb_model
    mu, sigma = K.mu_sigma()
    return dict(genome=PackedGenome.from_sequences(K.genome_sequences()), st=K.stacked(K.cohort_rows()), mu=mu, sigma=sigma,
                s_prob=np.stack([nb_model._s_prob_table(K.s_prob(c), 1) for c in range(K.C)]), chroms=[str(c) for c in K.IDX[:, 0]],
                starts=K.IDX[:, 1], ends=K.IDX[:, 2], C=K.C, cap=K.CAP, seqs=K.genome_sequences())


BINSIZE = 1


@functools.lru_cache(maxsize=None)
def tile_planes():
    """engine.tiled_nb_model of tile_problem() from the default stream: the input of the routes behind it."""
    import torch
    from digdriver_amd import engine
    P = tile_problem()
    up = lambda x: torch.as_tensor(x, device="cuda:0")
    st = P["st"]
    res = engine.tiled_nb_model(P["genome"], P["chroms"], P["starts"], P["ends"], P["s_prob"], P["mu"], P["sigma"], st["chrom"], up(st["start"]),
                                up(st["end"]), up(st["cohort"]), binsize=BINSIZE)
    torch.cuda.synchronize()
    return res


def _up(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda:0")


# =====================================================================================================================================
# 2  current-stream form: route name -> builder(tmp) -> fn(stream) (the stream is ignored: the helper makes the side stream current)
# =====================================================================================================================================
ROUTES = {}


def route(fn):
    ROUTES[fn.__name__] = fn
    return fn


# ---- the workload routes ---------------------------------------------------------------------------------------------------------
@route
def accumulate_elements(tmp):
    t = workload(37)[1]
    return lambda s: _accumulate(t)


@route
def element_stats(tmp):
    t, acc = workload(37)[1], accumulated(37)
    return lambda s: _element_stats(t, acc)


@route
def element_pipeline_general(tmp):
    t = workload(37)[1]
    return lambda s: _element_pipeline(t)


@route
def element_pipeline_compact(tmp):
    """compact="auto" builds a PipelinePlan inside the call: dig_element_pipeline_prepare with its host wait, then the compact form.
    That every such plan did take the compact form is asserted behind the runs (fn.check)."""
    from digdriver_amd import engine
    t = workload(37)[1]
    forms = []

    class Spy(engine.PipelinePlan):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            forms.append(self.compact)

    def fn(s):
        real, engine.PipelinePlan = engine.PipelinePlan, Spy
        try:
            return _element_pipeline(t, compact="auto")
        finally:
            engine.PipelinePlan = real

    def check():
        assert len(forms) >= 3 and all(forms), forms

    fn.check = check
    return fn


@route
def gene_pipeline(tmp):
    from digdriver_amd import engine
    g = gene_inputs()
    return lambda s: engine.gene_pipeline(*g["tabs"], g["obs"], g["n_samp"], g["cj"], g["t_indel"])


@route
def gene_stats(tmp):
    from digdriver_amd import engine
    g = gene_inputs()
    a = g["acc"]
    return lambda s: engine.gene_stats(a["MU"], a["SIGMA"], a["P"], a["P_INDEL"], g["obs"], g["n_samp"], g["cj"], g["t_indel"])


@route
def gene_selection(tmp):
    from digdriver_amd import engine
    g = gene_inputs()
    return lambda s: engine.gene_selection(g["alpha"], g["theta"], g["acc"]["P"], g["obs"])


@route
def scale_suffstats(tmp):
    t = workload(37)[1]
    return lambda s: _scale_suffstats(t)


@route
def gather_bins(tmp):
    """A track subset (the wide kernel), all tracks, and the transposed bf16 form."""
    from digdriver_amd import engine
    rng = np.random.default_rng(4)
    x = _up(rng.integers(-1200, 12000, (50, 100, 64)).astype(np.int16))
    rows, tracks = _up(np.array([0, 49, 25, 0, 49, 1, 48], np.int64)), _up(rng.permutation(64)[:40].astype(np.int32))
    return lambda s: [engine.gather_bins(x, rows, tracks), engine.gather_bins(x, rows), engine.gather_bins(x, rows, tracks, "bf16", True)]


# ---- the counting routes ---------------------------------------------------------------------------------------------------------
@route
def gene_counts(tmp):
    import gene_cohort_cases as K
    import pandas as pd
    from digdriver_amd import engine
    from digdriver_amd.data_tools import tabulate_gpu
    case = K.small_case(tmp)
    rows = [tabulate_gpu.encode_gene_rows(f, pd.Index(K.GENES), c) for c, f in enumerate(case["files"])]
    offsets = np.concatenate([[0], np.cumsum([len(r["sample_names"]) for r in rows])])
    cat = {k: _up(np.concatenate([r[k] for r in rows])) for k in ("gene", "sample", "annot", "cohort")}
    return lambda s: engine.gene_counts(cat["gene"], cat["sample"], cat["annot"], cat["cohort"], offsets, len(K.GENES), case["C"],
                                        K.GENES.index("TP53"), max_muts_per_sample=case["max_muts_per_sample"],
                                        max_muts_per_gene_per_sample=case["max_muts_per_gene_per_sample"])


@route
def panel_counts(tmp):
    import target_cohort_cases as T
    from digdriver_amd import engine
    args, _ = T.kernel_cases()["lanes600"]
    rows = [_up(args[k]) for k in ("label", "sample", "annot", "cohort")]
    return lambda s: engine.panel_counts(*rows, args["sample_offsets"], args["label_mask"], args["P"], skip=args["skip"])


def _window_rows(n, n_samples, n_uid, seed):
    """Rows over the windows of tests/test_gpu_sequence_models.py WINDOWS: chromosomes 1, 2 and one the windows do not have."""
    rng = np.random.default_rng(seed)
    chrom = rng.choice([1, 1, 2, 3], n).astype(np.int64)
    start = rng.integers(0, 1100, n).astype(np.int64)
    return chrom, start, start + rng.integers(1, 4, n), rng.integers(0, n_samples, n).astype(np.int32), rng.integers(0, n_uid, n).astype(np.int32)


WINDOWS = np.array([(1, 0, 100), (1, 100, 200), (1, 150, 260), (1, 400, 500), (1, 400, 500), (2, 0, 1000)], np.int64)


@route
def window_objectives(tmp):
    from digdriver_amd import engine
    chrom, start, end, sample, uid = _window_rows(700, 12, 50, 6)
    indel = (np.arange(700) % 5 == 0).astype(np.uint8)
    cols = [_up(x) for x in (chrom, start, end, sample, uid, indel)]
    keep = lambda hits: (np.arange(12) % 4 != 1).astype(np.uint8)
    return lambda s: engine.window_objectives(WINDOWS[:, 0], WINDOWS[:, 1], WINDOWS[:, 2], *cols, [0, 4, 8, 12], 50, keep_from_hits=keep)


@route
def sequence_counts(tmp):
    from digdriver_amd import engine
    chrom, start, _, cohort, typ = _window_rows(1100, 3, 97, 7)                    # (type 96 = K: a label pair the table does not hold)
    cols = [_up(x) for x in (chrom, start, start + 1, typ, cohort)]
    return lambda s: engine.sequence_counts(WINDOWS[:, 0], WINDOWS[:, 1], WINDOWS[:, 2], *cols, 96, 3)


@route
def site_counts(tmp):
    import sites_cohort_cases as K
    from digdriver_amd import engine
    args, _, _ = K.encoded(*K.write_files(tmp))
    arrays, (off, E, C) = [_up(a) for a in args[:9]], args[9:]
    return lambda s: engine.site_counts(*arrays, off, E, C)


@route
def overlap_join(tmp):
    import overlap_join_cases as K
    from digdriver_amd import engine
    from digdriver_amd._marshal import device_backend
    _, start_key, runmax_key, end_eff = engine.join_blocks(*K.block_table())
    be = device_backend("cuda:0")
    table, muts = [_up(x) for x in (start_key, runmax_key, end_eff)], [_up(x) for x in K.mutation_rows()]
    return lambda s: engine.overlap_join(be, *table, *muts)


# ---- the context routes ----------------------------------------------------------------------------------------------------------
def _count_contexts(**kw):
    from digdriver_amd import engine
    P = tile_problem()
    minus = (np.arange(len(P["chroms"])) % 2).astype(np.uint8)
    return lambda s: engine.count_contexts(P["genome"], P["chroms"], P["starts"], P["ends"], minus, device=0, **kw)


@route
def count_contexts_2bit(tmp):
    return _count_contexts()


@route
def count_contexts_4bit(tmp):
    return _count_contexts(form="4bit")


@route
def count_contexts_penta(tmp):
    return _count_contexts(n_up=2, n_down=2)


@route
def mutation_contexts(tmp):
    from digdriver_amd import engine
    P = tile_problem()
    rng = np.random.default_rng(9)
    n = 64 * 5 + 3
    chrom = np.sort(rng.choice(["1", "2"], n))
    start = np.array([rng.integers(0, len(P["seqs"][c])) for c in chrom], np.int64)
    start[10:160][chrom[10:160] == chrom[10]] = start[10]                       # a run of one (chromosome, START) longer than two waves
    letters = [P["seqs"][c][s].upper() for c, s in zip(chrom, start)]
    refs = [b if (b in "ACGT" and rng.random() < 0.85) else "ACGT"[int(rng.integers(0, 4))] for b in letters]
    return lambda s: engine.mutation_contexts(P["genome"], chrom, start, refs, 2, 2)


@functools.lru_cache(maxsize=None)
def _gene_pairs():
    """The genes of tests/test_gpu_guarded_calls.py gene_case and SNVs on the first and the last CDS base of each."""
    import mutfunc_statement as S
    from test_gpu_guarded_calls import gene_case
    seqs, g, genes, gch, stated = gene_case()
    rng = np.random.default_rng(23)
    rows = []
    for gi, x in enumerate(stated):
        cds = S.cds_positions(x)
        for p in (cds[0], cds[-1], cds[len(cds) // 2]):
            rows.append((gi, p, p, 0, int(rng.integers(0, 4)), int(rng.integers(0, 4))))
        rows.append((gi, cds[len(cds) // 2], cds[len(cds) // 2] + 1, 1, 0, 0))        # an insertion inside the CDS
    cols = list(zip(*rows))
    dts = (np.int32, np.int64, np.int64, np.uint8, np.uint8, np.uint8)
    return g, genes, gch, [np.array(c, dt) for c, dt in zip(cols, dts)]


@route
def mutation_function(tmp):
    from digdriver_amd import engine
    g, genes, gch, pairs = _gene_pairs()
    dev_pairs = [_up(p) for p in pairs]
    return lambda s: engine.mutation_function(g, genes, gch, *dev_pairs)


@route
def gene_site_counts(tmp):
    """(returns host arrays: the route waits for its own stream, which must be the side stream alone)"""
    from digdriver_amd import engine
    g, genes, gch, _ = _gene_pairs()
    return lambda s: engine.gene_site_counts(g, genes, gch, on_device=True, return_status=True)


@route
def element_context_counts(tmp):
    from digdriver_amd import engine
    P = tile_problem()
    g = P["genome"]
    chrom, minus = ["1", "2", "1", "2"], np.array([0, 1, 1, 0], np.uint8)
    ptr = np.array([0, 2, 3, 6, 6], np.int64)                                    # (the last element has no block)
    start = np.array([0, 500, 100, 1000, 1200, 1990], np.int64)
    end = np.array([300, 900, 900, 1100, 1700, 2000], np.int64)
    d = [_up(x) for x in (g.chrom_index(chrom), minus, ptr, start, end)]
    return lambda s: [engine.element_context_counts(g, *d), engine.element_context_counts(g, chrom, minus, ptr, start, end, on_device=True)]


# ---- the tile routes -------------------------------------------------------------------------------------------------------------
@route
def base_tile_probs(tmp):
    from digdriver_amd import engine
    P = tile_problem()
    return lambda s: engine.base_tile_probs(P["genome"], P["chroms"], P["starts"], P["ends"], P["s_prob"], BINSIZE)


def _rows_on_device():
    st = tile_problem()["st"]
    return st["chrom"], _up(st["start"]), _up(st["end"]), _up(st["cohort"])


@route
def tile_mut_counts(tmp):
    from digdriver_amd import engine
    P, base, rows = tile_problem(), tile_planes(), _rows_on_device()
    T = base["pt"].shape[2]
    return lambda s: engine.tile_mut_counts(P["genome"], P["chroms"], P["starts"], P["ends"], base["first_pos"], base["n_valid"], *rows, P["C"],
                                            BINSIZE, T)


@route
def tile_sample_counts(tmp):
    from digdriver_amd import engine
    P, base, rows = tile_problem(), tile_planes(), _rows_on_device()
    st = P["st"]
    sample, keep = _up(st["sample"]), _up((np.arange(int(st["sample_offsets"][-1])) % 7 != 3).astype(np.uint8))
    T = base["pt"].shape[2]
    return lambda s: engine.tile_sample_counts(P["genome"], P["chroms"], P["starts"], P["ends"], base["first_pos"], base["n_valid"], *rows, sample,
                                               st["sample_offsets"], keep, P["cap"], P["C"], BINSIZE, T)


@route
def tiled_nb_model(tmp):
    from digdriver_amd import engine
    P, rows = tile_problem(), _rows_on_device()
    return lambda s: engine.tiled_nb_model(P["genome"], P["chroms"], P["starts"], P["ends"], P["s_prob"], P["mu"], P["sigma"], *rows, binsize=BINSIZE)


@route
def tiled_nb_model_by_sample(tmp):
    from digdriver_amd import engine
    P, rows = tile_problem(), _rows_on_device()
    st = P["st"]
    sample = _up(st["sample"])
    return lambda s: engine.tiled_nb_model(P["genome"], P["chroms"], P["starts"], P["ends"], P["s_prob"], P["mu"], P["sigma"], *rows, binsize=BINSIZE,
                                           mut_sample=sample, sample_offsets=st["sample_offsets"], cap=P["cap"], by_sample=True)


def _sparse_problem():
    import sparse_tiles_cases as SP
    C = 4
    tables = [SP.s_prob(c, 1) for c in range(C)]
    s_prob = np.array([[t[k] for k in sorted(tables[0])] for t in tables])
    mu, sigma = SP.mu_sigma(C)
    st = SP.stacked(SP.cohort_rows(C))
    return tile_problem()["genome"], [str(c) for c in SP.IDX[:, 0]], SP.IDX[:, 1], SP.IDX[:, 2], s_prob, mu, sigma, st


@route
def tile_census(tmp):
    from digdriver_amd import engine
    g, chroms, rs, re_, s_prob, _, _, _ = _sparse_problem()
    return lambda s: engine.tile_census(g, chroms, rs, re_, s_prob, 7)


@route
def sparse_tile_test(tmp):
    import torch
    from digdriver_amd import engine
    g, chroms, rs, re_, s_prob, mu, sigma, st = _sparse_problem()
    first, nval, denom, _ = engine.tile_census(g, chroms, rs, re_, s_prob, 7)
    torch.cuda.synchronize()
    T = int(max(1, -(-int((re_ - rs).max()) // 7)))
    rows = (st["chrom"], _up(st["start"]), _up(st["end"]), _up(st["cohort"]))
    return lambda s: engine.sparse_tile_test(g, chroms, rs, re_, s_prob, 7, T, first, nval, denom, mu, sigma, *rows)


@route
def tile_select(tmp):
    from digdriver_amd import engine
    base = tile_planes()
    return lambda s: [engine.tile_select(base["pval"], base["n_valid"], [0.05, 0.5, 0.01], pt=base["pt"], exp=base["exp"], k=base["k"]),
                      engine.tile_select(base["pval"], base["n_valid"], 0.2, index=False)]


@route
def tile_window_test(tmp):
    from digdriver_amd import engine
    P, base = tile_problem(), tile_planes()
    return lambda s: [engine.tile_window_test(base["pt"], base["k"], P["mu"], P["sigma"], base["n_valid"], w) for w in (3, 150)]


@route
def tile_window_test_rows_longer_than_a_chunk(tmp):
    """The long rows of tests/tile_windows_cases.py (T = 10 000: a row is cut into chunks of 1 024 tiles with a halo), widths 7 and
    1 024, behind the dense route on the same genome."""
    import torch
    import tile_windows_cases as W
    from digdriver_amd import engine
    from digdriver_amd.data_tools.genome import PackedGenome
    from digdriver_amd.sequence_model import nb_model
    g = PackedGenome.from_sequences(W.long_genome_sequences())
    rows = W.long_rows()
    s_prob = np.stack([nb_model._s_prob_table(W.long_s_prob(c), 1) for c in range(W.LONG_C)])
    mu, sigma = W.long_mu_sigma()
    chrom = np.concatenate([r[0] for r in rows])
    start, end = _up(np.concatenate([r[1] for r in rows])), _up(np.concatenate([r[2] for r in rows]))
    cohort = _up(np.concatenate([np.full(len(r[1]), c, np.int32) for c, r in enumerate(rows)]))
    base = engine.tiled_nb_model(g, [str(c) for c in W.LONG_IDX[:, 0]], W.LONG_IDX[:, 1], W.LONG_IDX[:, 2], s_prob, mu, sigma, chrom, start, end,
                                 cohort, binsize=1)
    torch.cuda.synchronize()
    assert base["pt"].shape[2] == W.LONG_T > W.CHUNK
    return lambda s: [engine.tile_window_test(base["pt"], base["k"], mu, sigma, base["n_valid"], w) for w in W.LONG_WIDTHS]


# ---- sort and q-values -----------------------------------------------------------------------------------------------------------
def _bh_ragged(case, lookup):
    """Which form dig_bh_qvalues_ragged takes follows from the rows (tests/test_gpu_guarded_calls.py _records_and_capacity: the records
    of a row's reverse running minimum against the entries its table holds): asserted, so that a changed rule cannot turn both
    routes into one path unnoticed."""
    from digdriver_amd.sequence_model import nb_model
    from test_gpu_guarded_calls import _records_and_capacity
    rows, rp, p = case()
    fit = _records_and_capacity(rows, rp)
    if lookup:
        assert all(rec == 0 or rec + 2 <= cap for rec, cap in fit), "every row must stay in the lookup form"
    else:
        assert not all(rec <= cap for rec, cap in fit), "a row must hold more records than its table: the payload fallback"
    p_dev = _up(p)
    return lambda s: nb_model.bh_ragged(p_dev, rp, want_q=True, want_row_min=True)


@route
def bh_ragged_lookup_form(tmp):
    from test_gpu_guarded_calls import lookup_rows_case
    return _bh_ragged(lookup_rows_case, True)


@route
def bh_ragged_payload_fallback(tmp):
    from test_gpu_guarded_calls import sort_rows_case
    return _bh_ragged(sort_rows_case, False)


@route
def get_q_vals_rows(tmp):
    from digdriver_amd.sequence_model import nb_model
    rng = np.random.default_rng(12)
    p = _up(np.stack([rng.random(4097), rng.random(4097) ** 4, np.minimum(1.0, rng.exponential(0.05, 4097))]))
    return lambda s: nb_model.get_q_vals_rows(p)


@pytest.mark.parametrize("name", sorted(ROUTES))
def test_route_inside_a_side_stream(dev, name, tmp_path):
    import torch
    fn = ROUTES[name](tmp_path)
    torch.cuda.synchronize()
    ref = side_stream_call(fn, dev, name)
    assert sum(v.size for v in ref.values()) > 0
    getattr(fn, "check", lambda: None)()


# =====================================================================================================================================
# 3  explicit-stream form: the busy default stream is current, stream=side is passed
# =====================================================================================================================================
def _plan(C, **kw):
    from digdriver_amd import engine
    t = workload(C)[1]
    return engine.PipelinePlan(*[t[k] for k in _TABLES], *[t[k] for k in _OBS[:3]], **kw), t


def _plan_scratch(plan):
    """What a PipelinePlan keeps between its kernels and calls, for side_stream_call to overwrite between the reference and the side
    run: its workspace (what the contexts and dot stages leave for the next stage) and the record-major outputs unpack() reads.  A
    compact plan also keeps, from construction on, its [E, 64] copy of L and the repetition flag in the workspace: `restore` runs
    dig_element_pipeline_prepare again, as the constructor does, on the poisoned workspace."""
    import ctypes
    from digdriver_amd import _lib
    scratch = [plan.ws] + ([plan.out_records] if plan.records_out else [])

    def restore():
        if plan.compact:
            ok = ctypes.c_int(0)
            _lib.call("dig_element_pipeline_prepare", _lib.dev_ptr(plan.keep[7]), plan.E, plan.C, plan._ws, plan.wsb, ctypes.byref(ok), _lib.stream_ptr())
            assert ok.value == 1

    return dict(scratch=scratch, restore=restore)


@pytest.mark.parametrize("form", ["general", "compact", "records_out"])
@pytest.mark.parametrize("C", [5, 37])
def test_pipeline_plan_run_with_an_explicit_stream(dev, C, form):
    """PipelinePlan.run(stream=side); records_out followed by unpack(stream=side).  The plan's outputs, its workspace and its
    record-major outputs persist, so the helper overwrites them after the reference run: the side run has to produce every one of
    them again, on the side stream."""
    import torch
    plan, t = _plan(C, compact=False if form == "general" else "auto", records_out=form == "records_out")
    assert plan.compact == (form != "general")
    torch.cuda.synchronize()

    def fn(stream):
        res = plan.run(t["cj"], t["cj_indel"], stream=stream)
        return plan.unpack(stream=stream) if form == "records_out" else res

    side_stream_call(fn, dev, "PipelinePlan.run %s C=%d" % (form, C), explicit=True, **_plan_scratch(plan))


@pytest.mark.parametrize("compact", [False, "auto"], ids=["general", "compact"])
def test_pipeline_plan_stage_by_stage_with_an_explicit_stream(dev, compact):
    """stages = 1, 2, then 4 | 8 (DIG_PIPE_WORKLIST_CLEAN) in three calls on stream=side: the bits of the one-call run.  What stages
    1 and 2 leave for stage 4 lives in the plan's workspace, which is overwritten between the runs (_plan_scratch): a stage 1 or 2
    kernel on another queue would leave stage 4 with poison."""
    import torch
    from digdriver_amd import _lib
    plan, t = _plan(37, compact=compact)
    whole = [GA._host_copy(torch, x) for x in plan.run(t["cj"], t["cj_indel"])]
    torch.cuda.synchronize()

    def fn(stream):
        plan.run(t["cj"], t["cj_indel"], stages=_lib.DIG_PIPE_CONTEXTS, stream=stream)
        plan.run(t["cj"], t["cj_indel"], stages=_lib.DIG_PIPE_DOT, stream=stream)
        return plan.run(t["cj"], t["cj_indel"], stages=_lib.DIG_PIPE_STATISTICS | _lib.DIG_PIPE_WORKLIST_CLEAN, stream=stream)

    ref = side_stream_call(fn, dev, "PipelinePlan.run in three stages", explicit=True, **_plan_scratch(plan))
    one = GA._flatten(whole, "", {})
    assert set(one) == set(ref) and all(GA.same_bits(one[k], ref[k]) for k in one)


@pytest.mark.parametrize("C", [5, 300])
def test_scale_factor_plan_with_an_explicit_stream(dev, C):
    import torch
    from digdriver_amd import engine
    rng = np.random.default_rng(C)
    mu, flag = _up(rng.gamma(9.0, 3.0, (4097, C))), _up((rng.uniform(size=(4097, C)) < 0.1).astype(np.uint8))
    plan = engine.ScaleFactorPlan(mu, flag, _up(np.rint(rng.uniform(1e3, 1e6, C))), _up(np.rint(rng.uniform(1e2, 1e5, C))))
    outs = [torch.empty(C, dtype=torch.float64, device=dev) for _ in range(3)]

    def fn(stream):
        plan.run(*outs, stream=stream)
        return outs

    side_stream_call(fn, dev, "ScaleFactorPlan.run C=%d" % C, explicit=True, scratch=[plan.ws])


def test_chunked_scale_factor_plan_of_two_ranks_with_an_explicit_stream(dev):
    """world = 2 walked on one device as tests/test_gpu_sharded.py walks it: enqueue_part(stream=side) per rank, the stack of the
    parts (the caller's own torch operation: issued with the stream made current, as the plan's _on does for its copies), then
    finish(stacked, stream=side) per rank, which copies the parts apart through _on."""
    import torch
    from digdriver_amd import engine, parallel
    w = workload(37)[0]
    plans = parallel.plan_shards(w["ov_ptr"], w["ov_idx"], w["bin_mu"].shape[0], 2)
    shards = [parallel.shard_inputs(w, p, 2) for p in plans]
    ranks = [engine.ChunkedScaleFactorPlan(_up(sh["bin_mu"]), _up(sh["bin_flag"]), _up(sh["n_snv_obs"]), _up(sh["n_ind_obs"]), sh["chunk_rows"],
                                           parallel.N_CHUNKS, world=2) for sh in shards]
    outs = [[torch.empty(37, dtype=torch.float64, device=dev) for _ in range(3)] for _ in ranks]
    torch.cuda.synchronize()

    def fn(stream):
        parts = [r.enqueue_part(stream=stream) for r in ranks]
        with ranks[0]._on(stream):
            stacked = torch.stack(parts)
        for r, (cj, cji, total) in zip(ranks, outs):
            r.finish(stacked, cj, cji, out_sum=total, stream=stream)
        return [stacked] + outs

    # what the plans keep between their kernels: the chunk sums of `part` (its last two rows are the observed counts, set when the plan
    # is built), the copies finish() makes of the parts, the workspace -- overwritten between the runs, so that enqueue_part's kernels and
    # finish's copy_ calls have to fill them again on the side stream
    scratch = [x for r in ranks for x in (r.part[:r.n_own], r.sums, r.obs, r.ws)]
    ref = side_stream_call(fn, dev, "ChunkedScaleFactorPlan world=2", explicit=True, scratch=scratch)
    assert GA.same_bits(ref["[1][0]"], ref["[2][0]"]) and GA.same_bits(ref["[1][1]"], ref["[2][1]"])       # every rank: the same factors
    assert np.isfinite(ref["[1][0]"]).all() and (ref["[1][2]"] > 0).all()


@pytest.mark.parametrize("explicit", [False, True], ids=["current", "explicit"])
def test_stage_timer_selftest_on_a_side_stream(dev, explicit):
    """dig_stage_timer_selftest(timer, stream) launches an empty kernel with the timer's events (measurement only, no output): launched on
    the side stream, read_ms() -- which waits for that kernel -- returns while the default stream is still busy."""
    import torch
    from digdriver_amd import engine
    side, = GA.side_streams(torch, dev, 1)
    default = torch.cuda.default_stream(dev)
    tm = engine.StageTimer()
    try:
        tm.selftest()
        assert tm.read_ms() >= 0.0                                                 # (loads the kernel)
        torch.cuda.synchronize()
        with torch.cuda.stream(default):
            GA.enqueue_delay(torch, dev, GA.delay_for(0.0, "StageTimer.selftest"))
        if explicit:
            tm.selftest(stream=side)
        else:
            with torch.cuda.stream(side):
                tm.selftest()
        ms = tm.read_ms()
        still_busy = default.query() is False
        torch.cuda.synchronize()
        assert still_busy, "inconclusive: the empty kernel ran behind the default stream's delay, or read_ms waited for the device"
        assert 0.0 <= ms < GA.MIN_DELAY_MS
    finally:
        tm.close()


# =====================================================================================================================================
# 4  two calls at once: one cached workspace per (kind, device, stream)
# =====================================================================================================================================
TWO_AT_ONCE = {"element_stats": ("element_stats", lambda t, acc: _element_stats(t, acc)),
               "accumulate_elements": ("accumulate", lambda t, acc: _accumulate(t)),
               "element_pipeline": ("pipeline", lambda t, acc: _element_pipeline(t)),
               "scale_suffstats": ("suffstats", lambda t, acc: _scale_suffstats(t))}


@pytest.mark.parametrize("name", sorted(TWO_AT_ONCE))
def test_two_calls_at_once_on_two_side_streams(dev, name):
    """The same one-shot route with DIFFERENT inputs of one shape on two side streams, each stream behind a delay of its own, so
    that both calls are enqueued before either starts (asserted: both streams are still busy then).  Each result must carry the
    bits of its sequential run, and engine._WS_CACHE must hold two distinct tensors under the two stream keys -- that part is
    deterministic.  That the kernels of the two calls really overlap is likely (nothing orders them and each leaves most of the chip
    idle at this size) but cannot be forced, and is not asserted."""
    import time
    import torch
    from digdriver_amd import _lib, engine
    kind, run = TWO_AT_ONCE[name]
    C = 37
    inputs = [(workload(C, seed)[1], accumulated(C, seed)) for seed in (101, 202)]
    assert not torch.equal(inputs[0][0]["bin_mu"], inputs[1][0]["bin_mu"])
    N = inputs[0][0]["bin_mu"].shape[0]
    assert _lib.workspace_bytes(kind, N if kind == "suffstats" else E33, C) > 0, "the route must use a cached workspace at this size"
    streams = GA.side_streams(torch, dev, 2)
    torch.cuda.synchronize()
    want, t0 = [], time.perf_counter()
    for t, acc in inputs:                                                          # one after the other on the default stream
        want.append(GA._flatten(GA._host_copy(torch, run(t, acc)), "", {}))
    torch.cuda.synchronize()
    ms = GA.delay_for((time.perf_counter() - t0) * 1e3, "two calls of " + name)
    got = []
    for s, (t, acc) in zip(streams, inputs):
        with torch.cuda.stream(s):
            GA.enqueue_delay(torch, dev, ms)
    for s, (t, acc) in zip(streams, inputs):
        with torch.cuda.stream(s):
            got.append(run(t, acc))
    both_waiting = [s.query() is False for s in streams]
    host = []
    for s, g in zip(streams, got):
        s.synchronize()
        with torch.cuda.stream(s):
            host.append(GA._flatten(GA._host_copy(torch, g), "", {}))
    torch.cuda.synchronize()
    assert both_waiting == [True, True], "inconclusive: a call was not enqueued behind its stream's delay before the other started"
    for i in (0, 1):
        assert set(host[i]) == set(want[i])
        for k in want[i]:
            assert GA.same_bits(host[i][k], want[i][k]), "call %d of two at once: `%s` differs from its sequential run, first at element %s" % (
                i, k, GA._first_difference(host[i][k], want[i][k]))
    assert any(not GA.same_bits(want[0][k], want[1][k]) for k in want[0])          # (the two calls do compute different things)
    ws = [engine._WS_CACHE.get((kind, dev.index, s.cuda_stream)) for s in streams]
    assert ws[0] is not None and ws[1] is not None and ws[0].data_ptr() != ws[1].data_ptr()
    assert streams[0].cuda_stream != streams[1].cuda_stream
