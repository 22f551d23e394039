"""Every device entry point of include/dig_hip.h called through `_lib.call` with pointers carved from a guarded arena
(tests/guarded_arena.py): each argument at exactly its documented alignment and no more, exact workspace sizes, 64 KiB of typed
in-domain poison on either side of every buffer, twice (poison A / B).  Three results per call: (a) no band touched, (b) outputs
bit-identical between A and B, (c) outputs equal the operation's existing reference within its existing tolerance AND carry the
bits of the same call on ordinary tensors.  The values themselves stay with the oracles of the tests named at each check; new
here is where the pointers sit and what lies around them.  DESIGN.md section 5.3 has the table."""
import ctypes
import functools

import numpy as np
import pytest

import guarded_arena as GA
from conftest import rel_close
from guarded_arena import GuardedArena, guarded_runs, out, ws

pytestmark = pytest.mark.gpu

RTOL = 1e-6                     # tests/test_gpu_parity.py: the tolerance contract for p-values and expected counts


@pytest.fixture(scope="module")
def dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def arr(dtype, data, **kw):
    return GA.inp(dtype, np.ascontiguousarray(data, GA._NP[dtype]), **kw)


# ---- the entry points' argument lists: a name = a pointer carved under that name (absent: NULL), #x a scalar, @ws the workspace
# pointer and its byte count, %x a HOST pointer (numpy array or ctypes object); the stream is appended ---------------------------
_BIN = "bin_mu bin_std bin_y bin_flag bin_ctx ov_ptr ov_idx L"
_ACC_OUT = "MU SIGMA R_OBS FLAG P R_SIZE ELT_SIZE P_INDEL"
_G2 = "words2 #n_words2 nint_start nint_end #n_int nint_bucket #n_buckets chrom_off chrom_len #n_chrom"
_GENES = "gene_chrom gene_minus blk_ptr blk_start blk_end cds_off spl_ptr spl_pos #n_genes"
_SITES = "site_pos site_end site_attr site_elt #S #E row_pos row_end row_attr row_sample row_cohort sample_off #n #C #n_samples"
SIG = {
    "dig_accumulate_elements": _BIN + " #n_class strand_minus gene_length d_pr " + _ACC_OUT + " #N #E #C @ws",
    "dig_element_stats": "mu sigma mu_indel sigma_indel pi_sum pi_indel #per_cohort obs_snv obs_samples obs_indel cj cj_indel out #E #C @ws",
    "dig_element_pipeline": _BIN + " strand_minus gene_length d_pr obs_snv obs_samples obs_indel cj cj_indel " + _ACC_OUT +
                            " out #N #E #C bin_records #stages @ws",
    "dig_element_pipeline_prepare": "L #E #C @ws %compact_ok",
    "dig_bin_records_pack": "bin_mu bin_std bin_y bin_flag #N #C bin_records #records_bytes",
    "dig_element_records_unpack": "out #E #C out7 MU SIGMA R_OBS FLAG #cohort_major",
    "dig_gene_pipeline": _BIN + " strand_minus gene_length d_pr obs n_samp cj t_indel #with_indel " + _ACC_OUT + " out #N #E #C @ws",
    "dig_scale_suffstats": "bin_mu bin_flag #N #C out_sum @ws",
    "dig_scale_factors_local": "bin_mu bin_flag #N #C n_snv_obs n_ind_obs out_sum cj cj_indel @ws",
    "dig_scale_suffstats_chunked": "bin_mu bin_flag #C %chunk_rows #n_chunks out_chunks @ws",
    "dig_scale_factors_chunked": "out_chunks #n_chunks obs #world #C out_sum cj cj_indel",
    "dig_sort_rows": "p %row_ptr #rows p_sorted order @ws",
    "dig_bh_qvalues_ragged": "p %row_ptr #rows %n_global %rank0 %carry q row_min #sorted_out @ws",
    "dig_bh_qvalues_sorted": "p #n #rows q @ws",
    "dig_gather_bins": "x #src #N #L #T rows #B tracks #T_sel out #dst #transpose",
    "dig_count_contexts": "words #n_words chrom_off chrom_len #n_chrom reg_chrom reg_start reg_end reg_minus #R out",
    "dig_count_contexts2": _G2 + " reg_chrom reg_start reg_end reg_minus #R out",
    "dig_count_contexts5": _G2 + " reg_chrom reg_start reg_end reg_minus #R out",
    "dig_mutation_contexts": _G2 + " row_chrom row_start row_ref #n_rows #n_up #n_down #collapse status context @ws",
    "dig_mutation_function": _G2 + " " + _GENES + " pair_gene pair_start pair_end pair_kind pair_ref pair_alt #n_pairs impact status "
                             "n_cds cds_min cds_max",
    "dig_gene_site_counts": _G2 + " " + _GENES + " L n_stop_loss status",
    "dig_base_tile_probs_ctx": "words #n_words chrom_off chrom_len #n_chrom reg_chrom reg_start reg_end #R s_prob #C #n_up #binsize "
                               "#n_tiles pt first_pos n_valid",
    "dig_tile_mut_counts": "pair_mut pair_reg #n_pairs mut_start mut_cohort first_pos n_valid #binsize #n_tiles #R #C k",
    "dig_overlap_join_count": "blk_start_key blk_runmax_key blk_end #n_blk mut_chrom mut_start mut_end #n_mut counts",
    "dig_overlap_join_fill": "blk_start_key blk_runmax_key blk_end #n_blk mut_chrom mut_start mut_end #n_mut offsets pair_mut pair_blk",
    "dig_scale_factors": "parts #world #C cj cj_indel",
    "dig_gene_row_keys": "gene sample annot cohort sample_off #n #G #C #n_samples keys sample_total",
    "dig_window_pair_keys": "pair_row pair_blk #n_pairs blk_window #n_blk row_sample row_uid row_indel #n_rows #n_samples #N #n_uid keys",
    "dig_gene_counts": "keys #n sample_total #n_samples #max_s #max_gs #tp53 #G #C obs n_samp extra n_syn blacklisted scratch",
    "dig_window_sample_hits": "keys #n #n_samples #N #n_uid hits",
    "dig_window_objectives": "keys #n keep sample_off #n_samples #N #C #n_uid labels scratch",
    "dig_sequence_counts": "pair_row #n_pairs row_type row_cohort #n #K #C counts",
    "dig_site_match_count": _SITES + " counts",
    "dig_site_match_keys": _SITES + " offsets #total keys",
    "dig_site_counts": "keys #total #E #C #n_samples obs_snv obs_samples",
    "dig_rbf_cross": "Z X #m #n #d #lengthscale #outputscale K",
    "dig_rbf_backward": "g K #m #n #lengthscale #outputscale W partial",
    "dig_nb_midp_upper": "k alpha p out #n", "dig_nb_exact": "k alpha p out #n", "dig_nb_greater": "k alpha p out #n",
    "dig_nb_midp_twosided": "k alpha p out #n", "dig_fisher": "p1 p2 out #n",
    "dig_normal_params_to_gamma": "mu sigma alpha theta #n",
    "dig_tiled_nb_test": "pt #pt_per_cohort k mu sigma pval exp #C #n_bins #n_tiles",
    "dig_gene_stats": "mu sigma mu_indel sigma_indel pi #n_pi pi_indel #per_cohort obs n_samp cj t_indel #with_indel out #G #C",
    "dig_gene_selection": "alpha theta pi #n_pi obs out #G #C",
}


def call(a, name, alias=None, **scalars):
    """One entry point on the buffers of arena `a` (GuardedArena or PlainBuffers).  alias: argument name -> buffer name."""
    from digdriver_amd import _lib
    alias = alias or {}
    args = []
    for tok in SIG[name].split():
        if tok[0] == "#":
            args.append(scalars[tok[1:]])
        elif tok[0] == "%":
            h = scalars.get(tok[1:])
            args.append(_lib.host_ptr(h) if isinstance(h, np.ndarray) else (None if h is None else ctypes.byref(h)))
        elif tok == "@ws":
            n = alias.get("ws", "ws")
            args += [a.ptr(n), a.bufs[n].nbytes if n in a.bufs else 0]
        else:
            args.append(a.ptr(alias.get(tok, tok)))
    _lib.call(name, *args, _lib.stream_ptr())


def query(name, *args):
    from digdriver_amd import _lib
    return int(getattr(_lib.load(), name)(*args))


def guarded(what, bufs, invoke, dev):
    """Checks (a), (b) and the bit equality with ordinary tensors of (c); returns the outputs for the reference."""
    return guarded_runs(bufs, invoke, device=dev, what=what, plain=True)


def close(got, ref, tol):
    """rel_close, with infinities (an element without bins) in the same places: tests/test_gpu_parity.py
    test_compact_pipeline_against_general_form_and_oracle."""
    fin = ~np.isinf(ref)
    assert np.array_equal(got[~fin], ref[~fin])
    rel_close(got[fin], ref[fin], tol)


# =====================================================================================================================================
# statistics, accumulation, pipeline (dig_nb.hip, dig_accumulate.hip, dig_pipeline.hip)
# E = 33: two 16-row tiles and one row, E * C no multiple of 64; C = 5 quad tail, 37 two tiles + quad + one, 49 two chunks
# =====================================================================================================================================
E33 = 33


@functools.lru_cache(maxsize=None)
def workload(C):
    """make_workload(900, 33, C) as tests/test_gpu_parity.py _accumulate_vs_oracle builds it, with the oracle's accumulation and
    statistics (computed once per cohort count and left unchanged)."""
    from bench import make_workload
    from oracle import dig_oracle as O
    w = make_workload(n_bins=900, n_elements=E33, n_cohorts=C, seed=11 + C)
    acc = O.accumulate_elements(w["bin_mu"], w["bin_std"], w["bin_y"], w["bin_flag"], w["bin_ctx"], w["ov_ptr"], w["ov_idx"], w["L"],
                                w["strand_minus"].astype(bool), w["d_pr"])
    st = O.element_stats(acc["MU"], acc["SIGMA"], acc["P"][:, 0, :], acc["P_INDEL"][:, None], w["obs_snv"], w["obs_samples"],
                         w["obs_indel"], w["cj"][None, :], w["cj_indel"][None, :])
    return w, acc, st


def table_bufs(w, L=None, gene_length=None):
    """The bin tables, the overlap CSR and the element table every accumulation takes."""
    L = w["L"] if L is None else L
    N, nnz = w["bin_mu"].shape[0], len(w["ov_idx"])
    b = dict(bin_mu=arr("f64", w["bin_mu"]), bin_std=arr("f64", w["bin_std"]), bin_y=arr("i32", w["bin_y"], poison=(0, 9)),
             bin_flag=arr("u8", w["bin_flag"]), bin_ctx=arr("i32", w["bin_ctx"], poison=(0, 9)),
             ov_ptr=arr("i64", w["ov_ptr"], index=(0, nnz)), ov_idx=arr("i32", w["ov_idx"], index=(0, N - 1)),
             L=arr("i32", L, poison=(0, 3)), strand_minus=arr("u8", w["strand_minus"]), d_pr=arr("f64", w["d_pr"]))
    if gene_length is not None:
        b["gene_length"] = arr("i32", gene_length, poison=(300, 9000))
    return b


def acc_out_bufs(E, C, n_class=1, rates=True):
    b = {}
    if rates:
        b.update(MU=out("f64", (E, C)), SIGMA=out("f64", (E, C)), R_OBS=out("i32", (E, C)), FLAG=out("i32", (E, C)))
    b.update(P=out("f64", (E, n_class, C)), R_SIZE=out("i32", E), ELT_SIZE=out("i32", E), P_INDEL=out("f64", E))
    return b


def obs_bufs(w):
    return dict(obs_snv=arr("i32", w["obs_snv"], poison=(0, 50)), obs_samples=arr("i32", w["obs_samples"], poison=(0, 50)),
                obs_indel=arr("i32", w["obs_indel"], poison=(0, 50)), cj=arr("f64", w["cj"]), cj_indel=arr("f64", w["cj_indel"]))


def check_accumulation(got, want, p_tol=1e-11, rates=True):
    """The bounds of tests/test_gpu_parity.py _accumulate_vs_oracle."""
    if rates:
        close(got["MU"], want["MU"], 1e-12)
        close(got["SIGMA"], want["SIGMA"], 1e-12)
        assert np.array_equal(got["R_OBS"], want["R_OBS"]) and np.array_equal(got["FLAG"], want["FLAG"])
    close(got["P"], want["P"], p_tol)
    close(got["P_INDEL"], want["P_INDEL"], 1e-15)
    assert np.array_equal(got["R_SIZE"], want["R_SIZE"]) and np.array_equal(got["ELT_SIZE"], want["ELT_SIZE"])


def check_statistics(planes, want):
    """planes [7, E, C] against the oracle's statistics: tests/test_gpu_parity.py test_configs0_chr21_every_element_against_the_oracle."""
    from digdriver_amd import engine
    for j, name in enumerate(engine.ES_PLANES):
        close(planes[j], want[name], RTOL)


_ACC_WS = {}


def accumulate_with_workspace(C, dev):
    if C not in _ACC_WS:
        w, want, _ = workload(C)
        N = w["bin_mu"].shape[0]
        b = {**table_bufs(w), **acc_out_bufs(E33, C), "ws": ws(query("dig_accumulate_workspace", E33, C), align=256)}
        _ACC_WS[C] = guarded("dig_accumulate_elements C=%d" % C, b, lambda a: call(a, "dig_accumulate_elements", n_class=1, N=N, E=E33, C=C), dev)
    return _ACC_WS[C]


@pytest.mark.parametrize("C", [5, 37, 49])
def test_accumulate_elements_with_its_exact_workspace(dev, C):
    check_accumulation(accumulate_with_workspace(C, dev), workload(C)[1])


@pytest.mark.parametrize("C", [5, 37, 49])
def test_accumulate_elements_without_workspace(dev, C):
    """The single-kernel LDS form against the workspace form: 1e-12 and exact integers, tests/test_gpu_parity.py
    _accumulate_vs_oracle."""
    w, want, _ = workload(C)
    b = {**table_bufs(w), **acc_out_bufs(E33, C)}
    got = guarded("dig_accumulate_elements (NULL workspace) C=%d" % C, b,
                  lambda a: call(a, "dig_accumulate_elements", n_class=1, N=w["bin_mu"].shape[0], E=E33, C=C), dev)
    ref = accumulate_with_workspace(C, dev)
    for name in ("MU", "SIGMA", "P", "P_INDEL"):
        close(got[name], ref[name], 1e-12)
    for name in ("R_OBS", "FLAG", "R_SIZE", "ELT_SIZE"):
        assert np.array_equal(got[name], ref[name]), name
    check_accumulation(got, want)


def test_the_arena_names_an_output_declared_one_element_short(dev):
    """Teeth without a modified library: MU of dig_accumulate_elements declared one element shorter than the [E, C] the call
    writes.  Exactly that argument, rear side, offset 0 -- and nothing else: the store stays inside the slab."""
    C = 5
    w, _, _ = workload(C)
    b = {**table_bufs(w), **acc_out_bufs(E33, C), "ws": ws(query("dig_accumulate_workspace", E33, C), align=256)}
    b["MU"] = out("f64", E33 * C - 1)
    for variant in ("A", "B"):
        a = GuardedArena(b, variant, dev)
        call(a, "dig_accumulate_elements", n_class=1, N=w["bin_mu"].shape[0], E=E33, C=C)
        assert a.violations() == [("MU", "rear", 0)]
    with pytest.raises(GA.GuardViolation, match=r"rear band of `MU`, byte offset 0$"):
        guarded_runs(b, lambda a: call(a, "dig_accumulate_elements", n_class=1, N=w["bin_mu"].shape[0], E=E33, C=C), device=dev)


def stats_bufs(C):
    w, acc, _ = workload(C)
    return dict(mu=arr("f64", acc["MU"]), sigma=arr("f64", acc["SIGMA"]), pi_sum=arr("f64", acc["P"][:, 0, :]), pi_indel=arr("f64", acc["P_INDEL"]),
                **obs_bufs(w), out=out("f64", (7, E33, C)))


@pytest.mark.parametrize("C", [5, 37])
def test_element_stats_with_its_exact_workspace(dev, C):
    b = {**stats_bufs(C), "ws": ws(query("dig_element_stats_workspace", E33, C), align=4)}
    got = guarded("dig_element_stats C=%d" % C, b, lambda a: call(a, "dig_element_stats", per_cohort=0, E=E33, C=C), dev)
    check_statistics(got["out"], workload(C)[2])


@pytest.mark.parametrize("C", [5, 37])
def test_element_stats_without_workspace(dev, C):
    got = guarded("dig_element_stats (NULL workspace) C=%d" % C, stats_bufs(C),
                  lambda a: call(a, "dig_element_stats", per_cohort=0, E=E33, C=C), dev)
    check_statistics(got["out"], workload(C)[2])


@pytest.mark.parametrize("C", [5, 37, 49])
def test_element_pipeline_one_shot_general_form(dev, C):
    w, acc, st = workload(C)
    N = w["bin_mu"].shape[0]
    b = {**table_bufs(w), **obs_bufs(w), **acc_out_bufs(E33, C), "out": out("f64", (7, E33, C)),
         "ws": ws(query("dig_element_pipeline_workspace", E33, C), align=256)}
    got = guarded("dig_element_pipeline C=%d" % C, b, lambda a: call(a, "dig_element_pipeline", N=N, E=E33, C=C, stages=7), dev)
    check_accumulation(got, acc)
    check_statistics(got["out"], st)
    # "results are bit-identical to the two separate calls" (include/dig_hip.h): the accumulation of the guarded separate call
    sep = accumulate_with_workspace(C, dev)
    for name in sep:
        assert GA.same_bits(got[name], sep[name]), name


@pytest.mark.parametrize("C", [5, 37, 49])
def test_element_pipeline_one_shot_compact_form(dev, C):
    """dig_element_pipeline_prepare + DIG_PIPE_COMPACT_L on one workspace; P within 1e-11 of the oracle as in
    tests/test_gpu_parity.py test_accumulate_and_compact_pipeline_at_every_cohort_cut."""
    from digdriver_amd import _lib
    w, acc, st = workload(C)
    N = w["bin_mu"].shape[0]
    b = {**table_bufs(w), **obs_bufs(w), **acc_out_bufs(E33, C), "out": out("f64", (7, E33, C)),
         "ws": ws(query("dig_element_pipeline_workspace", E33, C), align=256)}

    def invoke(a):
        ok = ctypes.c_int(0)
        call(a, "dig_element_pipeline_prepare", E=E33, C=C, compact_ok=ok)
        assert ok.value == 1, "make_workload repeats every context count three times"
        call(a, "dig_element_pipeline", N=N, E=E33, C=C, stages=7 | _lib.DIG_PIPE_COMPACT_L)

    got = guarded("compact dig_element_pipeline C=%d" % C, b, invoke, dev)
    check_accumulation(got, acc)
    check_statistics(got["out"], st)


@pytest.mark.parametrize("C", [5, 37, 49])
def test_pipeline_plan_form_with_packed_records_and_record_major_out(dev, C):
    """What engine.PipelinePlan(records_out=True) does, call by call, every buffer at its exact size: prepare, pack the bin
    records, the compact pipeline with record-major `out`, unpack.  MU / SIGMA / R_OBS / FLAG leave through the unpack only."""
    from digdriver_amd import _lib
    w, acc, st = workload(C)
    N = w["bin_mu"].shape[0]
    b = {**table_bufs(w), **obs_bufs(w), **acc_out_bufs(E33, C, rates=False),
         "ws": ws(query("dig_element_pipeline_workspace", E33, C), align=256),
         "bin_records": ws(query("dig_bin_records_bytes", N, C), align=256),
         "out": ws(query("dig_element_records_bytes", E33, C), "f64", align=256),
         "out7": out("f64", (7, E33, C)), "MU": out("f64", (E33, C)), "SIGMA": out("f64", (E33, C)), "R_OBS": out("i32", (E33, C)),
         "FLAG": out("i32", (E33, C))}
    rates = ("MU", "SIGMA", "R_OBS", "FLAG")

    def invoke(a):
        ok = ctypes.c_int(0)
        call(a, "dig_element_pipeline_prepare", E=E33, C=C, compact_ok=ok)
        assert ok.value == 1
        call(a, "dig_bin_records_pack", N=N, C=C, records_bytes=b["bin_records"].nbytes)
        call(a, "dig_element_pipeline", alias={k: "absent" for k in rates}, N=N, E=E33, C=C,
             stages=7 | _lib.DIG_PIPE_COMPACT_L | _lib.DIG_PIPE_RECORDS)
        call(a, "dig_element_records_unpack", E=E33, C=C, cohort_major=0)

    got = guarded("plan form C=%d" % C, b, invoke, dev)
    check_accumulation(got, acc)
    check_statistics(got["out7"], st)


def test_gene_pipeline(dev):
    """dig_gene_pipeline at G = 33, C = 5 with the inputs and bounds of tests/test_gpu_parity.py
    test_gene_pipeline_all_cohorts_against_oracle."""
    from bench import make_workload
    from digdriver_amd import engine
    from oracle import dig_oracle as O
    G, C, N = 33, 5, 900
    w = make_workload(n_bins=N, n_elements=G, n_cohorts=C, seed=41, max_blocks=8)
    rng = np.random.default_rng(42)
    L = np.repeat(rng.poisson(6.0, (G, 4, 64)), 3, axis=2).astype(np.int32)
    L[:, :, ::7] += rng.integers(0, 3, (G, 4, 28))
    gene_length = rng.integers(300, 9000, G).astype(np.int32)
    acc_w = O.accumulate_elements(w["bin_mu"], w["bin_std"], w["bin_y"], w["bin_flag"], w["bin_ctx"], w["ov_ptr"], w["ov_idx"], L,
                                  w["strand_minus"].astype(bool), w["d_pr"], gene_length=gene_length)
    alpha = acc_w["MU"] ** 2 / acc_w["SIGMA"] ** 2
    theta = acc_w["SIGMA"] ** 2 / acc_w["MU"] * w["cj"][None, :]
    P4 = acc_w["P"]
    pi = {"SYN": P4[:, 0], "MIS": P4[:, 1], "NONS": P4[:, 2], "SPL": P4[:, 3]}
    pi["TRUNC"] = pi["NONS"] + pi["SPL"]
    pi["NONSYN"] = pi["MIS"] + pi["TRUNC"]
    obs5 = np.stack([rng.poisson(alpha * theta * pi[c] * 1.2) for c in ("SYN", "MIS", "NONS", "SPL")] +
                    [rng.poisson(alpha * theta * acc_w["P_INDEL"][:, None] * 0.1)], axis=1).astype(np.int32)
    obs5[::10, 1] += 400
    obs = {"SYN": obs5[:, 0], "MIS": obs5[:, 1], "NONS": obs5[:, 2], "SPL": obs5[:, 3]}
    obs["TRUNC"] = obs["NONS"] + obs["SPL"]
    obs["NONSYN"] = obs["MIS"] + obs["TRUNC"]
    ns = {c: rng.binomial(obs[c], 0.9) for c in O.GENE_CLASSES}
    n_samp = np.stack([ns[c] for c in O.GENE_CLASSES], axis=1).astype(np.int32)
    t_indel = rng.uniform(0.05, 0.3, C)
    want = O.gene_stats(acc_w["MU"], acc_w["SIGMA"], pi, obs, ns, w["cj"][None, :], pi_indel=acc_w["P_INDEL"][:, None],
                        obs_indel=obs5[:, 4], t_indel=t_indel[None, :])
    b = {**table_bufs(w, L, gene_length), "obs": arr("i32", obs5, poison=(0, 50)), "n_samp": arr("i32", n_samp, poison=(0, 50)),
         "cj": arr("f64", w["cj"]), "t_indel": arr("f64", t_indel), **acc_out_bufs(G, C, 4), "out": out("f64", (22, G, C)),
         "ws": ws(query("dig_accumulate_workspace", G, C), align=256)}
    got = guarded("dig_gene_pipeline", b, lambda a: call(a, "dig_gene_pipeline", with_indel=1, N=N, E=G, C=C), dev)
    rel_close(got["P"], acc_w["P"], 1e-11)
    rel_close(got["P_INDEL"], acc_w["P_INDEL"], 1e-12)
    assert np.array_equal(got["R_SIZE"], acc_w["R_SIZE"])
    for j, name in enumerate(engine.GS_PLANES):
        rel_close(got["out"][j], want[name], 1e-12 if name.startswith(("EXP", "THETA")) else RTOL)


# =====================================================================================================================================
# scale factors (dig_suffstats.hip): both branches of C <= 256, one row, a ragged last block
# =====================================================================================================================================
def _rates(N, C, seed=2):
    rng = np.random.default_rng([seed, N, C])
    return rng.gamma(9.0, 3.0, (N, C)), (rng.uniform(size=(N, C)) < 0.1).astype(np.uint8), rng


def _expected_sum(mu, flag):
    """1 / cj for one observed mutation: tests/test_gpu_parity.py test_scale_suffstats (rtol 1e-12)."""
    from oracle import dig_oracle as O
    return np.array([O.scale_factor_genome(mu[:, c], flag[:, c], 1.0, 1.0)[0] for c in range(mu.shape[1])])


@pytest.mark.parametrize("N, C", [(1, 1), (4097, 64), (300, 300)])
def test_scale_suffstats_and_the_local_scale_factors(dev, N, C):
    mu, flag, rng = _rates(N, C)
    wsb = query("dig_scale_suffstats_workspace", N, C)
    b = dict(bin_mu=arr("f64", mu), bin_flag=arr("u8", flag), out_sum=out("f64", C), ws=ws(wsb, align=8))
    got = guarded("dig_scale_suffstats", b, lambda a: call(a, "dig_scale_suffstats", N=N, C=C), dev)
    np.testing.assert_allclose(1.0 / got["out_sum"], _expected_sum(mu, flag), rtol=1e-12)
    snv, ind = np.rint(rng.uniform(1e3, 1e6, C)), np.rint(rng.uniform(1e2, 1e5, C))
    b2 = dict(bin_mu=arr("f64", mu), bin_flag=arr("u8", flag), n_snv_obs=arr("f64", snv), n_ind_obs=arr("f64", ind), out_sum=out("f64", C),
              cj=out("f64", C), cj_indel=out("f64", C), ws=ws(wsb, align=8))
    loc = guarded("dig_scale_factors_local", b2, lambda a: call(a, "dig_scale_factors_local", N=N, C=C), dev)
    # "Same bits as dig_scale_suffstats + dig_scale_factors(world = 1)", world = 1 being a plain division (include/dig_hip.h)
    assert GA.same_bits(loc["out_sum"], got["out_sum"])
    assert GA.same_bits(loc["cj"], snv / got["out_sum"]) and GA.same_bits(loc["cj_indel"], ind / got["out_sum"])


@pytest.mark.parametrize("world, C", [(1, 1), (3, 300)])
def test_scale_factors_from_parts(dev, world, C):
    """dig_scale_factors: both sums in rank order, then the division (include/dig_hip.h) -- the same IEEE operations in numpy, bit
    for bit."""
    rng = np.random.default_rng([world, C])
    parts = np.stack([rng.gamma(9.0, 3.0, (world, C)) * 1e4, np.rint(rng.uniform(1e3, 1e6, (world, C))), np.rint(rng.uniform(1e2, 1e5, (world, C)))], axis=1)
    b = dict(parts=arr("f64", parts), cj=out("f64", C), cj_indel=out("f64", C))
    got = guarded("dig_scale_factors", b, lambda a: call(a, "dig_scale_factors", world=world, C=C), dev)
    tot = np.zeros((3, C))
    for r in range(world):
        tot = tot + parts[r] if r else parts[r].copy()
    assert GA.same_bits(got["cj"], tot[1] / tot[0]) and GA.same_bits(got["cj_indel"], tot[2] / tot[0])


@pytest.mark.parametrize("C", [37, 256])
def test_chunked_suffstats_with_uneven_chunks(dev, C):
    """Three chunks of 1, 700 and 299 rows: chunk sums and scale factors bit for bit the host twin of
    tests/test_gpu_coresident_kernels.py (its _chunk_sums_twin, its divisions)."""
    from test_gpu_coresident_kernels import _bits, _chunk_sums_twin
    rows = np.array([0, 1, 701, 1000], np.int64)
    mu, flag, rng = _rates(1000, C, seed=3)
    obs = np.rint(rng.uniform(1e3, 1e6, (1, 2, C)))
    b = dict(bin_mu=arr("f64", mu), bin_flag=arr("u8", flag), out_chunks=out("f64", (3, C)), obs=arr("f64", obs), out_sum=out("f64", C),
             cj=out("f64", C), cj_indel=out("f64", C),
             ws=ws(query("dig_scale_suffstats_chunked_workspace", rows.ctypes.data_as(ctypes.c_void_p), 3, C), align=8))

    def invoke(a):
        call(a, "dig_scale_suffstats_chunked", C=C, chunk_rows=rows, n_chunks=3)
        call(a, "dig_scale_factors_chunked", n_chunks=3, world=1, C=C)

    got = guarded("chunked suffstats C=%d" % C, b, invoke, dev)
    want = _chunk_sums_twin(mu, flag, rows)
    assert np.array_equal(_bits(got["out_chunks"]), _bits(want))
    e = np.zeros(C)
    for j in range(3):
        e = e + want[j]
    assert np.array_equal(_bits(got["out_sum"]), _bits(e))
    assert np.array_equal(_bits(got["cj"]), _bits((0.0 + obs[0, 0]) / e)) and np.array_equal(_bits(got["cj_indel"]), _bits((0.0 + obs[0, 1]) / e))


# =====================================================================================================================================
# sort and Benjamini-Hochberg (dig_sort.hip, dig_bh.hip)
# =====================================================================================================================================
LENGTHS = [0, 1, 4095, 4097, 0, 8193, 17]            # odd row starts; the record tables are 8-byte entries over 4-byte slots


@functools.lru_cache(maxsize=None)
def sort_rows_case():
    """Rows of the value kinds of tests/test_gpu_sort.py _rows, a row of 257 values that share their upper 36 bits (the fix-up
    gives up: csrc/dig_sort.hip) and one whose q-values strictly increase: every element a record, more than the n / 2 entries
    its table holds (the tables live in the payload buffers, 4 bytes per element for 8-byte entries), so the call falls back to the
    payload form by itself."""
    from test_gpu_sort import _rows
    rng = np.random.default_rng(77)
    rows = _rows(rng, LENGTHS)
    rows.append(0.5 + rng.permutation(257) * 2.0 ** -40)
    steep = ((np.arange(4097) + 1.0) / 4097) ** 2
    rng.shuffle(steep)
    rows.append(steep)
    rp = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
    return rows, rp, np.concatenate(rows)


@functools.lru_cache(maxsize=None)
def lookup_rows_case():
    """Rows whose records fit their tables, so the lookup form itself writes q (no fallback): null-like lists, ties, an empty row, odd
    row starts."""
    rng = np.random.default_rng(78)
    rows = [rng.random(4095), rng.choice(rng.random(50), 4097), np.zeros(0), np.where(rng.random(8193) < 0.02, rng.random(8193) ** 6 * 1e-3, rng.random(8193)), rng.random(17)]      # a signal among nulls
    rp = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
    return rows, rp, np.concatenate(rows)


def _records_and_capacity(rows, rp):
    """Per row: the steps of the reverse running minimum of p / (rank / n), and bh_table_cap of csrc/dig_sort.hip (8-byte entries over
    the row's 4-byte slots)."""
    res = []
    for r, x in enumerate(rows):
        v = np.sort(x) / (np.arange(1, len(x) + 1) / max(len(x), 1))
        suffix = np.minimum.accumulate(np.concatenate([v, [np.inf]])[::-1])[::-1]
        res.append((int((v <= suffix[1:]).sum()), int(((rp[r] + len(x)) >> 1) - ((rp[r] + 1) >> 1))))
    return res


def _bh_ws(rp):
    from digdriver_amd import _lib
    return ws(query("dig_bh_ragged_workspace", _lib.host_ptr(rp), rp.size - 1))


@pytest.mark.parametrize("wanted", ["both", "p_sorted", "order"])
def test_sort_rows(dev, wanted):
    """Values and order bit for bit numpy's stable sort: tests/test_gpu_sort.py test_radix_sort_of_ragged_rows_equals_numpy_stable_sort."""
    rows, rp, p = sort_rows_case()
    n = p.size
    b = dict(p=arr("f64", p), ws=_bh_ws(rp))
    if wanted != "order":
        b["p_sorted"] = out("f64", n)
    if wanted != "p_sorted":
        b["order"] = out("u32", n)
    got = guarded("dig_sort_rows (%s)" % wanted, b, lambda a: call(a, "dig_sort_rows", row_ptr=rp, rows=rp.size - 1), dev)
    for r, row in enumerate(rows):
        order = np.argsort(row, kind="stable")
        if "p_sorted" in got:
            assert np.array_equal(got["p_sorted"][rp[r]:rp[r + 1]], row[order]), r
        if "order" in got:
            assert np.array_equal(got["order"][rp[r]:rp[r + 1]].astype(np.int64), order), r


@pytest.mark.parametrize("form", ["payload by fallback", "lookup"])
@pytest.mark.parametrize("wanted", ["both", "q", "row_min"])
def test_bh_qvalues_ragged(dev, wanted, form):
    """q-values bit for bit the host form nb_model.get_q_vals and row minima as in tests/test_gpu_sort.py
    test_bh_qvalues_of_ragged_rows_equal_the_host_form_bit_for_bit.  The rows of sort_rows_case hold lists with more records than their
    tables take (the call sorts again with a payload); those of lookup_rows_case fit with room to spare."""
    from digdriver_amd.sequence_model import nb_model
    rows, rp, p = sort_rows_case() if form != "lookup" else lookup_rows_case()
    fits = [rec <= cap for rec, cap in _records_and_capacity(rows, rp)]
    assert all(rec == 0 or rec + 2 <= cap for rec, cap in _records_and_capacity(rows, rp)) if form == "lookup" else not all(fits)
    b = dict(p=arr("f64", p), ws=_bh_ws(rp))
    if wanted != "row_min":
        b["q"] = out("f64", p.size)
    if wanted != "q":
        b["row_min"] = out("f64", len(rows))
    got = guarded("dig_bh_qvalues_ragged (%s)" % wanted, b,
                  lambda a: call(a, "dig_bh_qvalues_ragged", row_ptr=rp, rows=len(rows), sorted_out=0), dev)
    for r, row in enumerate(rows):
        if "q" in got and len(row):
            assert np.array_equal(got["q"][rp[r]:rp[r + 1]], nb_model.get_q_vals(row), equal_nan=True), r
        if "row_min" in got:
            want = (np.sort(row) / (np.arange(1, len(row) + 1) / float(len(row)))).min() if len(row) else np.inf
            assert got["row_min"][r] == want, r


def test_bh_qvalues_ragged_as_ranges_of_longer_lists(dev):
    """rank0 / n_global / carry given: the operations of tests/test_gpu_sort.py test_q_values_of_random_lists_and_ranges_fuzz."""
    rows, rp, p = sort_rows_case()
    rng = np.random.default_rng(8)
    n_glob = np.array([len(x) + int(rng.integers(0, 5000)) for x in rows], np.float64)
    rank0 = np.array([int(rng.integers(0, int(n_glob[r]) - len(x) + 1)) for r, x in enumerate(rows)], np.int64)
    carry = np.array([rng.random() * 2.0 if r % 3 else np.inf for r in range(len(rows))])
    b = dict(p=arr("f64", p), ws=_bh_ws(rp), q=out("f64", p.size), row_min=out("f64", len(rows)))
    got = guarded("dig_bh_qvalues_ragged (ranges)", b,
                  lambda a: call(a, "dig_bh_qvalues_ragged", row_ptr=rp, rows=len(rows), n_global=n_glob, rank0=rank0, carry=carry,
                                 sorted_out=0), dev)
    for r, x in enumerate(rows):
        if len(x) == 0:
            assert got["row_min"][r] == np.inf
            continue
        order = np.argsort(x, kind="stable")
        with np.errstate(all="ignore"):
            v = x[order] / ((rank0[r] + np.arange(1, len(x) + 1)) / n_glob[r])
        run = np.minimum.accumulate(np.minimum(v, carry[r])[::-1])[::-1]
        want = np.empty_like(run)
        want[order] = np.minimum(run, 1.0)
        assert np.array_equal(got["q"][rp[r]:rp[r + 1]], want), r
        assert got["row_min"][r] == v.min(), r


def test_bh_qvalues_sorted(dev):
    """(n, rows) = (4097, 3): two chunks per row, the second of one value; the host form's bits (include/dig_hip.h)."""
    from digdriver_amd.sequence_model import nb_model
    n, rows = 4097, 3
    rng = np.random.default_rng(12)
    p = np.sort(np.stack([rng.random(n), rng.random(n) ** 4, np.minimum(1.0, rng.exponential(0.05, n))]), axis=1)
    b = dict(p=arr("f64", p), q=out("f64", (rows, n)), ws=ws(query("dig_bh_workspace", n, rows), align=8))
    got = guarded("dig_bh_qvalues_sorted", b, lambda a: call(a, "dig_bh_qvalues_sorted", n=n, rows=rows), dev)
    for r in range(rows):
        assert np.array_equal(got["q"][r], nb_model.get_q_vals(p[r])), r


def test_misaligned_workspaces_are_refused(dev):
    """The alignments include/dig_hip.h states for the workspaces are checked before anything is launched."""
    import torch
    from digdriver_amd import _lib
    need = query("dig_element_stats_workspace", 1, 1)
    buf = torch.zeros((1 << 16) + need, dtype=torch.uint8, device=dev)
    p = buf.data_ptr()
    lib = _lib.load()
    s = _lib.stream_ptr()
    assert lib.dig_bh_qvalues_sorted(p + 1024, 10, 1, p + 2048, p + 4, 1 << 12, s) == -1 and "8-byte aligned" in _lib.last_error()
    rows = np.array([0, 10], np.int64)
    assert lib.dig_scale_suffstats_chunked(p + 1024, None, 1, _lib.host_ptr(rows), 1, p + 2048, p + 4, 1 << 12, s) == -1
    assert "8-byte aligned" in _lib.last_error()
    assert lib.dig_scale_suffstats(p + 1024, p + 512, 10, 1, p + 2048, p + 4, 1 << 12, s) == -1 and "8-byte aligned" in _lib.last_error()
    assert lib.dig_element_stats(*([p] * 6), 0, *([p] * 6), 1, 1, p + 2, need, s) == -1 and "4-byte aligned" in _lib.last_error()
    torch.cuda.synchronize()


# =====================================================================================================================================
# gather (dig_gather.hip): all six kernels of launch_gather, each reached by shape and by alignment alone
# =====================================================================================================================================
GATHER_ALL = [(50, 100, 77), (50, 99, 77)]                                       # (N, L, T), all tracks
GATHER_SUBSET = [(11, 100, 64, 64), (9, 99, 77, 40), (5, 100, 1100, 16), (3, 4, 8, 8)]          # (N, L, T, n_sel)
GATHER_MODES = {"vector": (), "x at element alignment": ("x",), "out at element alignment": ("out",),
                "tracks at element alignment": ("tracks",)}
_SRC = {"i16": 2, "f32": 0, "f64": 1}                                           # DIG_I16, DIG_F32, DIG_F64
_DST = {"f32": 0, "bf16": 3}
FAST = {"block": "rows", "wide": None, "subset": "rows", "transpose_all": "transpose"}      # a fast kernel -> where misalignment must send it


def gather_kernel(S, D, L, T, T_sel, has_tracks, transpose, x, o, tr):
    """The conditions of launch_gather (csrc/dig_gather.hip) on the addresses a call was given: which kernel ran."""
    sel_ok = has_tracks and T_sel % 4 == 0 and 0 < T_sel <= 2048 and o % 16 == 0 and tr % 16 == 0
    if not transpose and not has_tracks and (L * T) % 4 == 0 and x % 32 == 0 and o % 16 == 0:
        return "block"
    if not transpose and sel_ok and T <= 1024 and x % 8 == 0 and (L * T * S) % 8 == 0 and L % (8 // S) == 0 and (T_sel * D) % 16 == 0:
        return "wide"
    if not transpose and sel_ok and T <= 2048:
        return "subset"
    if not transpose:
        return "rows"
    if not has_tracks and L % 4 == 0 and L <= 252 and o % 16 == 0 and x % (4 * S) == 0:
        return "transpose_all"
    return "transpose"


@pytest.mark.parametrize("dst", ["f32", "bf16"])
@pytest.mark.parametrize("src", ["i16", "f32", "f64"])
def test_gather_bins_every_kernel_by_shape_and_by_alignment(dev, src, dst):
    """Reference: x[rows][:, :, tracks] in numpy, exact (bf16 through .to(torch.bfloat16) of it).  Rows include bin 0 and bin
    N - 1, x holds exactly N * L * T elements."""
    import torch
    S, D = GA._NP[src].itemsize, GA._NP[dst].itemsize
    rng = np.random.default_rng([S, D])
    seen = {}                                                                      # (shape, transpose) -> {mode: kernel}
    for shape in GATHER_ALL + GATHER_SUBSET:
        N, L, T = shape[:3]
        n_sel = shape[3] if len(shape) == 4 else None
        x = (rng.integers(-1200, 12000, (N, L, T)) / (1 if src == "i16" else 4)).astype(GA._NP[src])
        rows = np.array([0, N - 1, N // 2, 0, N - 1, 1, N - 2], np.int64)
        tracks = None if n_sel is None else rng.permutation(T)[:n_sel].astype(np.int32)
        T_sel = T if tracks is None else n_sel
        for transpose in (0, 1):
            want = x[rows].astype(np.float32) if tracks is None else x[rows][:, :, tracks].astype(np.float32)
            want = np.ascontiguousarray(want.transpose(0, 2, 1)) if transpose else want
            if dst == "bf16":
                want = torch.from_numpy(want).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
            for mode, low in GATHER_MODES.items():
                if tracks is None and mode.startswith("tracks"):
                    continue
                b = dict(x=arr(src, x, align=S if "x" in low else 32), rows=arr("i64", rows, index=(0, N - 1)))
                if tracks is not None:
                    b["tracks"] = arr("i32", tracks, index=(0, T - 1), align=4 if "tracks" in low else 16)
                b["out"] = out(dst, want.shape, align=D if "out" in low else 16)

                def invoke(a):
                    if isinstance(a, GuardedArena):
                        seen.setdefault((shape, transpose), {})[mode] = gather_kernel(
                            S, D, L, T, T_sel, tracks is not None, transpose, a.ptr("x"), a.ptr("out"), a.ptr("tracks") or 0)
                    call(a, "dig_gather_bins", src=_SRC[src], N=N, L=L, T=T, B=len(rows), T_sel=T_sel, dst=_DST[dst], transpose=transpose)

                got = guarded("dig_gather_bins %s->%s %s transpose=%d, %s" % (src, dst, shape, transpose, mode), b, invoke, dev)
                assert GA.same_bits(got["out"], want), (shape, transpose, mode)
    by_shape = {k: v["vector"] for k, v in seen.items()}
    assert set(by_shape.values()) == {"block", "wide", "subset", "rows", "transpose_all", "transpose"}, by_shape
    for key, kernel in by_shape.items():                     # every vector kernel is also left through alignment alone
        if kernel in FAST:
            others = {m: k for m, k in seen[key].items() if m != "vector"}
            assert any(k != kernel for k in others.values()), (key, kernel, others)
            if FAST[kernel]:
                assert FAST[kernel] in others.values(), (key, kernel, others)


# =====================================================================================================================================
# genome readers (dig_context.hip, dig_context5.hip, dig_mutctx.hip, dig_mutfunc.hip, dig_genesites.hip, dig_tiles.hip,
# dig_tiles_rows.hip): genome arrays at exactly their documented length, pads included, at 16 (mod 32); regions, rows and genes
# touch base 0 of the first chromosome and the last base of the last one
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def tile_problem():
    from digdriver_amd.data_tools.genome import PackedGenome
    from test_gpu_tile_cuts import _problem
    seqs, regions, S3, S5 = _problem()
    g = PackedGenome.from_sequences(seqs)
    ci = g.chrom_index([r[0] for r in regions])
    starts, ends = np.array([r[1] for r in regions], np.int64), np.array([r[2] for r in regions], np.int64)
    assert starts[0] == 0 and ci[0] == 0 and ci[1] == len(seqs) - 1 and ends[1] > g.lengths[-1]      # base 0 ... the last base
    return seqs, regions, S3, S5, g, ci.astype(np.int32), starts, ends


def genome4_bufs(g):
    """The 4-bit genome of dig_count_contexts / dig_base_tile_probs: one pad word at either end."""
    assert g.words.size == 2 + int(((g.lengths + 7) // 8).sum())
    return dict(words=arr("u32", g.words, align=16), chrom_off=arr("i64", g.offsets, index=(0, int(g.offsets.max()))),
                chrom_len=arr("i64", g.lengths, index=(int(g.lengths.min()), int(g.lengths.max())))), dict(n_words=g.words.size, n_chrom=len(g.names))


def genome2_bufs(g):
    """The 2-bit genome: 4 pad words in front, 24 behind the last chromosome (include/dig_hip.h), the run list and its buckets."""
    w2, ns, ne, bk = g.two_bit()
    total = int(((g.lengths + 7) // 8 * 8).sum())
    assert w2.size == 4 + (total + 15) // 16 + 24 and len(ns) > 0
    b = dict(words2=arr("u32", w2, align=16), nint_start=arr("i64", ns, index=(0, 64 + total)), nint_end=arr("i64", ne, index=(0, 64 + total)),
             nint_bucket=arr("i32", bk, index=(0, len(ns))), chrom_off=arr("i64", g.offsets, index=(0, int(g.offsets.max()))),
             chrom_len=arr("i64", g.lengths, index=(int(g.lengths.min()), int(g.lengths.max()))))
    return b, dict(n_words2=w2.size, n_int=len(ns), n_buckets=len(bk), n_chrom=len(g.names))


def region_bufs(g, ci, starts, ends, minus=None):
    lo = int(g.lengths.min())
    b = dict(reg_chrom=arr("i32", ci, index=(0, len(g.names) - 1)), reg_start=arr("i64", starts, index=(0, lo)), reg_end=arr("i64", ends, index=(0, lo)))
    if minus is not None:
        b["reg_minus"] = arr("u8", minus)
    return b


@pytest.mark.parametrize("form", ["dig_count_contexts", "dig_count_contexts2", "dig_count_contexts5"])
def test_context_counts(dev, form):
    """Trinucleotide counts against oracle.dig_oracle.count_contexts_regions (tests/test_gpu_parity.py
    test_context_counting_matches_reference_golden_and_oracle), penta-nucleotide counts against the statement rule5_regions of
    tests/test_penta_context_host.py: exact."""
    from oracle import dig_oracle as O
    from test_penta_context_host import rule5_regions
    seqs, regions, _, _, g, ci, starts, ends = tile_problem()
    chroms = [r[0] for r in regions]
    minus = (np.arange(len(regions)) % 2).astype(np.uint8)
    gb, gs = genome4_bufs(g) if form == "dig_count_contexts" else genome2_bufs(g)
    penta = form.endswith("5")
    R = len(regions)
    b = {**gb, **region_bufs(g, ci, starts, ends, minus), "out": out("i32", (R, 1024 if penta else 64), align=16 if penta else 4)}
    got = guarded(form, b, lambda a: call(a, form, R=R, **gs), dev)
    want = rule5_regions(seqs, chroms, starts, ends, minus.astype(bool)) if penta else O.count_contexts_regions(seqs, chroms, starts, ends, minus)
    assert np.array_equal(got["out"].astype(np.int64), want)
    assert want[0].sum() > 0 and want[1].sum() > 0


@functools.lru_cache(maxsize=None)
def tile_oracle(n_up, binsize, n_tiles):
    from test_gpu_tile_cuts import _oracle
    seqs, regions, S3, S5 = tile_problem()[:4]
    return _oracle(seqs, regions, (S3 if n_up == 1 else S5)[:49 if n_up == 1 else 9], n_up, binsize, n_tiles)


@pytest.mark.parametrize("n_up, C, binsize, n_tiles", [(1, 5, 7, 20), (1, 37, 7, 20), (1, 49, 7, 20), (1, 5, 1, 300),
                                                       (2, 3, 7, 20), (2, 9, 7, 20), (2, 3, 1, 300), (2, 9, 1, 300)])
def test_base_tile_probs(dev, n_up, C, binsize, n_tiles):
    """_problem() and the bounds (_check: 1e-12) of tests/test_gpu_tile_cuts.py; binsize 1 leaves the long region to the general
    kernel (the deferred path).  pt, first_pos and n_valid guarded."""
    from test_gpu_tile_cuts import _check
    seqs, regions, S3, S5, g, ci, starts, ends = tile_problem()
    S = (S3 if n_up == 1 else S5)[:C]
    R = len(regions)
    gb, gs = genome4_bufs(g)
    b = {**gb, **region_bufs(g, ci, starts, ends), "s_prob": arr("f64", S), "pt": out("f64", (C, R, n_tiles)), "first_pos": out("i64", R),
         "n_valid": out("i32", R)}
    got = guarded("dig_base_tile_probs_ctx n_up=%d C=%d binsize=%d" % (n_up, C, binsize), b,
                  lambda a: call(a, "dig_base_tile_probs_ctx", R=R, C=C, n_up=n_up, binsize=binsize, n_tiles=n_tiles, **gs), dev)
    _check((got["pt"], got["first_pos"], got["n_valid"]), tile_oracle(n_up, binsize, n_tiles), C)


@pytest.mark.parametrize("binsize, n_tiles", [(7, 20), (1, 300)])
def test_tile_mut_counts(dev, binsize, n_tiles):
    """k against the definition in include/dig_hip.h, exact: a pair counts when the mutation's START is one of the region's
    positions, in the tile that holds it, for a cohort inside [0, C)."""
    seqs, regions, _, _, g, ci, starts, ends = tile_problem()
    _, first, nval, _ = tile_oracle(1, binsize, n_tiles)
    C, R, M = 5, len(regions), 3000
    rng = np.random.default_rng(binsize)
    m_chrom = rng.integers(0, 2, M)
    m_start = np.where(rng.random(M) < 0.5, rng.integers(0, 2100, M), rng.choice(np.concatenate([starts, ends - 1, [0, 1, 1500, 2002]]), M)).astype(np.int64)
    m_start[:2] = [0, g.lengths[-1] - 1]
    m_chrom[:2] = [0, len(g.names) - 1]
    m_cohort = rng.integers(0, C, M).astype(np.int32)
    pm, pr = [], []
    for m in range(M):                                       # mutation-major, regions ascending: the order of dig_overlap_join_fill
        for r in range(R):
            if ci[r] == m_chrom[m] and starts[r] <= m_start[m] < ends[r]:
                pm.append(m)
                pr.append(r)
    pm, pr = np.array(pm, np.int32), np.array(pr, np.int32)
    want = np.zeros((C, R, n_tiles), np.int32)
    for m, r in zip(pm, pr):
        off = m_start[m] - first[r]
        if off >= 0 and off // binsize < nval[r]:
            want[m_cohort[m], r, off // binsize] += 1
    assert want.sum() > 200 and want[:, 0].sum() > 0 and want[:, 1].sum() > 0
    b = dict(pair_mut=arr("i32", pm, index=(0, M - 1)), pair_reg=arr("i32", pr, index=(0, R - 1)), mut_start=arr("i64", m_start, poison=(0, 1000)),
             mut_cohort=arr("i32", m_cohort, index=(0, C - 1)), first_pos=arr("i64", first, poison=(0, 100)),
             n_valid=arr("i32", nval, index=(0, n_tiles)), k=out("i32", (C, R, n_tiles)))
    got = guarded("dig_tile_mut_counts", b, lambda a: call(a, "dig_tile_mut_counts", n_pairs=len(pm), binsize=binsize, n_tiles=n_tiles, R=R, C=C), dev)
    assert np.array_equal(got["k"], want)


def _decode(code, W):
    return "".join("ACGT"[(int(code) >> (2 * k)) & 3] for k in range(W))


@pytest.mark.parametrize("n_up, n_down, collapse", [(2, 2, 0), (1, 1, 1), (7, 8, 0)])
def test_mutation_contexts_with_its_exact_workspace(dev, n_up, n_down, collapse):
    """Against the per-row rule rule3 of tests/test_mutation_context_host.py (tests/test_gpu_mutation_context.py
    test_fuzz_against_rule): a kept row carries the rule's window, a mismatching or dropped row has none, a row left to the host
    is one whose window the 2-bit genome cannot give (a letter other than ACGT, a window cut by the chromosome's ends)."""
    from test_mutation_context_host import rule3
    seqs, _, _, _, g, _, _, _ = tile_problem()
    names = list(seqs)
    rng = np.random.default_rng(n_up)
    n = 64 * 5 + 3                                           # five full waves and three rows: runs cross wave and workgroup edges
    chrom = np.sort(rng.integers(0, 2, n)).astype(np.int32)
    start = np.empty(n, np.int64)
    i = 0
    while i < n:                                             # runs of rows with one START, some far longer than a wave
        k = int(min(rng.choice([1, 1, 2, 3, 150]), n - i, np.sum(chrom[i:] == chrom[i])))
        start[i:i + k] = rng.integers(0, len(seqs[names[chrom[i]]]))
        i += k
    first_chr2 = int(np.argmax(chrom == 1))
    start[0], start[-1] = 0, len(seqs[names[1]]) - 1          # base 0 of the first chromosome, the last base of the last
    start[first_chr2 - 1] = 620                              # inside the N run
    letters = [seqs[names[c]][s].upper() for c, s in zip(chrom, start)]
    refs = [b if (b in "ACGT" and rng.random() < 0.85) else "ACGT"[int(rng.integers(0, 4))] for b in letters]
    W = n_up + n_down + 1
    gb, gs = genome2_bufs(g)
    b = {**gb, "row_chrom": arr("i32", chrom, index=(0, 1)), "row_start": arr("i64", start, index=(0, int(g.lengths.min()) - 1)),
         "row_ref": arr("u8", np.array(["ACGT".index(r) for r in refs], np.uint8)), "status": out("u8", n), "context": out("u32", n),
         "ws": ws(query("dig_mutation_contexts_workspace", n), align=4)}
    got = guarded("dig_mutation_contexts", b,
                  lambda a: call(a, "dig_mutation_contexts", n_rows=n, n_up=n_up, n_down=n_down, collapse=collapse, **gs), dev)
    status, context = got["status"], got["context"]
    seen = set()
    for c in (0, 1):
        sel = np.flatnonzero(chrom == c)
        inner = [j for j in sel if start[j] >= n_up]         # (the rule's Python slice wraps for a window that starts before base 0)
        rule = dict(zip(inner, rule3(seqs[names[c]], [int(start[j]) for j in inner], [refs[j] for j in inner], n_up, n_down, bool(collapse))))
        for j in sel:
            seen.add(int(status[j]))
            if status[j] == 0:                               # DIG_MC_KEPT
                assert _decode(context[j], W) == rule[j], j
            elif status[j] in (1, 2):                        # DIG_MC_MISMATCH, DIG_MC_DROPPED
                assert j not in rule or rule[j] == "", j
                assert (status[j] == 1) == (letters[j] != refs[j]), j
            else:                                            # DIG_MC_HOST: the rule has no full ACGT window either
                assert status[j] == 3 and (j not in rule or len(rule[j]) < W), j
    assert seen == {0, 1, 2, 3} and status[0] in (1, 3) and status[-1] in (1, 3)


@functools.lru_cache(maxsize=None)
def gene_case():
    import tempfile
    from pathlib import Path
    from test_gpu_gene_site_counts import genes_at_contig_ends, load
    from test_gpu_mutation_function import fuzz_bed12, fuzz_genome
    rng = np.random.default_rng(19)
    seqs = fuzz_genome(rng, sizes=(("chr1", 9000), ("chr2", 7001)), n_runs=2, n_iupac=6, max_run=40)
    n2 = len(seqs["chr2"])
    bed = fuzz_bed12(rng, seqs, 30, max_exons=5) + genes_at_contig_ends(seqs) + \
        "2\t%d\t%d\tat_end2\t0\t+\t%d\t%d\t0\t1\t12,\t0,\n" % (n2 - 12, n2, n2 - 12, n2)        # ... the last base of the last chromosome
    with tempfile.TemporaryDirectory() as tmp:
        g, genes, gch, stated = load(Path(tmp), bed, seqs)
    return seqs, g, genes, gch, stated


def gene_table_bufs(g, genes, gch):
    lo = int(g.lengths.min())
    n_blk, n_spl = len(genes.blk_start), len(genes.spl_pos)
    assert n_spl > 0
    return dict(gene_chrom=arr("i32", gch, index=(0, len(g.names) - 1)), gene_minus=arr("u8", genes.minus),
                blk_ptr=arr("i64", genes.blk_ptr, index=(0, n_blk)), blk_start=arr("i64", genes.blk_start, index=(1, lo)),
                blk_end=arr("i64", genes.blk_end, index=(1, lo)), cds_off=arr("i64", genes.cds_off, poison=(0, 3)),
                spl_ptr=arr("i64", genes.spl_ptr, index=(0, n_spl)), spl_pos=arr("i64", genes.spl_pos, index=(1, lo)))


def test_gene_site_counts(dev):
    """Against the statement gene_counts_statement.gene_counts, exact: tests/test_gpu_gene_site_counts.py
    test_kernel_fuzz_against_statement (the genes the kernel leaves to the host have zero rows)."""
    import gene_counts_statement as GS
    seqs, g, genes, gch, stated = gene_case()
    G = len(stated)
    want = [GS.gene_counts(seqs, x) for x in stated]
    L = np.array([w[0] for w in want], np.int32)
    nsl = np.array([w[1] for w in want], np.int32)
    other = np.array([w[2] for w in want], bool)
    gb, gs = genome2_bufs(g)
    b = {**gb, **gene_table_bufs(g, genes, gch), "L": out("i32", (G, 4, 192)), "n_stop_loss": out("i32", G), "status": out("u8", G)}
    got = guarded("dig_gene_site_counts", b, lambda a: call(a, "dig_gene_site_counts", n_genes=G, **gs), dev)
    assert np.array_equal(got["status"] == 1, other) and 0 < other.sum() < G
    assert np.array_equal(got["L"][~other], L[~other]) and np.array_equal(got["n_stop_loss"][~other], nsl[~other])
    assert (got["L"][other] == 0).all() and (got["n_stop_loss"][other] == 0).all()


def test_mutation_function(dev):
    """Against the statement mutfunc_statement.pair_outputs, exact: tests/test_gpu_mutation_function.py
    test_kernel_fuzz_against_statement, its pairs at a smaller count, plus SNVs on the first and the last CDS base of every gene."""
    import mutfunc_statement as S
    seqs, g, genes, gch, stated = gene_case()
    rng = np.random.default_rng(23)
    rows = []                                                # (gene, start, end, kind, ref, alt)
    for gi, x in enumerate(stated):
        cds = S.cds_positions(x)
        for p in (cds[0], cds[-1]):
            rows.append((gi, p, p, 0, int(rng.integers(0, 4)), int(rng.integers(0, 4))))
    for _ in range(1500):
        gi = int(rng.integers(0, len(stated)))
        x = stated[gi]
        if rng.random() < 0.85:
            cds = S.cds_positions(x)
            p = x["splice"][int(rng.integers(0, len(x["splice"])))] if x["splice"] and rng.random() < 0.1 else cds[int(rng.integers(0, len(cds)))]
            base = S.letter(seqs, x["chrom"], p)
            r = "ACGT".index(base) if base in "ACGT" and rng.random() < 0.9 else int(rng.integers(0, 4))
            rows.append((gi, p, p, 0, r, (r + int(rng.integers(1, 4))) % 4))
        else:
            lo, hi = x["blocks"][0][0], x["blocks"][-1][1]
            p = int(rng.integers(max(lo - 5, 1), hi + 5))
            rows.append((gi, p, p + int(rng.choice([0, 1, 3, 30, 400])), 1 + int(rng.integers(0, 2)), 0, 0))
    want = np.array([S.pair_outputs(seqs, stated[gi], p, q, k, "ACGT"[r] if k == 0 else "", "ACGT"[a] if k == 0 else "")
                     for gi, p, q, k, r, a in rows], np.int64)
    cols = list(zip(*rows))
    n, G = len(rows), len(stated)
    lo = int(g.lengths.min())
    gb, gs = genome2_bufs(g)
    b = {**gb, **gene_table_bufs(g, genes, gch), "pair_gene": arr("i32", cols[0], index=(0, G - 1)),
         "pair_start": arr("i64", cols[1], index=(1, lo)), "pair_end": arr("i64", cols[2], index=(1, lo)), "pair_kind": arr("u8", cols[3]),
         "pair_ref": arr("u8", cols[4]), "pair_alt": arr("u8", cols[5]), "impact": out("u8", n), "status": out("u8", n),
         "n_cds": out("i32", n), "cds_min": out("i32", n), "cds_max": out("i32", n)}
    got = guarded("dig_mutation_function", b, lambda a: call(a, "dig_mutation_function", n_genes=G, n_pairs=n, **gs), dev)
    for k, name in enumerate(("impact", "status", "n_cds", "cds_min", "cds_max")):
        bad = np.flatnonzero(got[name].astype(np.int64) != want[:, k])
        assert bad.size == 0, (name, bad[:5], got[name][bad[:5]], want[bad[:5], k])
    assert set(want[:, 1]) >= {S.OK, S.WRONG_REF} and len(set(want[:, 0])) >= 5


# =====================================================================================================================================
# key-run counters and the join (dig_genecounts.hip, dig_objectives.hip, dig_seqcounts.hip, dig_sitematch.hip, dig_join.hip):
# sorted key arrays of B - 1, B and B + 65 keys (B: the kernel's workgroup) whose first run starts at key 0 and crosses the wave and
# the workgroup edge, so what lies in front of keys[0] is what keys[i - 1] would read there
# =====================================================================================================================================
def _bits_for(n):
    """key_bits_for of csrc/dig_keyruns.hpp: the bits that hold 0 .. n - 1 (at least one)."""
    b = 1
    while b < 62 and (1 << b) < n:
        b += 1
    return b


def _edge_lengths(B):
    return [B - 1, B, B + 65]


def _first_run(n, B):
    """Length of the run at key 0: past the wave edge for n < B, past the workgroup edge otherwise."""
    return min(n, 100 if n < B else B + 10)


def test_overlap_join_count_and_fill(dev):
    """The block table and rows of tests/overlap_join_cases.py against oracle.interval_join_pairs: tests/test_gpu_overlap_join.py."""
    import overlap_join_cases as K
    from digdriver_amd import engine
    from oracle import dig_oracle as O
    blocks, muts = K.block_table(), K.mutation_rows()
    order, start_key, runmax_key, end_eff = engine.join_blocks(*blocks)
    n_blk, n_mut = len(order), len(muts[0])
    hi = int(start_key.max())
    table = dict(blk_start_key=arr("i64", start_key, index=(0, hi)), blk_runmax_key=arr("i64", runmax_key, index=(0, hi)),
                 blk_end=arr("i64", end_eff, index=(0, 1000)), mut_chrom=arr("i64", muts[0], index=(0, 7)),
                 mut_start=arr("i64", muts[1], index=(0, 1000)), mut_end=arr("i64", muts[2], index=(0, 1000)))
    got = guarded("dig_overlap_join_count", {**table, "counts": out("i32", n_mut)},
                  lambda a: call(a, "dig_overlap_join_count", n_blk=n_blk, n_mut=n_mut), dev)
    counts = got["counts"].astype(np.int64)
    offsets = np.cumsum(counts) - counts
    total = int(counts.sum())
    b = {**table, "offsets": arr("i64", offsets, index=(0, total)), "pair_mut": out("i32", total), "pair_blk": out("i32", total)}
    got = guarded("dig_overlap_join_fill", b, lambda a: call(a, "dig_overlap_join_fill", n_blk=n_blk, n_mut=n_mut), dev)
    mi, bi = O.interval_join_pairs(*muts, *blocks)
    want = sorted(zip(mi.tolist(), bi.tolist()))
    assert len(want) > 200 and sorted(zip(got["pair_mut"].tolist(), order[got["pair_blk"]].tolist())) == want
    assert (np.diff(got["pair_mut"]) >= 0).all()


@pytest.mark.parametrize("n, max_s", [(255, 270.0), (256, 270.0), (321, 270.0), (321, 25.0)])
def test_gene_row_keys_and_gene_counts(dev, n, max_s):
    """dig_gene_row_keys against the key of include/dig_hip.h and dig_gene_counts (kGeneCountBlock = 256) against the statement
    gene_obs_statement.cohort_counts, exact: tests/test_gpu_gene_cohorts.py.  max_s = 25: the sample of the run at key 0 is
    blacklisted and none of its rows counts."""
    import gene_obs_statement as GO
    G, C, per = 6, 3, 40                                     # genes of the model, cohorts, samples per cohort
    S = C * per
    rng = np.random.default_rng(n)
    run = _first_run(n, 256)
    cohort = np.concatenate([np.zeros(run, np.int64), rng.integers(0, C, n - run)])
    gene = np.concatenate([np.zeros(run, np.int64), rng.integers(0, G + 2, n - run)])        # G: outside the model, G + 1: TP53
    sample = np.concatenate([np.zeros(run, np.int64), rng.integers(0, 12, n - run)])         # dense per cohort
    cls = np.concatenate([np.zeros(run, np.int64), rng.integers(0, 6, n - run)])
    sb = _bits_for(S)
    gs = cohort * per + sample
    shuffle = rng.permutation(n)                             # rows in any order
    off = (np.arange(C + 1) * per).astype(np.int64)
    rk = dict(gene=arr("i32", gene[shuffle], index=(0, G + 1)), sample=arr("i32", sample[shuffle], index=(0, per - 1)),
              annot=arr("u8", cls[shuffle], index=(0, 5)), cohort=arr("i32", cohort[shuffle], index=(0, C - 1)), sample_off=arr("i64", off, index=(0, S)),
              keys=out("i64", n), sample_total=out("i32", S))
    made = guarded("dig_gene_row_keys n=%d" % n, rk, lambda a: call(a, "dig_gene_row_keys", n=n, G=G, C=C, n_samples=S), dev)
    assert np.array_equal(made["keys"], (((cohort * (G + 2) + gene) << (sb + 3)) | (gs << 3) | cls)[shuffle])
    total = np.bincount(gs, minlength=S).astype(np.int32)
    assert np.array_equal(made["sample_total"], total)
    keys = np.sort(made["keys"])
    assert keys[0] == 0 and keys[run - 1] == 0 and (n == run or keys[run] != 0)
    max_gs = 3.0
    names = ["g%d" % g for g in range(G)] + ["outside", "TP53"]
    annots = GO.OBS_CLASSES + ("other",)
    top = ((C * (G + 2) - 1) << (sb + 3)) | ((S - 1) << 3) | 5         # the largest valid key
    b = dict(keys=arr("i64", keys, index=(0, top)), sample_total=arr("i32", total, poison=(0, 20)), obs=out("i32", (G, 5, C)),
             n_samp=out("i32", (G, 6, C)), extra=out("i32", (G, 2, C)), n_syn=out("i64", C), blacklisted=out("u8", S), scratch=out("i32", (G, 5, C)))
    got = guarded("dig_gene_counts n=%d" % n, b,
                  lambda a: call(a, "dig_gene_counts", n=n, n_samples=S, max_s=max_s, max_gs=max_gs, tp53=G + 1, G=G, C=C), dev)
    black = set()
    for c in range(C):
        rows = [(names[g], "s%d" % s, annots[k]) for g, s, k, cc in zip(gene, sample, cls, cohort) if cc == c]
        want = GO.cohort_counts(rows, names[:G], max_s, max_gs)
        black |= {c * per + int(s[1:]) for s in want["blacklist"]}
        for g in range(G):
            for k, a in enumerate(GO.OBS_CLASSES):
                assert got["obs"][g, k, c] == want["obs"].get((names[g], a), 0), (c, g, a)
            for k, q in enumerate(("SYN", "MIS", "NONS", "SPL", "TRUNC", "NONSYN")):
                assert got["n_samp"][g, k, c] == want["n_samp"].get((names[g], q), 0), (c, g, q)
            assert got["extra"][g, 0, c] == want["n_samp"].get((names[g], "INDEL"), 0) and got["extra"][g, 1, c] == want["pairs"].get(names[g], 0)
        assert got["n_syn"][c] == want["n_syn"], c
    assert np.array_equal(np.flatnonzero(got["blacklisted"]), sorted(black)) and (0 in black) == (max_s < run)
    assert got["obs"][0, 0, 0] >= (0 if 0 in black else 3)   # the run at key 0: one (gene, sample, class) group, clipped to 3


@pytest.mark.parametrize("n", _edge_lengths(256))
def test_window_pair_keys_hits_and_objectives(dev, n):
    """dig_window_pair_keys against the key of include/dig_hip.h; dig_window_sample_hits / dig_window_objectives (kObjBlock = 256) against the statement objectives_statement (sample_loads,
    window_labels), exact: tests/test_gpu_objectives.py.  One pair per row: every row lies in one window."""
    import objectives_statement as OS
    N, C, per, n_uid = 37, 3, 9, 50
    S = C * per
    rng = np.random.default_rng(n + 1)
    run = _first_run(n, 256)
    z = np.zeros(run, np.int64)
    sample = np.concatenate([z, rng.integers(0, S, n - run)])                 # global
    window = np.concatenate([z, rng.integers(0, N, n - run)])
    indel = np.concatenate([z, (rng.random(n - run) < 0.2).astype(np.int64)])
    uid = np.concatenate([z, rng.integers(0, 6, n - run)])                    # few ids: duplicates of one identity among the rows
    ub, wb = _bits_for(n_uid), _bits_for(N)
    # one pair per row, in any order; the blocks are the windows in another order (blk_window)
    shuffle, blk_window = rng.permutation(n), rng.permutation(N).astype(np.int32)
    pair_blk = np.argsort(blk_window)[window[shuffle]]
    pk = dict(pair_row=arr("i32", np.arange(n), index=(0, n - 1)), pair_blk=arr("i32", pair_blk, index=(0, N - 1)),
              blk_window=arr("i32", blk_window, index=(0, N - 1)), row_sample=arr("i32", sample[shuffle], index=(0, S - 1)),
              row_uid=arr("i32", uid[shuffle], index=(0, n_uid - 1)), row_indel=arr("u8", indel[shuffle]), keys=out("i64", n))
    made = guarded("dig_window_pair_keys n=%d" % n, pk,
                   lambda a: call(a, "dig_window_pair_keys", n_pairs=n, n_blk=N, n_rows=n, n_samples=S, N=N, n_uid=n_uid), dev)
    assert np.array_equal(made["keys"], ((((sample << wb) | window) << (1 + ub)) | (indel << ub) | uid)[shuffle])
    keys = np.sort(made["keys"])
    assert keys[0] == 0 and keys[run - 1] == 0
    keep = (np.arange(S) % 4 != 1).astype(np.uint8)
    off = (np.arange(C + 1) * per).astype(np.int64)
    top = int(((((S - 1) << wb) | (N - 1)) << (1 + ub)) | (1 << ub) | (n_uid - 1))       # the largest valid key
    got_h = guarded("dig_window_sample_hits n=%d" % n, dict(keys=arr("i64", keys, index=(0, top)), hits=out("i32", S)),
                    lambda a: call(a, "dig_window_sample_hits", n=n, n_samples=S, N=N, n_uid=n_uid), dev)
    b = dict(keys=arr("i64", keys, index=(0, top)), keep=arr("u8", keep), sample_off=arr("i64", off, index=(0, S)),
             labels=out("f64", (N, C)), scratch=out("i32", (N, C)))
    got_l = guarded("dig_window_objectives n=%d" % n, b,
                    lambda a: call(a, "dig_window_objectives", n=n, n_samples=S, N=N, C=C, n_uid=n_uid), dev)
    idx = np.stack([np.ones(N, np.int64), np.arange(N) * 100, np.arange(N) * 100 + 100], axis=1)
    hits = np.zeros(S, np.int32)
    for c in range(C):
        mine = (sample // per) == c
        rows = [(1, int(w) * 100 + int(u), int(w) * 100 + int(u) + 1, "A", "T", int(s), "g", "INDEL" if d else "Missense")
                for s, w, d, u in zip(sample[mine], window[mine], indel[mine], uid[mine])]
        _, loads = OS.sample_loads(idx, rows)
        for s, load in loads.items():
            hits[s] = load
        kept = [r for r in rows if keep[r[5]]]
        assert got_l["labels"][:, c].tolist() == [float(v) for v in OS.window_labels(idx, kept)], c
    assert np.array_equal(got_h["hits"], hits) and hits[0] >= 1


@pytest.mark.parametrize("n", _edge_lengths(1024))
def test_sequence_counts_from_the_pairs_of_a_join(dev, n):
    """dig_sequence_counts (kSeqBlock = 1024) against the statement sequence_counts_statement.sequence_counts, exact:
    tests/test_gpu_sequence_models.py.  Row 0 lies in as many (doubled) windows as the first run is long."""
    import sequence_counts_statement as SS
    K, C = 192, 3
    rng = np.random.default_rng(n + 2)
    run = _first_run(n, 1024)
    rest = n - run                                            # rows 1 .. rest - 1 in one window each; the last row in none
    n_rows = rest + 2
    win_chrom = np.zeros(run + rest, np.int64)
    win_start = np.concatenate([np.zeros(run, np.int64), 100 + 10 * np.arange(rest)])
    win_end = win_start + 10
    row_start = np.concatenate([[5], 100 + 10 * np.arange(rest) + 3, [50]]).astype(np.int64)
    row_type = rng.integers(0, K + 1, n_rows).astype(np.int32)                 # K: no table entry
    row_cohort = np.sort(rng.integers(0, C, n_rows)).astype(np.int32)
    row_type[0], row_cohort[0] = 7, 0
    pair_row = np.concatenate([np.zeros(run, np.int32), 1 + np.arange(rest, dtype=np.int32)])     # mutation-major
    assert len(pair_row) == n
    b = dict(pair_row=arr("i32", pair_row, index=(0, n_rows - 1)), row_type=arr("i32", row_type, index=(0, K)),
             row_cohort=arr("i32", row_cohort, index=(0, C - 1)), counts=out("i64", (C, K)))
    got = guarded("dig_sequence_counts n=%d" % n, b, lambda a: call(a, "dig_sequence_counts", n_pairs=n, n=n_rows, K=K, C=C), dev)
    want = SS.sequence_counts(win_chrom, win_start, win_end, np.zeros(n_rows, np.int64), row_start, row_start + 1, row_type, row_cohort, K, C)
    assert np.array_equal(got["counts"], want) and want[0, 7] >= 1 and want.sum() < n_rows


@pytest.mark.parametrize("n", _edge_lengths(256))
def test_site_match_and_site_counts(dev, n):
    """dig_site_match_count, dig_site_match_keys and dig_site_counts (kSiteBlock = 256) against the statement
    sites_statement.site_counts, exact: tests/test_gpu_sites_cohorts.py.  n matches in all; the first run is (cohort 0, element 0,
    sample 0) = key 0."""
    import sites_statement as ST
    E, C, per, n_sites = 7, 3, 11, 60
    S = C * per
    rng = np.random.default_rng(n + 3)
    site_pos = np.sort((1 << 40) | rng.integers(1000, 1400, n_sites)).astype(np.int64)        # equal positions: the walk over a run
    site_end = site_pos + 1
    site_attr = rng.integers(0, 3, n_sites).astype(np.int64)
    site_elt = rng.integers(0, E, n_sites).astype(np.int32)
    site_elt[0] = 0
    first = (site_pos == site_pos[0]) & (site_attr == site_attr[0])
    site_elt[first] = 0
    site_attr[(site_pos == site_pos[0]) & ~first] = 2 if site_attr[0] != 2 else 1
    m0 = int(first.sum())                                     # matches of a row on site 0
    run = _first_run(n, 256)
    pick = rng.integers(0, n_sites, 4 * n)
    row_pos, row_end, row_attr = site_pos[pick].copy(), site_end[pick].copy(), site_attr[pick].copy()
    row_cohort = rng.integers(0, C, 4 * n).astype(np.int32)
    row_sample = (row_cohort * per + rng.integers(0, per, 4 * n)).astype(np.int32)
    k0 = -(-run // m0)
    row_pos[:k0], row_end[:k0], row_attr[:k0], row_cohort[:k0], row_sample[:k0] = site_pos[0], site_end[0], site_attr[0], 0, 0
    row_attr[k0::9] = -1                                      # matches nothing
    row_end[k0 + 1::13] += 1                                  # another END: no match
    # keep rows until the matches add up to n
    per_row = np.array([int(((site_pos == p) & (site_end == e) & (site_attr == a)).sum()) for p, e, a in zip(row_pos, row_end, row_attr)])
    keep = int(np.searchsorted(np.cumsum(per_row), n, side="left")) + 1
    sl = slice(0, keep)
    row_pos, row_end, row_attr, row_cohort, row_sample, per_row = row_pos[sl], row_end[sl], row_attr[sl], row_cohort[sl], row_sample[sl], per_row[sl]
    while per_row.sum() > n:                                  # trim the overshoot of the last row: make it match nothing
        row_attr[-1], per_row[-1] = -1, 0
        extra = n - per_row.sum()
        if extra:                                             # ... and add rows with single matches
            single = [j for j in range(n_sites) if ((site_pos == site_pos[j]) & (site_attr == site_attr[j])).sum() == 1][:1]
            assert single
            j = single[0]
            row_pos = np.concatenate([row_pos, np.full(extra, site_pos[j])])
            row_end = np.concatenate([row_end, np.full(extra, site_end[j])])
            row_attr = np.concatenate([row_attr, np.full(extra, site_attr[j])])
            row_cohort = np.concatenate([row_cohort, np.full(extra, 1, np.int32)])
            row_sample = np.concatenate([row_sample, np.full(extra, per + 2, np.int32)])
            per_row = np.concatenate([per_row, np.ones(extra, np.int64)])
    n_rows = len(row_pos)
    assert per_row.sum() == n
    off = (np.arange(C + 1) * per).astype(np.int64)
    hi = int(site_pos.max())
    search = dict(site_pos=arr("i64", site_pos, index=(int(site_pos.min()), hi)), site_end=arr("i64", site_end, poison=(0, 5)),
                  site_attr=arr("i64", site_attr, poison=(0, 2)), site_elt=arr("i32", site_elt, index=(0, E - 1)),
                  row_pos=arr("i64", row_pos, poison=(0, hi)), row_end=arr("i64", row_end, poison=(0, 5)), row_attr=arr("i64", row_attr, poison=(0, 2)),
                  row_sample=arr("i32", row_sample, index=(0, S - 1)), row_cohort=arr("i32", row_cohort, index=(0, C - 1)),
                  sample_off=arr("i64", off, index=(0, S)))
    sc = dict(S=n_sites, E=E, n=n_rows, C=C, n_samples=S)
    got = guarded("dig_site_match_count", {**search, "counts": out("i32", n_rows)}, lambda a: call(a, "dig_site_match_count", **sc), dev)
    assert np.array_equal(got["counts"], per_row)
    offsets = (np.cumsum(per_row) - per_row).astype(np.int64)
    got = guarded("dig_site_match_keys", {**search, "offsets": arr("i64", offsets, index=(0, n)), "keys": out("i64", n)},
                  lambda a: call(a, "dig_site_match_keys", total=n, **sc), dev)
    keys = np.sort(got["keys"])
    assert keys[0] == 0 and keys[run - 1] == 0 and (keys >= 0).all()
    b = dict(keys=arr("i64", keys, index=(0, ((C * E - 1) << _bits_for(S)) | (S - 1))), obs_snv=out("i32", (E, C)), obs_samples=out("i32", (E, C)))
    got = guarded("dig_site_counts n=%d" % n, b, lambda a: call(a, "dig_site_counts", total=n, E=E, C=C, n_samples=S), dev)
    want = ST.site_counts(site_pos, site_end, site_attr, site_elt, row_pos, row_end, row_attr, row_sample, row_cohort, off, E, C)
    assert np.array_equal(got["obs_snv"], want["obs_snv"]) and np.array_equal(got["obs_samples"], want["obs_samples"])
    assert want["obs_snv"][0, 0] >= run and want["obs_samples"][0, 0] >= 1


# =====================================================================================================================================
# GP (dig_gp.hip)
# =====================================================================================================================================
@pytest.mark.parametrize("m, n, d", [(5, 300, 1), (37, 1025, 16), (17, 257, 32)])
def test_rbf_cross_and_backward(dev, m, n, d):
    """Values against numpy's direct RBF (rtol 1e-13) and the scalar gradients against the elementwise formulation (rtol 1e-10, atol
    1e-12): tests/test_gp_oracle.py test_rbf_cross_kernels_vs_numpy_and_autograd.  `partial` holds exactly
    dig_rbf_backward_partials(m, n) doubles."""
    rng = np.random.default_rng([m, n, d])
    Z, X, g = rng.normal(size=(m, d)), rng.normal(size=(n, d)), rng.normal(size=(m, n))
    ls, osc = 0.9 + 0.2 * d ** 0.5, 1.7
    got = guarded("dig_rbf_cross", dict(Z=arr("f64", Z), X=arr("f64", X), K=out("f64", (m, n))),
                  lambda a: call(a, "dig_rbf_cross", m=m, n=n, d=d, lengthscale=ls, outputscale=osc), dev)
    d2 = ((Z[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    np.testing.assert_allclose(got["K"], osc * np.exp(-0.5 * d2 / ls ** 2), rtol=1e-13, atol=1e-300)
    K = got["K"]
    n_part = query("dig_rbf_backward_partials", m, n)
    assert n_part == m * ((n + 1023) // 1024) * 2
    b = dict(g=arr("f64", g), K=arr("f64", K), W=out("f64", (m, n)), partial=out("f64", n_part))
    got = guarded("dig_rbf_backward", b, lambda a: call(a, "dig_rbf_backward", m=m, n=n, lengthscale=ls, outputscale=osc), dev)
    np.testing.assert_allclose(got["W"], g * K, rtol=1e-13, atol=1e-300)
    part = got["partial"].reshape(m, -1, 2)
    ref = osc * np.exp(-0.5 * d2 / ls ** 2)
    np.testing.assert_allclose(part[:, :, 0].sum() / osc, (g * ref).sum() / osc, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(part[:, :, 1].sum() / ls ** 3, (g * ref * d2).sum() / ls ** 3, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(part[:, :, 0].sum(1), (g * ref).sum(1), rtol=1e-10, atol=1e-12)


# =====================================================================================================================================
# element-wise entry points: n (or E * C) = 1, 255, 257 with values from the goldens
# =====================================================================================================================================
SIZES = [1, 255, 257]


def _golden(name):
    import os
    from conftest import GOLDEN
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


@pytest.mark.parametrize("n", SIZES)
def test_nb_entry_points(dev, n):
    """The four dig_nb_* on the reference's golden vectors within RTOL: tests/test_gpu_parity.py
    test_nb_midp_upper_golden_host_and_device and test_nb_scalar_siblings_golden."""
    d, e = _golden("nb_midp_golden"), _golden("nb_exact_golden")
    step = len(d["k"]) // n
    sl = slice(0, n * step, step)                             # spread over the whole golden sweep
    for name, src, col in (("dig_nb_midp_upper", d, "pval"), ("dig_nb_exact", e, "pval_exact"), ("dig_nb_greater", e, "pval_greater"),
                           ("dig_nb_midp_twosided", e, "pval_midp")):
        step = len(src["k"]) // n
        sl = slice(0, n * step, step)
        b = dict(k=arr("f64", src["k"][sl]), alpha=arr("f64", src["alpha"][sl]), p=arr("f64", src["p"][sl]), out=out("f64", n))
        got = guarded("%s n=%d" % (name, n), b, lambda a: call(a, name, n=n), dev)
        rel_close(got["out"], src[col][sl], RTOL)


@pytest.mark.parametrize("n", SIZES)
def test_fisher_and_normal_params_to_gamma(dev, n):
    """tests/test_gpu_parity.py test_fisher_and_gamma: Fisher within 1e-12 of the golden, alpha the reference's bits."""
    f, e = _golden("fisher_golden"), _golden("element_stats_golden")
    p1, p2, want = (np.resize(f[k], n) for k in ("p1", "p2", "out"))
    got = guarded("dig_fisher n=%d" % n, dict(p1=arr("f64", p1), p2=arr("f64", p2), out=out("f64", n)), lambda a: call(a, "dig_fisher", n=n), dev)
    rel_close(got["out"], want, 1e-12)
    sl = slice(0, n * 23, 23)
    b = dict(mu=arr("f64", e["mu"][sl]), sigma=arr("f64", e["sigma"][sl]), alpha=out("f64", n), theta=out("f64", n))
    got = guarded("dig_normal_params_to_gamma n=%d" % n, b, lambda a: call(a, "dig_normal_params_to_gamma", n=n), dev)
    assert np.array_equal(got["alpha"], e["out_ALPHA"][sl], equal_nan=True)
    with np.errstate(all="ignore"):
        assert np.array_equal(got["theta"] * float(e["cj"]), e["out_THETA"][sl], equal_nan=True)


@pytest.mark.parametrize("C, nb, nt", [(1, 1, 1), (3, 5, 17), (1, 1, 257)])
def test_tiled_nb_test(dev, C, nb, nt):
    """C * n_bins * n_tiles = 1, 255, 257 with the inputs and bounds of tests/test_gpu_parity.py test_tiled_nb_test_vs_oracle."""
    from oracle import dig_oracle as O
    rng = np.random.default_rng(8)
    mu, sigma = rng.gamma(9.0, 3.0, (C, nb)), rng.gamma(4.0, 1.0, (C, nb))
    pt = rng.dirichlet(np.ones(max(nt, 2)), size=nb)[:, :nt]
    pt[0, :1] = 0.0
    k = rng.poisson(mu[:, :, None] * pt[None] * 1.5).astype(np.int32)
    k[-1, -1, -1] = 40
    b = dict(pt=arr("f64", pt), k=arr("i32", k, poison=(0, 50)), mu=arr("f64", mu), sigma=arr("f64", sigma), pval=out("f64", (C, nb, nt)),
             exp=out("f64", (C, nb, nt)))
    got = guarded("dig_tiled_nb_test", b, lambda a: call(a, "dig_tiled_nb_test", pt_per_cohort=0, C=C, n_bins=nb, n_tiles=nt), dev)
    for c in range(C):
        wp, we = O.tiled_nb_test(pt, k[c], mu[c], sigma[c])
        rel_close(got["pval"][c], wp, RTOL)
        assert np.array_equal(got["exp"][c], we)


@pytest.mark.parametrize("G, C", [(1, 1), (85, 3), (257, 1)])
def test_gene_selection(dev, G, C):
    """G * C = 1, 255, 257 rows of tests/golden/gene_selection_golden.npz with the checks of tests/test_gpu_gene_selection.py
    _check_planes: rel_close 1e-6, the arithmetic planes the reference's bits."""
    from digdriver_amd import _lib
    g = _golden("gene_selection_golden")
    take = np.linspace(0, g["alpha"].shape[0] - 1, G).astype(int)      # regular genes and the edge block
    pi = np.ascontiguousarray(np.broadcast_to(g["pi"][take][:, :, None], (G, 6, C)))
    b = dict(alpha=arr("f64", g["alpha"][take][:, :C]), theta=arr("f64", g["theta"][take][:, :C]), pi=arr("f64", pi),
             obs=arr("i32", g["obs"][take][:, :, :C], poison=(0, 50)), out=out("f64", (34, G, C)))
    got = guarded("dig_gene_selection G=%d C=%d" % (G, C), b, lambda a: call(a, "dig_gene_selection", n_pi=6, G=G, C=C), dev)
    for i, name in enumerate(_lib.SEL_PLANES):
        want = g["planes"][i][take][:, :C]
        rel_close(got["out"][i], want, 1e-6)
        if name in ("T_SYN", "MRFOLD") or name.startswith(("EXP_", "SEL_")):
            assert np.array_equal(got["out"][i], want, equal_nan=True), name


@pytest.mark.parametrize("G, C", [(1, 1), (51, 5), (257, 1)])
def test_gene_stats(dev, G, C):
    """G * C = 1, 255, 257 against oracle.dig_oracle.gene_stats with the inputs and bounds of tests/test_gpu_parity.py
    test_gene_pipeline_all_cohorts_against_oracle (1e-12 for EXP_* and THETA_*, RTOL for the p-values)."""
    from digdriver_amd import engine
    from oracle import dig_oracle as O
    rng = np.random.default_rng([G, C])
    mu = np.exp(rng.uniform(np.log(0.5), np.log(200.0), (G, C)))
    sigma = mu * np.exp(rng.uniform(np.log(0.05), np.log(1.0), (G, C)))
    cj, t_indel = rng.uniform(0.2, 3, C), rng.uniform(0.05, 0.3, C)
    P4 = np.exp(rng.uniform(np.log(1e-4), np.log(0.2), (G, 4, C)))
    pi_indel = np.exp(rng.uniform(np.log(1e-4), np.log(0.2), G))
    alpha, theta = mu ** 2 / sigma ** 2, sigma ** 2 / mu * cj[None, :]
    pi = {"SYN": P4[:, 0], "MIS": P4[:, 1], "NONS": P4[:, 2], "SPL": P4[:, 3]}
    pi["TRUNC"] = pi["NONS"] + pi["SPL"]
    pi["NONSYN"] = pi["MIS"] + pi["TRUNC"]
    obs5 = np.stack([rng.poisson(alpha * theta * pi[c] * 1.2) for c in ("SYN", "MIS", "NONS", "SPL")] +
                    [rng.poisson(alpha * theta * pi_indel[:, None] * 0.1)], axis=1).astype(np.int32)
    obs5[::10, 1] += 400
    obs = {"SYN": obs5[:, 0], "MIS": obs5[:, 1], "NONS": obs5[:, 2], "SPL": obs5[:, 3]}
    obs["TRUNC"] = obs["NONS"] + obs["SPL"]
    obs["NONSYN"] = obs["MIS"] + obs["TRUNC"]
    ns = {c: rng.binomial(obs[c], 0.9) for c in O.GENE_CLASSES}
    n_samp = np.stack([ns[c] for c in O.GENE_CLASSES], axis=1).astype(np.int32)
    want = O.gene_stats(mu, sigma, pi, obs, ns, cj[None, :], pi_indel=pi_indel[:, None], obs_indel=obs5[:, 4], t_indel=t_indel[None, :])
    b = dict(mu=arr("f64", mu), sigma=arr("f64", sigma), pi=arr("f64", P4), pi_indel=arr("f64", pi_indel), obs=arr("i32", obs5, poison=(0, 50)),
             n_samp=arr("i32", n_samp, poison=(0, 50)), cj=arr("f64", cj), t_indel=arr("f64", t_indel), out=out("f64", (22, G, C)))
    got = guarded("dig_gene_stats G=%d C=%d" % (G, C), b,
                  lambda a: call(a, "dig_gene_stats", n_pi=4, per_cohort=0, with_indel=1, G=G, C=C), dev)
    for j, name in enumerate(engine.GS_PLANES):
        rel_close(got["out"][j], want[name], 1e-12 if name.startswith(("EXP", "THETA")) else RTOL)
