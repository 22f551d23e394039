"""The planned rates of the statistics kernel (DIG_PIPE_ELEMENT_RATES): the rate sums MU, SIGMA, R_OBS, FLAG of every (element,
cohort) pair are formed ONCE per plan (dig_element_rates_prepare, engine.PipelinePlan(element_rates=True)) and streamed by
element_stats_stream_fused_kernel<1024, true, 3, REC, true>, against the live form that walks the overlaps and gathers the packed
bin records every call (element_rates=False).  The planned form performs the live form's additions in its order and takes the
same square root, so every comparison here is bit for bit (torch.equal after nan_to_num / np.array_equal): there is no tolerance.

Shapes: about 70 elements over 0, 1, 2, 3 and 12 bins (both sides of the live form's two register slots, and its loop over further
bins); cohort counts that make E * C a multiple of 64 and not; records and planes; the compact and the general accumulation; pairs
parked for each of the three reasons; one problem larger than one pass of the prepare kernel's capped grid."""
import ctypes

import numpy as np
import pytest

import guarded_arena as GA

pytestmark = pytest.mark.gpu

_TABLES = ("bin_mu", "bin_std", "bin_y", "bin_flag", "bin_ctx", "ov_ptr", "ov_idx", "L", "strand_minus", "d_pr")
_OBS = ("obs_snv", "obs_samples", "obs_indel")
_ACC = ("P", "R_SIZE", "ELT_SIZE", "P_INDEL", "MU", "SIGMA", "R_OBS", "FLAG")
_BINS = (0, 1, 2, 3, 12)
RATE_TILE = 64 * 24                       # bytes of the table per 64-pair tile: 64 x {f64 mu, sigma}, then 64 x {i32 R_OBS, FLAG}
E0, N0 = 70, 64
HUGE = N0 - 1                             # the bin row whose rate puts alpha log p below the recurrence's range
PARK_COUNT, PARK_RANGE, PARK_PVALUE = 1, 2, 3          # elements (1, 2 and 3 bins) that carry the hostile pairs


@pytest.fixture(scope="module")
def dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _host_workload(E, C, seed, n_bins=N0, hostile=True):
    """bench.make_workload with the overlaps redrawn: element e overlaps _BINS[e % 5] random bin rows.  hostile: three pairs
    that the statistics kernel has to park, one for each reason (asserted from the outputs in _parked_for_each_reason)."""
    from bench import make_workload
    w = make_workload(n_bins=n_bins, n_elements=E, n_cohorts=C, seed=seed, max_blocks=3)
    rng = np.random.default_rng(seed + 1000)
    cnt = np.array(_BINS)[np.arange(E) % len(_BINS)]
    w["ov_ptr"] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    w["ov_idx"] = rng.integers(0, n_bins - 1, int(w["ov_ptr"][-1])).astype(np.int32)        # (never the HUGE row by chance)
    if E >= 2:
        w["strand_minus"][0], w["strand_minus"][E - 1] = 1, 0
    if hostile:
        w["bin_mu"][HUGE] = 1e7                                          # expected counts of ~1e5: alpha log p ~ -1e5
        w["ov_idx"][w["ov_ptr"][PARK_RANGE]] = HUGE
        for k in _OBS:
            w[k][PARK_RANGE] = 3                                         # (counts of at most 64: the range limit is -400)
        w["obs_snv"][PARK_COUNT, 0], w["obs_samples"][PARK_COUNT, 0] = 300, 290             # above the recurrence's 128
        w["obs_snv"][PARK_PVALUE, 0], w["obs_samples"][PARK_PVALUE, 0] = 120, 3             # far above an expectation of a few
    return w


def _on_device(w, dev):
    import torch
    return {k: torch.as_tensor(v, device=dev) for k, v in w.items() if isinstance(v, np.ndarray)}


@pytest.fixture(scope="module")
def problems(dev):
    """(host arrays, device tensors) per cohort count, built once and left unchanged."""
    return {C: (lambda w: (w, _on_device(w, dev)))(_host_workload(E0, C, 7 * C + 1)) for C in (1, 5, 37, 64, 65)}


def _plan(td, **kw):
    from digdriver_amd import engine
    return engine.PipelinePlan(*[td[k] for k in _TABLES], *[td[k] for k in _OBS], **kw)


def _outputs(plan, run):
    """Every output of one pass as a dict of fresh tensors: the eight accumulation outputs, the seven planes and, for a
    record plan, the records themselves (padding included)."""
    import torch
    for v in list(plan.acc.values()) + [plan.stats] + ([plan.out_records] if plan.records_out else []):
        v.fill_(-3)                                       # a stale right answer of the run before cannot pass for this one
    run(plan)
    acc, st = plan.unpack() if plan.records_out else (plan.acc, plan.stats)
    torch.cuda.synchronize()
    res = {k: acc[k].clone() for k in _ACC}
    res.update({"plane%d" % j: st[j].clone() for j in range(st.shape[0])})
    if plan.records_out:
        res["records"] = plan.out_records.clone()
    assert st.shape[0] == 7
    return res


def _same_bits(a, b, what):
    import torch
    assert set(a) == set(b)
    for k in a:
        x, y = a[k], b[k]
        if x.dtype.is_floating_point:
            x, y = x.view(torch.int64), y.view(torch.int64)
        assert torch.equal(x, y), (what, k)


def _whole(td):
    return lambda plan: plan.run(td["cj"], td["cj_indel"])


def _parked_for_each_reason(w, res):
    """From the outputs themselves: a count above 128; counts inside the recurrence's reach (<= 64) with alpha log p below its
    range (-400); counts <= 128 in range with a p-value below 10^-6 (where 1 - CDF cancels)."""
    mu, sg = res["MU"].cpu().numpy(), res["SIGMA"].cpu().numpy()
    P = res["P"].cpu().numpy().reshape(mu.shape)
    pv = res["plane1"].cpu().numpy()
    with np.errstate(all="ignore"):
        alpha, theta = mu ** 2 / sg ** 2, sg ** 2 / mu * w["cj"][None, :]
        lp0 = alpha * -np.log1p(theta * P)
    kmax = np.maximum(w["obs_snv"], w["obs_samples"])
    assert (w["obs_snv"] > 128).any(), "no count above 128"
    assert ((kmax <= 64) & (lp0 < -1000)).any(), "no pair below the recurrence's range"
    assert ((kmax <= 128) & (lp0 > -100) & (pv < 1e-6) & (pv >= 0)).any(), "no p-value below 1e-6 from a count the recurrence reaches"


# ---- 1. same bits, planned against live -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 5, 37, 64, 65])
def test_planned_rates_give_the_bits_of_the_live_form(dev, problems, C):
    from digdriver_amd import _lib
    w, td = problems[C]
    assert sorted(set(np.diff(w["ov_ptr"]))) == list(_BINS) and ((E0 * C) % 64 == 0) == (C == 64)
    for compact in ("auto", False):
        for rec in (False, True):
            live = _plan(td, element_rates=False, records_out=rec, compact=compact)
            planned = _plan(td, element_rates=True, records_out=rec, compact=compact)
            assert live.compact == planned.compact == (compact == "auto")
            assert live.elt_rates is None and not live._flags & _lib.DIG_PIPE_ELEMENT_RATES
            assert planned.elt_rates is not None and planned._flags & _lib.DIG_PIPE_ELEMENT_RATES
            assert planned.elt_rates.numel() == (E0 * C + 63) // 64 * RATE_TILE
            want = _outputs(live, _whole(td))
            _same_bits(_outputs(planned, _whole(td)), want, (C, compact, rec))
            if C == 37 or C == 5:
                _parked_for_each_reason(w, want)
            empty = np.flatnonzero(np.diff(w["ov_ptr"]) == 0)
            for k in ("MU", "SIGMA", "R_OBS", "FLAG"):                      # an element without bins gives 0, 0, 0, 0
                assert not want[k][empty].any()


def test_a_plan_without_packed_records_ignores_the_option(dev, problems):
    from digdriver_amd import _lib
    w, td = problems[5]
    plain = _plan(td, pack_bins=False)
    assert plain.records is None and plain.elt_rates is None and not plain._flags & _lib.DIG_PIPE_ELEMENT_RATES
    _same_bits(_outputs(plain, _whole(td)), _outputs(_plan(td), _whole(td)), "no records")


def test_default_is_planned_and_one_shot_callers_sum_live(dev, problems):
    from digdriver_amd import _lib, parallel
    w, td = problems[5]
    assert _plan(td)._flags & _lib.DIG_PIPE_ELEMENT_RATES
    import inspect
    from digdriver_amd import engine
    from digdriver_amd.driver_model import cohort_batch
    assert "element_rates=False" in inspect.getsource(engine.element_pipeline)
    assert "element_rates=False" in inspect.getsource(cohort_batch._element_planes)
    assert "element_rates" not in inspect.getsource(parallel.ShardedPipeline)


# ---- 2. the table itself ----------------------------------------------------------------------------------------------------------
def _table_numpy(w, E, C):
    """The table as the reference forms its sums (genic_driver_tools.py:262-271), one addition after the other in CSR order:
    bin j of every element that has one is added in round j.  (mu, sigma [slots], robs, flag [slots]); slots past E C repeat the last."""
    ptr, idx = w["ov_ptr"], w["ov_idx"]
    cnt = np.diff(ptr)
    mu, var = np.zeros((E, C)), np.zeros((E, C))
    robs, flag = np.zeros((E, C), np.int32), np.zeros((E, C), np.int32)
    sq = w["bin_std"] * w["bin_std"]
    for j in range(int(cnt.max()) if E else 0):
        has = np.flatnonzero(cnt > j)
        rows = idx[ptr[has] + j]
        mu[has] = mu[has] + w["bin_mu"][rows]
        var[has] = var[has] + sq[rows]
        robs[has] = robs[has] + w["bin_y"][rows]
        flag[has] |= (w["bin_flag"][rows] != 0)
    slots = (E * C + 63) // 64 * 64
    pad = lambda x: np.concatenate([x.ravel(), np.repeat(x.ravel()[-1:], slots - E * C)])
    return pad(mu), pad(np.sqrt(var)), pad(robs), pad(flag)


def _table_fields(raw, E, C):
    tiles = np.ascontiguousarray(raw).reshape(-1, RATE_TILE)
    assert tiles.shape[0] == (E * C + 63) // 64
    ms = tiles[:, :1024].copy().view(np.float64).reshape(-1, 64, 2)
    rf = tiles[:, 1024:].copy().view(np.int32).reshape(-1, 64, 2)
    return ms[:, :, 0].ravel(), ms[:, :, 1].ravel(), rf[:, :, 0].ravel(), rf[:, :, 1].ravel()


def _assert_table(raw, w, E, C):
    for got, want, name in zip(_table_fields(raw, E, C), _table_numpy(w, E, C), ("mu", "sigma", "r_obs", "flag")):
        assert GA.same_bits(got, want.astype(got.dtype)), name


@pytest.mark.parametrize("C", [5, 64])
def test_table_against_numpy_with_rates_of_every_magnitude(dev, C):
    """Bin rates over sixteen decades: the order of the additions shows in the last bits."""
    w = _host_workload(E0, C, 90 + C)
    rng = np.random.default_rng(C)
    w["bin_mu"] = np.exp(rng.uniform(-18, 18, w["bin_mu"].shape))
    w["bin_std"] = np.exp(rng.uniform(-9, 9, w["bin_std"].shape))
    td = _on_device(w, dev)
    plan = _plan(td)
    import torch
    torch.cuda.synchronize()
    _assert_table(plan.elt_rates.cpu().numpy(), w, E0, C)
    # the check can tell orders apart: the twelve-bin elements summed last bin first differ from first to last somewhere
    mu = _table_numpy(w, E0, C)[0][:E0 * C].reshape(E0, C)
    twelve = np.flatnonzero(np.diff(w["ov_ptr"]) == 12)
    backwards = np.zeros((len(twelve), C))
    for j in range(11, -1, -1):
        backwards = backwards + w["bin_mu"][w["ov_idx"][w["ov_ptr"][twelve] + j]]
    assert not np.array_equal(backwards, mu[twelve])


def test_prepare_past_its_grid_cap(dev):
    """256 threads a workgroup, at most 8 workgroups per CU on 256 CUs: 524 288 slots in one pass of the grid.  8 200 elements
    x 65 cohorts are 533 000 pairs: the walk takes a second step, the last tile is ragged."""
    E, C = 8200, 65
    assert E * C > 256 * 8 * 256 and (E * C) % 64
    w = _host_workload(E, C, 11, n_bins=500, hostile=False)
    td = _on_device(w, dev)
    planned = _plan(td)
    import torch
    torch.cuda.synchronize()
    _assert_table(planned.elt_rates.cpu().numpy(), w, E, C)
    _same_bits(_outputs(planned, _whole(td)), _outputs(_plan(td, element_rates=False), _whole(td)), "past the grid cap")


# ---- 3. plan methods ----------------------------------------------------------------------------------------------------------------
def test_repack_bins_and_recontext_rebuild_the_table(dev):
    import torch
    w = _host_workload(E0, 37, 21)
    td = _on_device(w, dev)
    planned = _plan(td)
    shared = _plan(td, pack_bins=planned, element_rates=planned)          # another plan may share the table
    assert shared.elt_rates is planned.elt_rates
    before = _outputs(planned, _whole(td))
    _same_bits(_outputs(shared, _whole(td)), before, "shared table")
    # a bin table changes in place: the snapshot is what is read until repack_bins()
    td["bin_mu"].mul_(1.25)
    td["bin_y"].add_(1)
    torch.cuda.synchronize()
    _same_bits(_outputs(planned, _whole(td)), before, "the snapshot is what is read")
    fresh = _outputs(_plan(td), _whole(td))
    assert not torch.equal(fresh["MU"], before["MU"]) and not torch.equal(fresh["R_OBS"], before["R_OBS"])
    _same_bits(fresh, _outputs(_plan(td, element_rates=False), _whole(td)), "fresh plans")
    planned.repack_bins()
    _same_bits(_outputs(planned, _whole(td)), fresh, "after repack_bins()")
    # the overlaps change in place: recontext()
    td["ov_idx"].copy_((td["ov_idx"] + 5) % (N0 - 1))
    torch.cuda.synchronize()
    fresh2 = _outputs(_plan(td), _whole(td))
    assert not torch.equal(fresh2["MU"], fresh["MU"])
    _same_bits(fresh2, _outputs(_plan(td, element_rates=False), _whole(td)), "fresh plans, new overlaps")
    planned.recontext()
    _same_bits(_outputs(planned, _whole(td)), fresh2, "after recontext()")


@pytest.mark.parametrize("rec", [False, True], ids=["planes", "records"])
def test_statistics_only_call_with_new_scale_factors(dev, problems, rec):
    from digdriver_amd import _lib
    w, td = problems[37]
    cj2, cji2 = td["cj"] * 1.7, td["cj_indel"] * 0.6

    def again(plan):
        plan.run(td["cj"], td["cj_indel"])
        return plan.run(cj2, cji2, stages=_lib.DIG_PIPE_STATISTICS)
    planned, live = _plan(td, records_out=rec), _plan(td, element_rates=False, records_out=rec)
    got, want = _outputs(planned, again), _outputs(live, again)
    _same_bits(got, want, "statistics-only call")
    assert not np.array_equal(want["plane0"].cpu().numpy(), _outputs(live, _whole(td))["plane0"].cpu().numpy())


def _restore_lc(plan):
    from digdriver_amd import _lib
    ok = ctypes.c_int(0)
    _lib.call("dig_element_pipeline_prepare", _lib.dev_ptr(plan.keep[7]), plan.E, plan.C, plan._ws, plan.wsb, ctypes.byref(ok), _lib.stream_ptr())
    assert ok.value == 1


def test_plan_on_a_side_stream_while_the_default_stream_is_busy(dev, problems):
    w, td = problems[37]
    planned = _plan(td)
    assert planned.compact and planned.elt_rates is not None
    GA.side_stream_call(lambda stream: planned.run(td["cj"], td["cj_indel"], stream=stream), dev, "planned-rates PipelinePlan.run",
                        explicit=True, scratch=[planned.ws], restore=lambda: _restore_lc(planned))


# ---- 4. guard bands ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [5, 64])
def test_guarded_calls(dev, C):
    """pack, dig_element_rates_prepare and the pipeline with DIG_PIPE_ELEMENT_RATES, every pointer carved from a guarded arena at
    its documented alignment: the table at exactly dig_element_rates_bytes (the clamped loads of tiles past the end stay inside
    it), the workspace at exactly its size, ov_idx with valid rows as poison around it."""
    from digdriver_amd import _lib
    E = 33
    w = _host_workload(E, C, 60 + C)
    N, nnz = w["bin_mu"].shape[0], len(w["ov_idx"])
    lib = _lib.load()
    need, nrec, nrate = (int(lib.dig_element_pipeline_workspace(E, C)), int(lib.dig_bin_records_bytes(N, C)),
                         int(lib.dig_element_rates_bytes(E, C)))
    assert nrate == (E * C + 63) // 64 * RATE_TILE
    arr = lambda dtype, data, **kw: GA.inp(dtype, np.ascontiguousarray(data, GA._NP[dtype]), **kw)
    b = dict(bin_mu=arr("f64", w["bin_mu"]), bin_std=arr("f64", w["bin_std"]), bin_y=arr("i32", w["bin_y"], poison=(0, 9)),
             bin_flag=arr("u8", w["bin_flag"]), bin_ctx=arr("i32", w["bin_ctx"], poison=(0, 9)),
             ov_ptr=arr("i64", w["ov_ptr"], index=(0, nnz)), ov_idx=arr("i32", w["ov_idx"], index=(0, N - 1)),
             L=arr("i32", w["L"], poison=(0, 3)), strand_minus=arr("u8", w["strand_minus"]), d_pr=arr("f64", w["d_pr"]),
             obs_snv=arr("i32", w["obs_snv"], poison=(0, 50)), obs_samples=arr("i32", w["obs_samples"], poison=(0, 50)),
             obs_indel=arr("i32", w["obs_indel"], poison=(0, 50)), cj=arr("f64", w["cj"]), cj_indel=arr("f64", w["cj_indel"]),
             records=GA.ws(nrec, align=256), rates=GA.out("u8", (nrate,), align=256),
             MU=GA.out("f64", (E, C)), SIGMA=GA.out("f64", (E, C)), R_OBS=GA.out("i32", (E, C)), FLAG=GA.out("i32", (E, C)),
             P=GA.out("f64", (E, 1, C)), R_SIZE=GA.out("i32", E), ELT_SIZE=GA.out("i32", E), P_INDEL=GA.out("f64", E),
             out=GA.out("f64", (7, E, C)), ws=GA.ws(need, align=256))

    def invoke(a, planned=True):
        p, s = a.ptr, _lib.stream_ptr()
        ok = ctypes.c_int(0)
        _lib.call("dig_element_pipeline_prepare", p("L"), E, C, p("ws"), need, ctypes.byref(ok), s)
        assert ok.value == 1
        _lib.call("dig_bin_records_pack", p("bin_mu"), p("bin_std"), p("bin_y"), p("bin_flag"), N, C, p("records"), nrec, s)
        _lib.call("dig_element_rates_prepare", p("records"), p("ov_ptr"), p("ov_idx"), N, E, C, p("rates"), nrate, s)
        _lib.call("dig_element_pipeline", p("rates" if planned else "bin_mu"), p("bin_std"), p("bin_y"), p("bin_flag"), p("bin_ctx"),
                  p("ov_ptr"), p("ov_idx"), p("L"), p("strand_minus"), None, p("d_pr"), p("obs_snv"), p("obs_samples"), p("obs_indel"),
                  p("cj"), p("cj_indel"), p("MU"), p("SIGMA"), p("R_OBS"), p("FLAG"), p("P"), p("R_SIZE"), p("ELT_SIZE"), p("P_INDEL"),
                  p("out"), N, E, C, p("records"), 7 | _lib.DIG_PIPE_COMPACT_L | (_lib.DIG_PIPE_ELEMENT_RATES if planned else 0), p("ws"),
                  need, s)

    got = GA.guarded_runs(b, invoke, device=dev, what="dig_element_pipeline with planned rates C=%d" % C, plain=True)
    _assert_table(got["rates"], w, E, C)
    live = GA.PlainBuffers(b, dev)
    invoke(live, planned=False)
    live.assert_intact()
    for name in got:
        assert GA.same_bits(got[name], live.read(name)), name
