"""The planned form of the compact dot kernel (DIG_PIPE_ELEMENT_CTX): the elements' context rows are summed ONCE per plan
(dig_element_contexts_prepare, engine.PipelinePlan(element_contexts=True)) and streamed by acc_dot_ctx_kernel<NT, NQ, true>,
against the live form that walks the overlaps and gathers the bin rows every call (element_contexts=False).  The sums are
integers, so every comparison here is bit for bit (torch.equal after nan_to_num / np.array_equal): there is no tolerance.

Shapes: cohort counts on both sides of every (tiles, quads) cut and a second 48-cohort chunk; element counts around one
16-row tile, several tiles, and past one pass of the capped grid; elements over 0 ... 12 bins; both strands."""
import ctypes

import numpy as np
import pytest

import guarded_arena as GA

pytestmark = pytest.mark.gpu

_TABLES = ("bin_mu", "bin_std", "bin_y", "bin_flag", "bin_ctx", "ov_ptr", "ov_idx", "L", "strand_minus", "d_pr")
_OBS = ("obs_snv", "obs_samples", "obs_indel")
_ACC = ("P", "R_SIZE", "ELT_SIZE", "P_INDEL", "MU", "SIGMA", "R_OBS", "FLAG")


@pytest.fixture(scope="module")
def dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _without_bins(w, elements):
    """The workload with the CSR rows of `elements` emptied (rates 0, P = 0 / 0 or x / 0 as the reference forms them)."""
    ptr = w["ov_ptr"]
    keep = np.ones(len(w["ov_idx"]), bool)
    cnt = np.diff(ptr)
    for e in elements:
        keep[ptr[e]:ptr[e + 1]] = False
        cnt[e] = 0
    w["ov_idx"] = w["ov_idx"][keep]
    w["ov_ptr"] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    return w


def _workload(dev, nb, E, C, seed, mb, empty=()):
    import torch
    from bench import make_workload
    w = make_workload(n_bins=nb, n_elements=E, n_cohorts=C, seed=seed, max_blocks=mb)
    if E >= 2:                                            # both strands, whatever the draw
        w["strand_minus"][0], w["strand_minus"][E - 1] = 1, 0
    w = _without_bins(w, empty)
    td = {k: torch.as_tensor(v, device=dev) for k, v in w.items() if isinstance(v, np.ndarray)}
    if len(w["ov_idx"]) == 0:                             # an empty CSR: ov_ptr all zero in front of a pointer that is not null (an empty
        td["ov_idx"] = torch.zeros(1, dtype=torch.int32, device=dev)     # tensor has none), as the host backend stages it
    return w, td


def _plan(td, **kw):
    from digdriver_amd import engine
    plan = engine.PipelinePlan(*[td[k] for k in _TABLES], *[td[k] for k in _OBS], **kw)
    assert plan.compact, "make_workload repeats every context count three times"
    return plan


def _outputs(plan, run):
    """Every output of one pass as a dict of fresh tensors: the eight accumulation outputs and the seven planes."""
    import torch
    for v in list(plan.acc.values()) + [plan.stats] + ([plan.out_records] if plan.records_out else []):
        v.fill_(-3)                                       # a stale right answer of the run before cannot pass for this one
    run(plan)
    acc, st = plan.unpack() if plan.records_out else (plan.acc, plan.stats)
    torch.cuda.synchronize()
    res = {k: acc[k].clone() for k in _ACC}
    res.update({"plane%d" % j: st[j].clone() for j in range(st.shape[0])})
    assert st.shape[0] == 7
    return res


def _same_bits(a, b, what):
    import torch
    assert set(a) == set(b)
    for k in a:
        x, y = a[k], b[k]
        if x.dtype.is_floating_point:
            x, y = torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0)
        assert torch.equal(x, y), (what, k)


def _whole(td):
    return lambda plan: plan.run(td["cj"], td["cj_indel"])


# ---- 1. same bits, planned against live -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 5, 16, 17, 37, 48, 49, 104])
def test_planned_form_gives_the_bits_of_the_live_form(dev, C):
    from digdriver_amd import _lib
    for E in (1, 15, 16, 17, 333, 1601):
        for mb in (1, 3, 12):
            empty = sorted({E // 3, E // 2, E - 1}) if E >= 15 else ()      # three elements without bins, the last one among them
            w, td = _workload(dev, max(64, E // 2), E, C, 100 * C + E + mb, mb, empty)
            assert E < 2 or (w["strand_minus"].min() == 0 and w["strand_minus"].max() == 1)
            assert E < 15 or (np.diff(w["ov_ptr"]) == 0).sum() >= 3 and w["ov_ptr"][-1] == w["ov_ptr"][-2]
            for rec in (False, True):
                live = _plan(td, element_contexts=False, records_out=rec)
                planned = _plan(td, element_contexts=True, records_out=rec)
                assert live.elt_ctx is None and not live._flags & _lib.DIG_PIPE_ELEMENT_CTX
                assert planned.elt_ctx is not None and planned._flags & _lib.DIG_PIPE_ELEMENT_CTX
                _same_bits(_outputs(planned, _whole(td)), _outputs(live, _whole(td)), (C, E, mb, rec))
    assert np.diff(w["ov_ptr"]).max() > 2, "max_blocks = 12 must reach the live form's loop over further bins"


@pytest.mark.parametrize("rec", [False, True], ids=["planes", "records"])
def test_planned_form_with_an_empty_csr(dev, rec):
    E, C = 17, 5
    w, td = _workload(dev, 64, E, C, 5, 3, empty=range(E))
    assert len(w["ov_idx"]) == 0 and not w["ov_ptr"].any() and td["ov_idx"].data_ptr() != 0
    planned = _plan(td, element_contexts=True, records_out=rec)
    assert not planned.elt_ctx.any()
    _same_bits(_outputs(planned, _whole(td)), _outputs(_plan(td, element_contexts=False, records_out=rec), _whole(td)), "empty CSR")


# ---- 2. the table itself ----------------------------------------------------------------------------------------------------------
def _revcomp_map():
    j = np.arange(64)
    t, k, u = j >> 4, (j >> 2) & 3, j & 3
    return 16 * (3 - u) + 4 * (3 - k) + (3 - t)


def _table_numpy(bin_ctx, ov_ptr, ov_idx, strand_minus):
    E = len(ov_ptr) - 1
    want = np.zeros((E, 64), np.int64)
    full = np.flatnonzero(np.diff(ov_ptr) > 0)
    if len(full):
        want[full] = np.add.reduceat(bin_ctx[ov_idx].astype(np.int64), ov_ptr[full], axis=0)
    minus = strand_minus.astype(bool)
    want[minus] = want[minus][:, _revcomp_map()]
    assert np.abs(want).max() < 2 ** 31
    return want.astype(np.int32)


def test_table_against_numpy_with_twelve_bins_and_sums_near_two_to_the_31(dev):
    import torch
    from digdriver_amd import _lib
    rng = np.random.default_rng(12)
    N, E = 40, 50
    bin_ctx = rng.integers(160_000_000, 178_000_000, (N, 64)).astype(np.int32)      # 12 x 1.78e8 = 2.136e9 < 2^31 = 2.147e9
    cnt = rng.integers(0, 13, E)
    cnt[[7, E - 1]] = 12
    cnt[[0, 20]] = 0
    ov_ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    ov_idx = rng.integers(0, N, int(ov_ptr[-1])).astype(np.int32)
    ov_idx[ov_ptr[7]:ov_ptr[8]] = N - 1                                             # the largest sums: twelve times the last row
    strand = (np.arange(E) % 2).astype(np.uint8)
    want = _table_numpy(bin_ctx, ov_ptr, ov_idx, strand)
    assert want.max() > 1.9e9
    t = [torch.as_tensor(x, device=dev) for x in (bin_ctx, ov_ptr, ov_idx, strand)]
    got = torch.full((E, 64), -5, dtype=torch.int32, device=dev)
    _lib.call("dig_element_contexts_prepare", *[_lib.dev_ptr(x) for x in t], N, E, _lib.dev_ptr(got), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("E,mb", [(17, 3), (1601, 12)])
def test_table_is_the_one_the_general_form_leaves_in_its_workspace(dev, E, mb):
    import torch
    from digdriver_amd import engine
    w, td = _workload(dev, 300, E, 5, 77 + E, mb, empty=(2, E // 2, E - 1))
    planned = _plan(td)
    general = engine.PipelinePlan(*[td[k] for k in _TABLES], *[td[k] for k in _OBS], compact=False)
    assert not general.compact and general.elt_ctx is None
    general.run(td["cj"], td["cj_indel"], stages=1)
    torch.cuda.synchronize()
    rcp = general.ws[:E * 256].view(torch.int32).reshape(E, 64)
    assert torch.equal(planned.elt_ctx, rcp)
    assert np.array_equal(rcp.cpu().numpy(), _table_numpy(w["bin_ctx"], w["ov_ptr"], w["ov_idx"], w["strand_minus"]))


# ---- 3. more than one tile per wave, a ragged end ------------------------------------------------------------------------------
def test_more_than_one_tile_per_wave_and_a_ragged_end(dev):
    """The grid is capped at the CU count (256) and a workgroup has 12 waves of 16-element tiles: E = 16 * 12 * 256 * 2 + 17
    gives every wave two tiles and some a third, the last tile one row."""
    E = 16 * 12 * 256 * 2 + 17
    w, td = _workload(dev, 5000, E, 5, 3, 3, empty=(5, E - 1))
    _same_bits(_outputs(_plan(td, element_contexts=True), _whole(td)), _outputs(_plan(td, element_contexts=False), _whole(td)), E)


# ---- 4. stages and streams --------------------------------------------------------------------------------------------------------
def _restore_lc(plan):
    from digdriver_amd import _lib
    ok = ctypes.c_int(0)
    _lib.call("dig_element_pipeline_prepare", _lib.dev_ptr(plan.keep[7]), plan.E, plan.C, plan._ws, plan.wsb, ctypes.byref(ok), _lib.stream_ptr())
    assert ok.value == 1


def _in_stages(td, stream=None):
    from digdriver_amd import _lib

    def run(plan):
        plan.run(td["cj"], td["cj_indel"], stages=_lib.DIG_PIPE_CONTEXTS, stream=stream)
        plan.run(td["cj"], td["cj_indel"], stages=_lib.DIG_PIPE_DOT, stream=stream)
        return plan.run(td["cj"], td["cj_indel"], stages=_lib.DIG_PIPE_STATISTICS | _lib.DIG_PIPE_WORKLIST_CLEAN, stream=stream)
    return run


def test_stages_as_three_calls_and_a_poisoned_workspace(dev):
    import torch
    w, td = _workload(dev, 900, 333, 37, 41, 3, empty=(3, 11, 332))
    planned, live = _plan(td, element_contexts=True), _plan(td, element_contexts=False)
    one = _outputs(planned, _whole(td))
    _same_bits(one, _outputs(live, _whole(td)), "one call")
    _same_bits(_outputs(planned, _in_stages(td)), one, "three calls")
    # the table is plan-owned memory outside the workspace: poison the workspace, restore only Lc, same bits
    assert not (planned.ws.data_ptr() <= planned.elt_ctx.data_ptr() < planned.ws.data_ptr() + planned.ws.numel())
    planned.ws.fill_(85)
    _restore_lc(planned)
    torch.cuda.synchronize()
    _same_bits(_outputs(planned, _whole(td)), one, "after the workspace was overwritten")


def test_stages_on_a_side_stream_while_the_default_stream_is_busy(dev):
    import torch
    w, td = _workload(dev, 900, 333, 37, 42, 3, empty=(3, 11, 332))
    planned = _plan(td, element_contexts=True)
    whole = [GA._host_copy(torch, x) for x in planned.run(td["cj"], td["cj_indel"])]
    torch.cuda.synchronize()
    ref = GA.side_stream_call(lambda stream: _in_stages(td, stream)(planned), dev, "planned PipelinePlan.run in three stages", explicit=True,
                              scratch=[planned.ws], restore=lambda: _restore_lc(planned))
    one = GA._flatten(whole, "", {})
    assert set(one) == set(ref) and all(GA.same_bits(one[k], ref[k]) for k in one)
    GA.side_stream_call(lambda stream: planned.run(td["cj"], td["cj_indel"], stream=stream), dev, "planned PipelinePlan.run", explicit=True,
                        scratch=[planned.ws], restore=lambda: _restore_lc(planned))


# ---- 5. recontext() ---------------------------------------------------------------------------------------------------------------
def test_recontext_rebuilds_the_snapshot(dev):
    import torch
    w, td = _workload(dev, 400, 333, 17, 51, 6)
    planned = _plan(td, element_contexts=True)
    shared = _plan(td, element_contexts=planned)                       # another plan may share the table
    assert shared.elt_ctx is planned.elt_ctx
    before = _outputs(planned, _whole(td))
    _same_bits(_outputs(shared, _whole(td)), before, "shared table")
    td["bin_ctx"].add_(torch.arange(td["bin_ctx"].numel(), device=dev, dtype=torch.int32).reshape(td["bin_ctx"].shape) % 7 + 1)
    torch.cuda.synchronize()
    _same_bits(_outputs(planned, _whole(td)), before, "the snapshot is what is read")
    fresh = _outputs(_plan(td, element_contexts=True), _whole(td))
    assert not torch.equal(fresh["R_SIZE"], before["R_SIZE"])
    _same_bits(fresh, _outputs(_plan(td, element_contexts=False), _whole(td)), "fresh plans")
    planned.recontext()
    _same_bits(_outputs(planned, _whole(td)), fresh, "after recontext()")


# ---- 6. guard bands ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [17, 33])
def test_guarded_calls(dev, E):
    """prepare, dig_element_contexts_prepare and the planned pipeline with every pointer carved from a guarded arena at its
    documented alignment: the table at exactly [E, 64] (the replayed last row of tiles past the end stays inside it), the
    workspace at exactly its size, ov_idx / bin_ctx with valid rows as poison around them."""
    from bench import make_workload
    from digdriver_amd import _lib
    C = 5
    w = _without_bins(make_workload(n_bins=900, n_elements=E, n_cohorts=C, seed=60 + E, max_blocks=12), (4, E - 1))
    N, nnz = w["bin_mu"].shape[0], len(w["ov_idx"])
    arr = lambda dtype, data, **kw: GA.inp(dtype, np.ascontiguousarray(data, GA._NP[dtype]), **kw)
    need = int(_lib.load().dig_element_pipeline_workspace(E, C))
    b = dict(bin_mu=arr("f64", w["bin_mu"]), bin_std=arr("f64", w["bin_std"]), bin_y=arr("i32", w["bin_y"], poison=(0, 9)),
             bin_flag=arr("u8", w["bin_flag"]), bin_ctx=arr("i32", w["bin_ctx"], poison=(0, 9)),
             ov_ptr=arr("i64", w["ov_ptr"], index=(0, nnz)), ov_idx=arr("i32", w["ov_idx"], index=(0, N - 1)),
             L=arr("i32", w["L"], poison=(0, 3)), strand_minus=arr("u8", w["strand_minus"]), d_pr=arr("f64", w["d_pr"]),
             obs_snv=arr("i32", w["obs_snv"], poison=(0, 50)), obs_samples=arr("i32", w["obs_samples"], poison=(0, 50)),
             obs_indel=arr("i32", w["obs_indel"], poison=(0, 50)), cj=arr("f64", w["cj"]), cj_indel=arr("f64", w["cj_indel"]),
             elt_ctx=GA.out("i32", (E, 64), align=256),
             MU=GA.out("f64", (E, C)), SIGMA=GA.out("f64", (E, C)), R_OBS=GA.out("i32", (E, C)), FLAG=GA.out("i32", (E, C)),
             P=GA.out("f64", (E, 1, C)), R_SIZE=GA.out("i32", E), ELT_SIZE=GA.out("i32", E), P_INDEL=GA.out("f64", E),
             out=GA.out("f64", (7, E, C)), ws=GA.ws(need, align=256))

    def invoke(a, planned=True):
        p, s = a.ptr, _lib.stream_ptr()
        ok = ctypes.c_int(0)
        _lib.call("dig_element_pipeline_prepare", p("L"), E, C, p("ws"), need, ctypes.byref(ok), s)
        assert ok.value == 1
        if planned:
            _lib.call("dig_element_contexts_prepare", p("bin_ctx"), p("ov_ptr"), p("ov_idx"), p("strand_minus"), N, E, p("elt_ctx"), s)
        _lib.call("dig_element_pipeline", p("bin_mu"), p("bin_std"), p("bin_y"), p("bin_flag"), p("elt_ctx" if planned else "bin_ctx"),
                  p("ov_ptr"), p("ov_idx"), p("L"), p("strand_minus"), None, p("d_pr"), p("obs_snv"), p("obs_samples"), p("obs_indel"),
                  p("cj"), p("cj_indel"), p("MU"), p("SIGMA"), p("R_OBS"), p("FLAG"), p("P"), p("R_SIZE"), p("ELT_SIZE"), p("P_INDEL"),
                  p("out"), N, E, C, None, 7 | _lib.DIG_PIPE_COMPACT_L | (_lib.DIG_PIPE_ELEMENT_CTX if planned else 0), p("ws"), need, s)

    got = GA.guarded_runs(b, invoke, device=dev, what="planned dig_element_pipeline E=%d" % E, plain=True)
    assert np.array_equal(got["elt_ctx"], _table_numpy(w["bin_ctx"], w["ov_ptr"], w["ov_idx"], w["strand_minus"]))
    live = GA.PlainBuffers(b, dev)
    invoke(live, planned=False)
    live.assert_intact()
    for name in got:
        if name != "elt_ctx":
            assert GA.same_bits(got[name], live.read(name)), name
