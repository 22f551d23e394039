"""The planned P of the pipeline (DIG_PIPE_ELEMENT_P): P, R_SIZE, ELT_SIZE and P_INDEL depend on nothing a run() is given, so a
plan runs its own accumulation form ONCE, keeps bit copies of the four outputs in one table (dig_element_p_prepare,
engine.PipelinePlan(element_p=True)) and the DOT stage of every later call is element_p_stream_kernel, which writes them back into
the caller's outputs -- against the live form that forms them every call (element_p=False).  The table holds copies, so every
comparison here is bit for bit (floats as int64 views): there is no tolerance.

Shapes: about 70 elements over 0, 1, 2, 3 and 12 bins (0 bins: the NaN / inf P of zero denominators), both strands; cohort counts
on both sides of the 48-cohort chunk, with E * C a multiple of 64 only at C = 64; an L that repeats (compact form) and one that
does not (general form); records and planes; a P that is 8- but not 16-byte aligned; one problem past one step of the copy
kernels' capped grid."""
import ctypes

import numpy as np
import pytest

import guarded_arena as GA

pytestmark = pytest.mark.gpu

_TABLES = ("bin_mu", "bin_std", "bin_y", "bin_flag", "bin_ctx", "ov_ptr", "ov_idx", "L", "strand_minus", "d_pr")
_OBS = ("obs_snv", "obs_samples", "obs_indel")
_ACC = ("P", "R_SIZE", "ELT_SIZE", "P_INDEL", "MU", "SIGMA", "R_OBS", "FLAG")
_KEPT = ("P", "P_INDEL", "R_SIZE", "ELT_SIZE")            # the table's sections, in its order
_BINS = (0, 1, 2, 3, 12)
E0, N0 = 70, 64
CS = (1, 5, 37, 64, 65)


@pytest.fixture(scope="module")
def dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _host_workload(E, C, seed, n_bins=N0, repeat=True):
    """bench.make_workload with the overlaps redrawn: element e overlaps _BINS[e % 5] random bin rows.  repeat=False: one count of
    L differs from the two others of its context, so the plan-time check refuses the compact form and the general one runs."""
    from bench import make_workload
    w = make_workload(n_bins=n_bins, n_elements=E, n_cohorts=C, seed=seed, max_blocks=3)
    rng = np.random.default_rng(seed + 1000)
    cnt = np.array(_BINS)[np.arange(E) % len(_BINS)]
    w["ov_ptr"] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    w["ov_idx"] = rng.integers(0, n_bins, int(w["ov_ptr"][-1])).astype(np.int32)
    w["strand_minus"][0], w["strand_minus"][E - 1] = 1, 0
    if not repeat:
        w["L"].reshape(E, 192)[17 % E, 5] += 1
    return w


def _on_device(w, dev):
    import torch
    return {k: torch.as_tensor(v, device=dev) for k, v in w.items() if isinstance(v, np.ndarray)}


@pytest.fixture(scope="module")
def problems(dev):
    """(host arrays, device tensors) per (cohort count, L repeats), built once and left unchanged."""
    return {(C, rep): (lambda w: (w, _on_device(w, dev)))(_host_workload(E0, C, 7 * C + 1, repeat=rep)) for C in CS for rep in (True, False)}


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


def _up(v):
    return (v + 255) // 256 * 256


def _sections(raw, E, C):
    """dig_element_p_prepare's table (a uint8 array) -> dict of its four sections."""
    o_pi = _up(8 * E * C)
    o_rs = o_pi + _up(8 * E)
    o_es = o_rs + _up(4 * E)
    assert raw.size == o_es + _up(4 * E)
    cut = lambda off, n, t: raw[off: off + n * np.dtype(t).itemsize].copy().view(t)
    return dict(P=cut(0, E * C, np.float64), P_INDEL=cut(o_pi, E, np.float64), R_SIZE=cut(o_rs, E, np.int32), ELT_SIZE=cut(o_es, E, np.int32))


# ---- 1. same bits, planned against live; the table ------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CS)
def test_planned_p_gives_the_bits_of_the_live_form(dev, problems, C):
    import torch
    from digdriver_amd import _lib
    for rep in (True, False):
        w, td = problems[(C, rep)]
        assert sorted(set(np.diff(w["ov_ptr"]))) == list(_BINS) and ((E0 * C) % 64 == 0) == (C == 64)
        assert set(w["strand_minus"].tolist()) == {0, 1}
        for rec in (False, True):
            live = _plan(td, element_p=False, records_out=rec)
            planned = _plan(td, element_p=True, records_out=rec)
            assert live.compact == planned.compact == rep
            assert live.elt_p is None and not live._flags & _lib.DIG_PIPE_ELEMENT_P
            assert planned.elt_p is not None and planned._flags & _lib.DIG_PIPE_ELEMENT_P
            assert planned.elt_p.numel() == int(_lib.load().dig_element_p_bytes(E0, C)) and planned.elt_p.data_ptr() % 256 == 0
            want = _outputs(live, _whole(td))
            _same_bits(_outputs(planned, _whole(td)), want, (C, rep, rec))
            # an element without bins: zero denominators, P is NaN or inf -- and the table carries exactly that
            empty = np.flatnonzero(np.diff(w["ov_ptr"]) == 0)
            assert len(empty) and not torch.isfinite(want["P"][empty]).any()
            assert torch.isfinite(want["P"][np.flatnonzero(np.diff(w["ov_ptr"]) == 12)]).all()
            # the table itself: bit copies of the live call's four outputs
            got = _sections(planned.elt_p.cpu().numpy(), E0, C)
            for k in _KEPT:
                assert GA.same_bits(got[k], want[k].cpu().numpy().ravel()), (C, rep, rec, k)


def test_default_is_planned_and_one_shot_callers_stay_live(dev, problems):
    import inspect
    from digdriver_amd import _lib, engine, parallel
    from digdriver_amd.driver_model import cohort_batch
    w, td = problems[(5, True)]
    assert _plan(td)._flags & _lib.DIG_PIPE_ELEMENT_P
    assert "element_p=False" in inspect.getsource(engine.element_pipeline)
    assert "element_p=False" in inspect.getsource(cohort_batch._element_planes)
    assert "element_p=" not in inspect.getsource(parallel.ShardedPipeline)          # (the default)
    # without packed records and without the context table the option stands on its own
    bare = _plan(td, pack_bins=False, element_contexts=False)
    assert bare.elt_p is not None and bare.elt_ctx is None and bare.records is None
    _same_bits(_outputs(bare, _whole(td)), _outputs(_plan(td, pack_bins=False, element_contexts=False, element_p=False), _whole(td)), "bare")


def test_p_of_eight_byte_alignment_takes_the_narrow_copies(dev, problems):
    """A caller's P is only promised 8-byte alignment: at an odd multiple of 8 both copy kernels fall back to 8-byte pieces."""
    import torch
    from digdriver_amd import engine
    for C in (5, 64):
        w, td = problems[(C, True)]
        slab = torch.full((E0 * C + 2,), -3.0, dtype=torch.float64, device=dev)
        acc = engine.alloc_accumulate_outputs(E0, C, 1, dev)
        acc["P"] = slab[1: 1 + E0 * C].view(E0, 1, C)
        assert acc["P"].data_ptr() % 16 == 8
        odd = _plan(td, out_acc=acc)
        assert odd.elt_p is not None
        _same_bits(_outputs(odd, _whole(td)), _outputs(_plan(td, element_p=False), _whole(td)), ("odd P", C))
        assert slab[0].item() == -3.0 and slab[-1].item() == -3.0


# ---- 2. stages as separate calls, the stage timer ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rep", [True, False], ids=["compact", "general"])
def test_stages_as_separate_calls(dev, problems, rep):
    import torch
    from digdriver_amd import _lib
    w, td = problems[(37, rep)]
    planned, live = _plan(td), _plan(td, element_p=False)
    want = _outputs(planned, _whole(td))

    def staged(plan):
        plan.run(td["cj"], td["cj_indel"], stages=1)
        torch.cuda.synchronize()
        assert all((plan.acc[k] == -3).all() for k in _KEPT)          # the CONTEXTS stage enqueues nothing
        plan.run(td["cj"], td["cj_indel"], stages=2)
        torch.cuda.synchronize()
        for k in _KEPT:                                               # the DOT stage alone restores the four
            x, y = plan.acc[k], want[k]
            assert torch.equal(x.view(torch.int64) if x.dtype.is_floating_point else x, y.view(torch.int64) if y.dtype.is_floating_point else y), k
        assert (plan.stats == -3).all()
        plan.run(td["cj"], td["cj_indel"], stages=4 | 8)
    _same_bits(_outputs(planned, staged), want, "stages 1, 2, 4|8")
    # new scale factors on the same accumulation: a statistics-only call (it clears the worklist header itself)
    cj2, cji2 = td["cj"] * 1.7, td["cj_indel"] * 0.6

    def again(plan):
        plan.run(td["cj"], td["cj_indel"])
        return plan.run(cj2, cji2, stages=_lib.DIG_PIPE_STATISTICS)
    got, ref = _outputs(planned, again), _outputs(live, again)
    _same_bits(got, ref, "statistics-only call")
    assert not torch.equal(ref["plane0"], want["plane0"])


def test_dot_stage_timer_reads_the_stream_kernel(dev, problems):
    import torch
    from digdriver_amd import _lib, engine
    w, td = problems[(37, True)]
    planned = _plan(td)
    want = _outputs(planned, _whole(td))
    timer = engine.StageTimer()

    def timed(plan):
        timer.arm(_lib.DIG_PIPE_DOT)
        plan.run(td["cj"], td["cj_indel"])
    got = _outputs(planned, timed)
    ms = timer.read_ms()
    timer.close()
    print("DOT stage timer on a planned plan: %.4f ms" % ms)
    assert 0.0 < ms < 50.0
    _same_bits(got, want, "timed run")


# ---- 3. the snapshot ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rep", [True, False], ids=["compact", "general"])
def test_snapshot_until_recontext(dev, rep):
    import torch
    w = _host_workload(E0, 37, 21, repeat=rep)
    td = _on_device(w, dev)
    planned = _plan(td)
    assert planned.compact == rep
    shared = _plan(td, pack_bins=planned, element_contexts=planned if rep else True, element_rates=planned, element_p=planned)
    assert shared.elt_p is planned.elt_p
    before = _outputs(planned, _whole(td))
    _same_bits(_outputs(shared, _whole(td)), before, "shared table")
    # d_pr changes in place (one cohort's row scaled): the snapshot is what is read until recontext()
    td["d_pr"][3].mul_(1.5)
    torch.cuda.synchronize()
    _same_bits(_outputs(planned, _whole(td)), before, "d_pr: the snapshot is what is read")
    fresh = _outputs(_plan(td), _whole(td))
    assert not torch.equal(fresh["P"], before["P"])
    _same_bits(fresh, _outputs(_plan(td, element_p=False), _whole(td)), "fresh plans, new d_pr")
    planned.recontext()
    _same_bits(_outputs(planned, _whole(td)), fresh, "after recontext(), new d_pr")
    # L changes in place, every context's three counts together (what repeats keeps repeating)
    L3 = td["L"].view(E0, 64, 3)
    L3[::2, 1::3, :] += 2
    torch.cuda.synchronize()
    _same_bits(_outputs(planned, _whole(td)), fresh, "L: the snapshot is what is read")
    fresh2 = _outputs(_plan(td), _whole(td))
    assert not torch.equal(fresh2["P"], fresh["P"]) and not torch.equal(fresh2["ELT_SIZE"], fresh["ELT_SIZE"])
    _same_bits(fresh2, _outputs(_plan(td, element_p=False), _whole(td)), "fresh plans, new L")
    planned.recontext()
    _same_bits(_outputs(planned, _whole(td)), fresh2, "after recontext(), new L")


# ---- 4. side stream, guard bands, grid cap --------------------------------------------------------------------------------------------------
def _restore_lc(plan):
    from digdriver_amd import _lib
    ok = ctypes.c_int(0)
    _lib.call("dig_element_pipeline_prepare", _lib.dev_ptr(plan.keep[7]), plan.E, plan.C, plan._ws, plan.wsb, ctypes.byref(ok), _lib.stream_ptr())
    assert ok.value == 1


def test_plan_on_a_side_stream_while_the_default_stream_is_busy(dev, problems):
    w, td = problems[(37, True)]
    planned = _plan(td)
    assert planned.compact and planned.elt_p is not None
    GA.side_stream_call(lambda stream: planned.run(td["cj"], td["cj_indel"], stream=stream), dev, "planned-P PipelinePlan.run",
                        explicit=True, scratch=[planned.ws], restore=lambda: _restore_lc(planned))


@pytest.mark.parametrize("C", [5, 64])
def test_guarded_calls(dev, C):
    """dig_element_p_prepare and the pipeline with DIG_PIPE_ELEMENT_P, every pointer carved from a guarded arena at its documented
    alignment: the table at exactly dig_element_p_bytes, P at its 8 bytes, the workspace at exactly its size.  The plan-time
    accumulation writes outputs of its own (P0 ...), so what the flagged call leaves in P ... came through the table."""
    from digdriver_amd import _lib
    E = 33
    w = _host_workload(E, C, 60 + C)
    N, nnz = w["bin_mu"].shape[0], len(w["ov_idx"])
    lib = _lib.load()
    need, ntab = int(lib.dig_element_pipeline_workspace(E, C)), int(lib.dig_element_p_bytes(E, C))
    assert ntab == _up(8 * E * C) + _up(8 * E) + 2 * _up(4 * E)
    arr = lambda dtype, data, **kw: GA.inp(dtype, np.ascontiguousarray(data, GA._NP[dtype]), **kw)
    b = dict(bin_mu=arr("f64", w["bin_mu"]), bin_std=arr("f64", w["bin_std"]), bin_y=arr("i32", w["bin_y"], poison=(0, 9)),
             bin_flag=arr("u8", w["bin_flag"]), bin_ctx=arr("i32", w["bin_ctx"], poison=(0, 9)),
             ov_ptr=arr("i64", w["ov_ptr"], index=(0, nnz)), ov_idx=arr("i32", w["ov_idx"], index=(0, N - 1)),
             L=arr("i32", w["L"], poison=(0, 3)), strand_minus=arr("u8", w["strand_minus"]), d_pr=arr("f64", w["d_pr"]),
             obs_snv=arr("i32", w["obs_snv"], poison=(0, 50)), obs_samples=arr("i32", w["obs_samples"], poison=(0, 50)),
             obs_indel=arr("i32", w["obs_indel"], poison=(0, 50)), cj=arr("f64", w["cj"]), cj_indel=arr("f64", w["cj_indel"]),
             table=GA.ws(ntab, align=256),                 # (a workspace: the padding behind each section is never written)
             P0=GA.out("f64", (E, 1, C)), R_SIZE0=GA.out("i32", E), ELT_SIZE0=GA.out("i32", E), P_INDEL0=GA.out("f64", E),
             MU=GA.out("f64", (E, C)), SIGMA=GA.out("f64", (E, C)), R_OBS=GA.out("i32", (E, C)), FLAG=GA.out("i32", (E, C)),
             P=GA.out("f64", (E, 1, C)), R_SIZE=GA.out("i32", E), ELT_SIZE=GA.out("i32", E), P_INDEL=GA.out("f64", E),
             out=GA.out("f64", (7, E, C)), ws=GA.ws(need, align=256))

    def pipeline(a, d_pr, outs, stages):
        p = a.ptr
        _lib.call("dig_element_pipeline", p("bin_mu"), p("bin_std"), p("bin_y"), p("bin_flag"), p("bin_ctx"), p("ov_ptr"), p("ov_idx"),
                  p("L"), p("strand_minus"), None, p(d_pr), p("obs_snv"), p("obs_samples"), p("obs_indel"), p("cj"), p("cj_indel"),
                  p("MU"), p("SIGMA"), p("R_OBS"), p("FLAG"), *[p(k) for k in outs], p("out"), N, E, C, None,
                  stages | _lib.DIG_PIPE_COMPACT_L, p("ws"), need, _lib.stream_ptr())

    def invoke(a, planned=True):
        p, s = a.ptr, _lib.stream_ptr()
        ok = ctypes.c_int(0)
        _lib.call("dig_element_pipeline_prepare", p("L"), E, C, p("ws"), need, ctypes.byref(ok), s)
        assert ok.value == 1
        pipeline(a, "d_pr", ("P0", "R_SIZE0", "ELT_SIZE0", "P_INDEL0"), 3)
        _lib.call("dig_element_p_prepare", p("P0"), p("R_SIZE0"), p("ELT_SIZE0"), p("P_INDEL0"), E, C, p("table"), ntab, s)
        if planned:
            pipeline(a, "table", ("P", "R_SIZE", "ELT_SIZE", "P_INDEL"), 7 | _lib.DIG_PIPE_ELEMENT_P)
        else:
            pipeline(a, "d_pr", ("P", "R_SIZE", "ELT_SIZE", "P_INDEL"), 7)

    got = GA.guarded_runs(b, invoke, device=dev, what="dig_element_pipeline with planned P C=%d" % C, plain=True)
    live = GA.PlainBuffers(b, dev)
    invoke(live, planned=False)
    live.assert_intact()
    for name in got:
        assert GA.same_bits(got[name], live.read(name)), name
    for k in _KEPT:
        assert GA.same_bits(got[k + "0"], got[k]), k


def test_copies_past_their_grid_cap(dev):
    """256 threads a workgroup, at most 8 workgroups per CU on 256 CUs, four pieces a thread: 2 097 152 pieces in one step of
    the grid.  65 000 elements x 65 cohorts are 4 225 000 doubles: 2 112 500 16-byte pieces, or twice as many 8-byte ones, so
    both widths of both kernels take a second step; E * C is even here, so the odd tail is pinned with E - 1 elements.  The
    inputs are arbitrary bits (the kernels copy): the accumulation stages do not run."""
    import torch
    from digdriver_amd import _lib
    lib = _lib.load()
    C = 65
    g = torch.Generator(device=dev).manual_seed(5)
    for E, shift in ((65000, 0), (65000, 1), (64999, 0)):
        n = E * C
        assert n // 2 > 256 * 8 * 256 * 4 and (n % 2 == 1) == (E == 64999)
        ntab, need = int(lib.dig_element_p_bytes(E, C)), int(lib.dig_element_pipeline_workspace(E, C))
        src = torch.randn(n + 2, dtype=torch.float64, device=dev, generator=g)
        src[::1001] = float("nan")
        src[5::1003] = float("inf")
        P_in = src[shift: shift + n]
        assert P_in.data_ptr() % 16 == 8 * shift
        PI_in = torch.randn(E, dtype=torch.float64, device=dev, generator=g)
        RS_in = torch.randint(0, 1 << 30, (E,), dtype=torch.int32, device=dev, generator=g)
        ES_in = torch.randint(0, 1 << 30, (E,), dtype=torch.int32, device=dev, generator=g)
        table = torch.full((ntab,), 0x5a, dtype=torch.uint8, device=dev)
        p = _lib.dev_ptr
        _lib.call("dig_element_p_prepare", p(P_in), p(RS_in), p(ES_in), p(PI_in), E, C, p(table), ntab, _lib.stream_ptr())
        dst = torch.full((n + 2,), -3.0, dtype=torch.float64, device=dev)
        P_out = dst[shift: shift + n]
        PI_out = torch.full((E,), -3.0, dtype=torch.float64, device=dev)
        RS_out, ES_out = torch.full((E,), -3, dtype=torch.int32, device=dev), torch.full((E,), -3, dtype=torch.int32, device=dev)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        any_ptr = p(PI_in)                                            # arguments of stages that do not run: checked for NULL only
        args = [None] * 10 + [p(table)] + [any_ptr] * 5 + [None] * 4 + [p(P_out), p(RS_out), p(ES_out), p(PI_out), any_ptr, 0, E, C, None,
                                                                         _lib.DIG_PIPE_DOT | _lib.DIG_PIPE_ELEMENT_P, p(ws), need, _lib.stream_ptr()]
        _lib.call("dig_element_pipeline", *args)
        torch.cuda.synchronize()
        sec = _sections(table.cpu().numpy(), E, C)
        as_bits = lambda t: t.cpu().numpy().ravel()
        for k, a_in, a_out in (("P", P_in, P_out), ("P_INDEL", PI_in, PI_out), ("R_SIZE", RS_in, RS_out), ("ELT_SIZE", ES_in, ES_out)):
            assert GA.same_bits(sec[k], as_bits(a_in)), (E, shift, k, "table")
            assert GA.same_bits(as_bits(a_out), as_bits(a_in)), (E, shift, k, "outputs")
        edge = torch.cat([dst[:shift], dst[shift + n:]])
        assert (edge == -3.0).all()
