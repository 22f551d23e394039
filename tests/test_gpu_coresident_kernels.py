"""The kernels of one step that share a CU: the scale factors' background kernels (suffstats_chunk_stage1 / _stage2,
scale_factors_chunked_kernel: at most 32 vector registers each) and the compact contexts + dot kernel (acc_dot_ctx_kernel: at most
160, so that three of its waves and one background wave fill a SIMD's 512).  Neither budget may cost a bit of the results:

  * chunk sums and scale factors against a host twin of the kernels' summation order, bit for bit.  (The library has no `_host`
    entry point for the CHUNKED form; the twin below follows the order dig_suffstats.hip documents: a thread adds its rows first to
    last, a workgroup its row groups first to last, a chunk its workgroups first to last, the factors the chunks first to last.);
  * the compact pipeline against tests/golden/coresident_parent_outputs.npz, recorded on the GPU from the commit BEFORE the dot
    kernel's registers were cut (tools/record_coresident_fixture.py; the file names the commit), byte for byte;
  * both at once on two streams against a sequential evaluation, byte for byte, twenty times."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SS_BLOCK = 256                    # dig_suffstats.hip: kSsBlock
SS_PASSES = 16                    # ss_chunk_rows_per_block(C) = 16 * (kSsBlock / C)
SS_UNROLL = 8                     # kSsUnroll: row loads in flight per thread


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _chunk_sums_twin(mu, flag, chunk_rows):
    """What dig_scale_suffstats_chunked computes, in its order, with numpy's IEEE additions (no contraction: sums only)."""
    C = mu.shape[1]
    rpp = SS_BLOCK // C
    rpb = SS_PASSES * rpp
    x = np.where(flag != 0, 0.0, mu)
    out = np.zeros((len(chunk_rows) - 1, C))
    for j in range(len(chunk_rows) - 1):
        s_chunk = np.zeros(C)
        for r0 in range(int(chunk_rows[j]), int(chunk_rows[j + 1]), rpb):
            r1 = min(r0 + rpb, int(chunk_rows[j + 1]))
            blk = np.zeros((SS_PASSES * rpp, C))                  # (rows a thread does not have: + 0.0 leaves its sum's bits alone)
            blk[: r1 - r0] = x[r0:r1]
            blk = blk.reshape(SS_PASSES, rpp, C)
            acc = np.zeros((rpp, C))
            for k in range(SS_PASSES):                            # thread (row group g, column c): rows g, g + rpp, ... first to last
                acc = acc + blk[k]
            s = np.zeros(C)
            for g in range(rpp):                                  # the workgroup: row groups first to last
                s = s + acc[g]
            s_chunk = s_chunk + s                                 # the chunk: workgroups first to last
        out[j] = s_chunk
    return out


def _chunk_layouts(C):
    rpp = SS_BLOCK // C
    rpb = SS_PASSES * rpp
    return {
        "empty, one row, ragged last block": (0, 1, 2 * rpb + 5),
        "rows off the unroll": (rpb + SS_UNROLL * rpp + 3, (SS_UNROLL - 1) * rpp + 1, (SS_UNROLL + 1) * rpp + rpp // 2 + 1),
    }


@pytest.mark.parametrize("premask", [False, True], ids=["bin_flag given", "bin_flag NULL"])
@pytest.mark.parametrize("C", [1, 37, 48, 104, 256])
def test_chunk_sums_and_scale_factors_match_the_host_twin_bit_for_bit(C, premask):
    import torch
    from digdriver_amd import engine
    dev = torch.device("cuda:0")
    for name, sizes in _chunk_layouts(C).items():
        rows = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        n = int(rows[-1])
        rng = np.random.default_rng([C, n])
        mu = rng.gamma(9.0, 3.0, (n, C)) * 10.0 ** rng.integers(-3, 4, (n, C))       # (magnitudes apart: the order of additions shows)
        mu[rng.uniform(size=(n, C)) < 0.05] *= -1.0
        flag = (rng.uniform(size=(n, C)) < 0.1).astype(np.uint8)
        obs = np.rint(rng.uniform(1e3, 1e6, (2, C)))
        plan = engine.ChunkedScaleFactorPlan(torch.as_tensor(mu, device=dev), torch.as_tensor(flag, device=dev), obs[0], obs[1], rows,
                                             len(sizes), world=1, premask=premask)
        assert (plan.masked is not None) == premask
        cj, cji, tot = (torch.empty(C, dtype=torch.float64, device=dev) for _ in range(3))
        plan.run(cj, cji, out_sum=tot)
        torch.cuda.synchronize()
        want = _chunk_sums_twin(mu, flag, rows)
        got = plan.part[: len(sizes)].cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), (name, C, premask)
        e = np.zeros(C)
        for j in range(len(sizes)):
            e = e + want[j]
        assert np.array_equal(_bits(tot.cpu().numpy()), _bits(e)), (name, C)
        with np.errstate(all="ignore"):
            assert np.array_equal(_bits(cj.cpu().numpy()), _bits((0.0 + obs[0]) / e)), (name, C)
            assert np.array_equal(_bits(cji.cpu().numpy()), _bits((0.0 + obs[1]) / e)), (name, C)


# ---- the compact pipeline against the outputs of the parent commit ---------------------------------------------------------
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coresident_parent_outputs.npz")
_IN = ("bin_mu", "bin_std", "bin_y", "bin_flag", "bin_ctx", "ov_ptr", "ov_idx", "L", "strand_minus", "d_pr", "obs_snv", "obs_samples", "obs_indel")


@pytest.fixture(scope="module")
def parent_outputs():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def _plan(td, **kw):
    from digdriver_amd import engine
    return engine.PipelinePlan(*(td[k] for k in _IN), **kw)


@pytest.mark.parametrize("C", [5, 37, 48])
def test_compact_pipeline_keeps_the_bytes_of_the_parent_commit(parent_outputs, C):
    import torch
    dev = torch.device("cuda:0")
    z = parent_outputs
    assert C in z["cases"] and str(z["recorded_from"]) != "unknown"
    td = {k: torch.as_tensor(z["C%d_in_%s" % (C, k)], device=dev) for k in _IN + ("cj", "cj_indel")}
    E = td["L"].shape[0]
    nov = np.diff(z["C%d_in_ov_ptr" % C])
    assert E == 50 and td["bin_mu"].shape[0] == 64 and nov.min() == 0 and nov.max() == 12 and 0 < int(td["strand_minus"].sum()) < E
    plan = _plan(td, records_out=True)
    assert plan.compact
    plan.out_records.zero_()
    acc, _ = plan.run(td["cj"], td["cj_indel"])
    torch.cuda.synchronize()
    rec = plan.out_records.cpu().numpy().copy()
    rec[-1, :, E * C - 64 * (rec.shape[0] - 1):, :] = 0.0          # (lanes behind the last pair belong to nobody)
    got = {"P": acc["P"][:, 0, :].cpu().numpy(), "R_SIZE": acc["R_SIZE"].cpu().numpy(), "ELT_SIZE": acc["ELT_SIZE"].cpu().numpy(),
           "P_INDEL": acc["P_INDEL"].cpu().numpy(), "records": rec}
    want_p = z["C%d_out_P" % C]
    assert np.isnan(want_p).any(), "the cases hold zero denominators"
    for k, g in got.items():
        w = z["C%d_out_%s" % (C, k)]
        assert g.dtype == w.dtype and g.shape == w.shape, k
        assert g.tobytes() == w.tobytes(), (k, C)


# ---- both kernels at once ---------------------------------------------------------------------------------------------------
def test_scale_factors_beside_the_pipeline_change_no_byte():
    """The scale-factor call on a side stream and the compact pipeline on the main stream, enqueued without any dependency so
    that their kernels share CUs; twenty iterations, each kept, each byte-equal to the same calls on ONE stream."""
    import torch
    from bench import make_workload
    from digdriver_amd import engine, parallel
    dev = torch.device("cuda:0")
    E, C, N, iters = 4096, 37, 8192, 20
    w = make_workload(n_bins=N, n_elements=E, n_cohorts=C, seed=29)
    td = {k: torch.as_tensor(w[k], device=dev) for k in _IN + ("cj", "cj_indel")}
    plan = _plan(td, records_out=True)
    assert plan.compact
    scale = engine.ChunkedScaleFactorPlan(td["bin_mu"], td["bin_flag"], w["n_snv_obs"], w["n_ind_obs"], parallel.canonical_chunks(N),
                                          parallel.N_CHUNKS, world=1)
    f = [torch.empty(C, dtype=torch.float64, device=dev) for _ in range(3)]
    outs = lambda: (f[0], f[1], f[2], scale.part, plan.acc["P"], plan.acc["R_SIZE"], plan.acc["ELT_SIZE"], plan.acc["P_INDEL"], plan.out_records)
    plan.out_records.zero_()
    # sequential: one stream, one call after the other
    scale.run(f[0], f[1], out_sum=f[2])
    plan.run(td["cj"], td["cj_indel"])
    torch.cuda.synchronize()
    want = [t.clone() for t in outs()]
    main, side = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    kept = [[torch.empty_like(t) for t in want] for _ in range(iters)]
    for t in outs():
        (t[: scale.n_own] if t is scale.part else t).zero_()         # (the rows of `part` behind the chunk sums are the plan's observed counts)
    torch.cuda.synchronize()
    for it in range(iters):
        scale.run(f[0], f[1], out_sum=f[2], stream=side)
        plan.run(td["cj"], td["cj_indel"], stream=main)
        with torch.cuda.stream(side):
            for dst, src in zip(kept[it][:4], outs()[:4]):
                dst.copy_(src, non_blocking=True)
        with torch.cuda.stream(main):
            for dst, src in zip(kept[it][4:], outs()[4:]):
                dst.copy_(src, non_blocking=True)
    torch.cuda.synchronize()
    for it in range(iters):
        for j, (g, x) in enumerate(zip(kept[it], want)):
            gb, xb = g.contiguous().view(torch.uint8), x.contiguous().view(torch.uint8)
            assert torch.equal(gb, xb), (it, j)
