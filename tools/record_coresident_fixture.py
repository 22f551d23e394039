#!/usr/bin/env python
"""Record tests/golden/coresident_parent_outputs.npz: small seeded inputs of the compact pipeline and what a build of the library
computes from them on the GPU -- `P`, the sizes and the statistics records of engine.PipelinePlan(records_out=True).

    python tools/record_coresident_fixture.py [OUT.npz]         (DIG_HIP_LIB=<a build of the parent commit> to record from it)

tests/test_gpu_coresident_kernels.py compares the current build byte for byte against the file: it pins "results stay what they
were" for acc_dot_ctx_kernel across changes of its register allocation.  The file names the commit it was recorded from in
`recorded_from`; give it as DIG_FIXTURE_COMMIT.  Cases: E = 50 elements over 0 ... 12 bins each (the first and a few more have
none: zero denominators), both strands, N = 64 bins, C = 5, 37, 48; some L counts are zero."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CASES = (5, 37, 48)
E, N = 50, 64
INPUTS = ("bin_mu", "bin_std", "bin_y", "bin_flag", "bin_ctx", "ov_ptr", "ov_idx", "L", "strand_minus", "d_pr", "obs_snv", "obs_samples",
          "obs_indel", "cj", "cj_indel")
OUTPUTS = ("P", "R_SIZE", "ELT_SIZE", "P_INDEL", "records")


def make_inputs(C, seed):
    rng = np.random.default_rng([20261017, seed, C])
    w = {}
    w["bin_mu"] = rng.gamma(9.0, 3.0, (N, C))
    w["bin_std"] = rng.gamma(4.0, 1.0, (N, C))
    w["bin_y"] = rng.poisson(w["bin_mu"]).astype(np.int32)
    w["bin_flag"] = (rng.uniform(size=(N, 1)) < 0.1).repeat(C, axis=1).astype(np.uint8)
    w["bin_ctx"] = rng.multinomial(10_000, rng.dirichlet(np.ones(64)), size=N).astype(np.int32)
    cnt = rng.integers(0, 13, E)
    cnt[[0, 17, 49]] = 0                                   # elements without bins (first, last, one inside a tile)
    cnt[[1, 2, 3]] = (1, 2, 12)
    w["ov_ptr"] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    first = rng.integers(0, N - 12, E)
    w["ov_idx"] = np.concatenate([first[e] + np.arange(cnt[e]) for e in range(E)]).astype(np.int32)
    L64 = rng.poisson(1.5, (E, 64)).astype(np.int32)       # (about a fifth of the counts are zero)
    L64[5] = 0
    w["L"] = np.repeat(L64, 3, axis=1)[:, None, :].astype(np.int32)
    w["strand_minus"] = (np.arange(E) % 3 == 1).astype(np.uint8)
    w["d_pr"] = rng.dirichlet(np.ones(192), size=C) * 1e-6 * 192
    w["obs_snv"] = rng.poisson(3.0, (E, C)).astype(np.int32)
    w["obs_samples"] = rng.binomial(w["obs_snv"], 0.9).astype(np.int32)
    w["obs_indel"] = rng.poisson(0.5, (E, C)).astype(np.int32)
    w["cj"] = rng.uniform(0.2, 3.0, C)
    w["cj_indel"] = rng.uniform(0.02, 0.3, C)
    return w


def run_case(w, dev):
    """The compact pipeline with record outputs -> dict of host arrays (OUTPUTS); the records' unused tail lanes zeroed."""
    import torch
    from digdriver_amd import engine
    td = {k: torch.as_tensor(v, device=dev) for k, v in w.items()}
    plan = engine.PipelinePlan(td["bin_mu"], td["bin_std"], td["bin_y"], td["bin_flag"], td["bin_ctx"], td["ov_ptr"], td["ov_idx"], td["L"],
                               td["strand_minus"], td["d_pr"], td["obs_snv"], td["obs_samples"], td["obs_indel"], records_out=True)
    assert plan.compact, "the inputs repeat every context count three times"
    plan.out_records.zero_()
    acc, _ = plan.run(td["cj"], td["cj_indel"])
    torch.cuda.synchronize()
    rec = plan.out_records.cpu().numpy().copy()
    n_pairs = plan.E * plan.C
    rec[-1, :, n_pairs - 64 * (rec.shape[0] - 1):, :] = 0.0
    out = {"P": acc["P"][:, 0, :].cpu().numpy(), "R_SIZE": acc["R_SIZE"].cpu().numpy(), "ELT_SIZE": acc["ELT_SIZE"].cpu().numpy(),
           "P_INDEL": acc["P_INDEL"].cpu().numpy(), "records": rec}
    return out


def main():
    import torch
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "coresident_parent_outputs.npz")
    dev = torch.device("cuda:0")
    store = {"recorded_from": np.array(os.environ.get("DIG_FIXTURE_COMMIT", "unknown")), "cases": np.array(CASES)}
    for C in CASES:
        w = make_inputs(C, 1)
        got = run_case(w, dev)
        for k in INPUTS:
            store["C%d_in_%s" % (C, k)] = w[k]
        for k in OUTPUTS:
            store["C%d_out_%s" % (C, k)] = got[k]
        print("C = %d: %d NaN and %d inf in P" % (C, int(np.isnan(got["P"]).sum()), int(np.isinf(got["P"]).sum())))
    np.savez_compressed(out_path, **store)
    print("wrote %s (%d bytes)" % (out_path, os.path.getsize(out_path)))


if __name__ == "__main__":
    main()
