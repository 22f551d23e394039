"""What the host path of an engine operation does that its device path does not (and the reverse), where no other test says so:
one-cohort tables given as vectors, one scale factor standing for every cohort, an empty overlap list, the output types of
gather_bins and of the element-wise tests of nb_model."""
import numpy as np
import pandas as pd
import pytest
import torch

from bench import make_workload
from digdriver_amd import _lib, engine
from digdriver_amd.sequence_model import nb_model

pytestmark = pytest.mark.gpu

ACC = ("bin_mu", "bin_std", "bin_y", "bin_flag", "bin_ctx", "ov_ptr", "ov_idx", "L", "strand_minus", "d_pr")


@pytest.fixture(scope="module")
def _gpu():
    _lib.require_device()


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f") for k in a) and set(a) == set(b)


def test_host_takes_one_cohort_tables_as_vectors(_gpu):
    w = make_workload(n_bins=300, n_elements=80, n_cohorts=1, seed=5)
    flat = dict(w, **{k: w[k][:, 0] for k in ("bin_mu", "bin_std", "bin_y", "bin_flag")})
    acc, acc1 = engine.accumulate_elements(*[w[k] for k in ACC]), engine.accumulate_elements(*[flat[k] for k in ACC])
    E = w["L"].shape[0]
    assert acc["MU"].shape == (E, 1) and same(acc, acc1)
    assert np.array_equal(engine.scale_suffstats(w["bin_mu"], w["bin_flag"]), engine.scale_suffstats(flat["bin_mu"], flat["bin_flag"]))
    obs = [w[k] for k in ("obs_snv", "obs_samples", "obs_indel")]
    st = engine.element_stats(acc["MU"], acc["SIGMA"], acc["P"][:, 0, :], acc["P_INDEL"], *obs, w["cj"], w["cj_indel"])
    st1 = engine.element_stats(acc["MU"][:, 0], acc["SIGMA"][:, 0], acc["P"][:, 0, 0], acc["P_INDEL"], *[o[:, 0] for o in obs],
                               float(w["cj"][0]), float(w["cj_indel"][0]))
    assert st["EXP_SNV"].shape == (E, 1) and same(st, st1)


def test_host_broadcasts_one_scale_factor_to_every_cohort(_gpu):
    w = make_workload(n_bins=300, n_elements=80, n_cohorts=3, seed=6)
    acc = engine.accumulate_elements(*[w[k] for k in ACC])
    args = [acc["MU"], acc["SIGMA"], acc["P"][:, 0, :], acc["P_INDEL"], w["obs_snv"], w["obs_samples"], w["obs_indel"]]
    assert same(engine.element_stats(*args, np.full(3, 1.25), np.full(3, 0.5)), engine.element_stats(*args, 1.25, [0.5]))
    dev = [torch.as_tensor(np.ascontiguousarray(a), device="cuda:0") for a in args]
    got = engine.element_stats(*dev, torch.full((3,), 1.25, dtype=torch.float64, device="cuda:0"),
                               torch.full((3,), 0.5, dtype=torch.float64, device="cuda:0"))
    assert all(v.is_cuda for v in got.values())
    assert same({k: v.cpu().numpy() for k, v in got.items()}, engine.element_stats(*args, 1.25, 0.5))


def test_host_takes_an_empty_overlap_list(_gpu):
    w = make_workload(n_bins=300, n_elements=40, n_cohorts=2, seed=7)
    E = w["L"].shape[0]
    w = dict(w, ov_ptr=np.zeros(E + 1, np.int64), ov_idx=np.zeros(0, np.int32))
    acc = engine.accumulate_elements(*[w[k] for k in ACC])
    assert acc["R_OBS"].shape == (E, 2) and not acc["R_OBS"].any() and not acc["R_SIZE"].any()


def test_gather_bins_output_types(_gpu):
    x = np.arange(4 * 5 * 3, dtype=np.int16).reshape(4, 5, 3)
    rows = [2, 0]
    host = engine.gather_bins(x, rows)
    assert host.dtype == np.float32 and np.array_equal(host, x[rows].astype(np.float32))
    with pytest.raises(ValueError):
        engine.gather_bins(x, rows, out_dtype="bf16")
    xd = torch.as_tensor(x, device="cuda:0")
    assert np.array_equal(engine.gather_bins(xd, rows).cpu().numpy(), host)
    bf = engine.gather_bins(xd, rows, out_dtype="bf16")
    assert bf.dtype == torch.bfloat16 and np.array_equal(bf.float().cpu().numpy(), host)       # (values below 256: exact in bf16)


def test_nb_model_result_types(_gpu):
    k, alpha, p = np.array([3.0, 0.0, 7.0]), np.array([2.0, 1.5, 4.0]), np.array([0.4, 0.5, 0.6])
    want = nb_model.nb_pvalue_greater_midp(k, alpha, p)
    assert isinstance(want, np.ndarray) and want.shape == (3,)
    one = nb_model.nb_pvalue_greater_midp(3.0, 2.0, 0.4)
    assert type(one) is float and one == want[0]
    ser = nb_model.nb_pvalue_greater_midp(pd.Series(k, index=list("abc")), alpha, p)
    assert isinstance(ser, pd.Series) and list(ser.index) == list("abc") and np.array_equal(ser.values, want)
    dev = nb_model.nb_pvalue_greater_midp(torch.as_tensor(k, device="cuda:0"), alpha, p)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), want)
    a, th = nb_model.normal_params_to_gamma(2.0, 3.0)
    assert type(a) is float and type(th) is float and (a, th) == tuple(float(v[0]) for v in nb_model.normal_params_to_gamma([2.0], [3.0]))
    f = nb_model.fisher_combine(pd.Series([0.1, 0.2]), 0.5)
    assert isinstance(f, pd.Series) and type(nb_model.fisher_combine(0.1, 0.5)) is float and f[0] == nb_model.fisher_combine(0.1, 0.5)
