"""The engine functions that moved onto the backend pair: the tile front half (base_tile_probs, tile_mut_counts) through the `_host`
twins against the device form, bit for bit, and scale_factors_local / scale_factors_from_parts against the plan, whose cached-argument
path is the one the benchmark runs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BINSIZE = 7
# chr1: 200 bases with a run of N at 60 .. 89; chr2: 150 bases
REGIONS = [("chr1", 100, 150),            # ordinary
           ("chr2", 120, 170),            # reaches past the end of chr2
           ("chr1", 0, 40),               # starts at 0
           ("chr1", 65, 85)]              # inside the run of N -- passed out of (chrom, start) order: order[pair_blk] matters
MUTS = [("chr1", 100, 101, 0),            # on the ordinary region's first position (n_up = 1; with n_up = 2 still inside it)
        ("chr1", 149, 150, 1),            # on its last
        ("chr1", 102, 103, 1), ("chr1", 102, 103, 1), ("chr1", 102, 103, 0),      # a position hit twice in one cohort
        ("chr1", 120, 124, 0),            # longer than one base
        ("chr1", 110, 110, 1),            # a zero-length row
        ("chr1", 160, 161, 0),            # outside every region
        ("chr2", 10, 11, 1),              # outside every region, other chromosome
        ("chr2", 130, 131, 0), ("chr2", 148, 149, 1),
        ("chr1", 2, 3, 0), ("chr1", 39, 40, 1),
        ("chr1", 70, 71, 0),              # in the run of N
        ("chr1", 105, 106, -1)]           # a cohort outside [0, C): skipped


@pytest.fixture(scope="module")
def genome():
    from digdriver_amd.data_tools.genome import PackedGenome
    rng = np.random.default_rng(12)
    chr1 = rng.choice(list("ACGT"), 200)
    chr1[60:90] = "N"
    return PackedGenome.from_sequences({"chr1": "".join(chr1), "chr2": "".join(rng.choice(list("ACGT"), 150))})


def _front_half(genome, regions, muts, s_prob, on_device):
    from digdriver_amd import engine
    chroms, starts, ends = [r[0] for r in regions], np.array([r[1] for r in regions], np.int64), np.array([r[2] for r in regions], np.int64)
    pt, first, nval = engine.base_tile_probs(genome, chroms, starts, ends, s_prob, BINSIZE, on_device=on_device)
    mc, ms, me = np.array([m[0] for m in muts], dtype=str), np.array([m[1] for m in muts], np.int64), np.array([m[2] for m in muts], np.int64)
    k = engine.tile_mut_counts(genome, chroms, starts, ends, first, nval, mc, ms, me, np.array([m[3] for m in muts], np.int32),
                               s_prob.shape[0], BINSIZE, pt.shape[2])
    got = dict(pt=pt, first_pos=first, n_valid=nval, k=k)
    assert all(engine.is_cuda(v) == on_device for v in got.values())
    return {name: v.cpu().numpy() if on_device else v for name, v in got.items()}


def _same(host, dev):
    for name in ("pt", "first_pos", "n_valid", "k"):
        assert host[name].dtype == dev[name].dtype and host[name].shape == dev[name].shape, name
        assert np.array_equal(host[name], dev[name], equal_nan=True), name


@pytest.mark.parametrize("n_up", [1, 2])
def test_tile_front_half_host_form_equals_device_form(genome, n_up):
    from digdriver_amd import engine
    C, R = 2, len(REGIONS)
    s_prob = np.random.default_rng(n_up).uniform(1e-3, 1e-2, (C, 4 ** (2 * n_up + 1)))
    host, dev = (_front_half(genome, REGIONS, MUTS, s_prob, on_device) for on_device in (False, True))
    _same(host, dev)
    T = 8                                                                              # the longest region: 50 positions in tiles of 7
    assert dev["pt"].shape == (C, R, T) and dev["k"].shape == (C, R, T) and dev["k"].dtype == np.int32
    assert dev["first_pos"].tolist() == [100, 120, n_up, 65]                           # (a region that starts at 0 begins at n_up)
    assert dev["n_valid"].tolist() == [8, -(-(150 - n_up - 120) // BINSIZE), -(-(40 - n_up) // BINSIZE), 3]
    # the counts sit in their regions' rows, in the order the regions were passed: region 0 holds (cohort 0) rows at 100, 102 and
    # 120 and (cohort 1) rows at 149, twice 102 and the zero-length row's start 110 when the join reports it
    k = dev["k"]
    assert k[0, 0].tolist() == [2, 0, 1, 0, 0, 0, 0, 0] and k[1, 0, 0] == 2 and k[1, 0, 7] == 1 and k[1, 0].sum() in (3, 4)
    assert k[0, 1].sum() == 1 and k[1, 1].sum() == (1 if n_up == 1 else 0)             # 148 is chr2's last position with a trinucleotide
    assert k[0, 2].sum() == 1 and k[1, 2].sum() == 1 and k[0, 3].sum() == 1 and k[1, 3].sum() == 0
    # without a mutation row, and without a region
    _same(*(_front_half(genome, REGIONS, [], s_prob, on_device) for on_device in (False, True)))
    none = [_front_half(genome, [], MUTS, s_prob, on_device) for on_device in (False, True)]
    _same(*none)
    assert none[1]["pt"].shape == (C, 0, 1) and none[1]["k"].shape == (C, 0, 1)
    # tiled_nb_model hands on_device through: arrays out of the host form, the same bits
    chroms, starts, ends = [r[0] for r in REGIONS], [r[1] for r in REGIONS], [r[2] for r in REGIONS]
    mu = np.full((C, R), 3.0)
    rows = [np.array([m[j] for m in MUTS]) for j in range(4)]
    whole = [engine.tiled_nb_model(genome, chroms, starts, ends, s_prob, mu, mu / 2, rows[0].astype(str), rows[1], rows[2],
                                   rows[3].astype(np.int32), binsize=BINSIZE, on_device=on_device) for on_device in (False, True)]
    assert all(isinstance(v, np.ndarray) for v in whole[0].values()) and all(engine.is_cuda(v) for v in whole[1].values())
    for name in ("pt", "first_pos", "n_valid", "k", "pval", "exp"):
        assert np.array_equal(whole[0][name], whole[1][name].cpu().numpy(), equal_nan=True), name
    _same(whole[0], dev)


def _scale_case(dev):
    import torch
    N, C = 5, 3
    rng = np.random.default_rng(5)
    flag = np.zeros((N, C), np.uint8)
    flag[[1, 4, 2], [0, 1, 2]] = 1                                                     # one flagged bin per cohort
    t = lambda a: torch.as_tensor(a, device=dev)
    return t(rng.uniform(0.5, 40.0, (N, C))), t(flag), t(rng.integers(50, 5000, C).astype(np.float64)), t(rng.integers(1, 300, C).astype(np.float64))


def _plan_result(mu, flag, n_snv, n_ind):
    import torch
    from digdriver_amd import engine
    out = [torch.empty(mu.shape[1], dtype=torch.float64, device=mu.device) for _ in range(3)]
    engine.ScaleFactorPlan(mu, flag, n_snv, n_ind).run(*out)
    torch.cuda.synchronize()
    return out                                                                         # exp_sum, cj, cj_indel


def test_scale_factors_through_the_backend_equal_the_plan():
    import torch
    from digdriver_amd import engine
    dev = torch.device("cuda:0")
    mu, flag, n_snv, n_ind = _scale_case(dev)
    exp_sum, cj, cji = _plan_result(mu, flag, n_snv, n_ind)
    got = engine.scale_factors_local(mu, flag, n_snv, n_ind)
    assert [torch.equal(a, b) for a, b in zip(got, (cj, cji, exp_sum))] == [True] * 3
    np.testing.assert_allclose(exp_sum.cpu().numpy(), (mu * (flag == 0)).sum(dim=0).cpu().numpy(), rtol=1e-13)
    into = tuple(torch.full((3,), float("nan"), dtype=torch.float64, device=dev) for _ in range(3))
    assert engine.scale_factors_local(mu, flag, n_snv, n_ind, out=into) is into and torch.equal(into[0], cj) and torch.equal(into[2], exp_sum)
    # the parts of one shard are the plan's own sums and counts: a plain division, the plan's bits
    parts = torch.stack([exp_sum, n_snv, n_ind]).unsqueeze(0).contiguous()
    got = engine.scale_factors_from_parts(parts)
    assert torch.equal(got[0], cj) and torch.equal(got[1], cji)
    # two shards whose sums add exactly (integer-valued rates): rows 0 .. 1 and 2 .. 4, the counts split between them
    whole = torch.floor(mu)
    exp2, cj2, cji2 = _plan_result(whole, flag, n_snv, n_ind)
    shards = []
    for rows, share in ((slice(0, 2), 0.25), (slice(2, 5), 0.75)):
        s = _plan_result(whole[rows].contiguous(), flag[rows].contiguous(), n_snv, n_ind)[0]
        shards.append(torch.stack([s, n_snv * share, n_ind * share]))
    got = engine.scale_factors_from_parts(torch.stack(shards))
    assert torch.equal(got[0], cj2) and torch.equal(got[1], cji2)


def test_scale_factors_land_on_the_current_stream():
    """Inside torch.cuda.stream(side) the launches belong to `side`: its synchronisation alone makes the results readable, while the
    default stream is still busy with work enqueued before them."""
    import torch
    from digdriver_amd import engine
    dev = torch.device("cuda:0")
    mu, flag, n_snv, n_ind = _scale_case(dev)
    exp_sum, cj, cji = _plan_result(mu, flag, n_snv, n_ind)
    parts = torch.stack([exp_sum, n_snv, n_ind]).unsqueeze(0).contiguous()
    nan = lambda: torch.full((3,), float("nan"), dtype=torch.float64, device=dev)
    local, from_parts = (nan(), nan(), nan()), (nan(), nan())
    busy = torch.ones(1 << 26, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    for _ in range(200):                                                               # tens of milliseconds in front of anything else there
        busy.mul_(1.0001)
    with torch.cuda.stream(side):
        engine.scale_factors_local(mu, flag, n_snv, n_ind, out=local)
        engine.scale_factors_from_parts(parts, out=from_parts)
        side.synchronize()
        host = [x.cpu() for x in local + from_parts]                                   # (copied on `side` as well)
    torch.cuda.synchronize()
    for got, want in zip(host, (cj, cji, exp_sum, cj, cji)):
        assert torch.equal(got, want.cpu())
