"""The meta-cohorts of the element route on the GPU: dig_group_fisher / dig_group_sums (engine.group_fisher, group_sums,
nb_model.fisher_combine_groups; device form and `_host` twins) bit for bit against each other, against the numpy statements of
tests/group_fisher_statement.py where the rule is exact (n_used, the sums, m = 0, 1, 2) and against the 80-digit table of
tests/test_group_fisher_fixture.py inside M_G where it is not (m >= 3); scipy.stats.chi2.sf agrees within the project's 1e-6 where the
reference is at least 1e-250.

Shapes: E in {0, 1, 63, 64, 65, 127, 128, 129, 517} x R in {1, 4} (a chunk is 128 elements: one short, exact, one over, several
workgroups; an odd E with R C >= 2 puts the cohort rows at 0 and at 8 (mod 16) in turn, so both load forms run), each with two of the
30 pairs of C in {1, 2, 3, 37, 64} and M in {1, 2, 8, 9, 32, 33}: M <= 8 and M > 8 are the two compiled forms, 33 is the engine's second
launch.  The group sets hold an empty group, a singleton, a pair, all cohorts, two identical groups and -- every other case -- a cohort
that is in no group.  The planes hold NaNs, an all-NaN cohort, an all-NaN element, zeros, ones, values above 1, 2^-1074 and 1e-300."""
import itertools

import numpy as np
import pytest

import group_fisher_statement as S
from test_group_fisher_fixture import M_G, check_group_fisher, load_fixture

pytestmark = pytest.mark.gpu

ES, RS, CS, MS = (0, 1, 63, 64, 65, 127, 128, 129, 517), (1, 4), (1, 2, 3, 37, 64), (1, 2, 8, 9, 32, 33)
_PAIRS = list(itertools.product(CS, MS))
CASES = [(E, R) + _PAIRS[(2 * i + k) % len(_PAIRS)] + (i + k,) for i, (E, R) in enumerate(itertools.product(ES, RS)) for k in (0, 1)]
assert {c[2:4] for c in CASES} == set(_PAIRS)


@pytest.fixture(scope="module")
def dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    return torch.device("cuda:0")


def hostile_plane(rng, R, C, E):
    p = rng.uniform(size=(R, C, E))
    p[rng.uniform(size=p.shape) < 0.1] = np.nan
    for v in (0.0, 1.0, 1.5, 2.0 ** -1074, 1e-300):
        p[rng.uniform(size=p.shape) < 0.02] = v
    if C > 1:
        p[0, 1, :] = np.nan                                  # a cohort that tested nothing
    if E > 2:
        p[:, :, 2] = np.nan                                  # an element nobody tested
    return p


def group_set(rng, C, M, variant):
    """member u8 [M, C].  variant 0: all cohorts, empty, singleton, pair, the pair again, then random groups, rotated so that a small M
    sees different ones from case to case; odd variants: the last cohort is in no group."""
    last = C - 1 if variant % 2 == 0 or C == 1 else C - 2
    protos = [np.ones(C, bool), np.zeros(C, bool), np.arange(C) == 0, (np.arange(C) == 0) | (np.arange(C) == last)]
    protos.append(protos[3].copy())
    while len(protos) < max(M, 8):
        protos.append(rng.uniform(size=C) < rng.uniform(0.1, 0.9))
    start = variant % 5 if M < 5 else 0
    member = np.stack([protos[(start + i) % len(protos)] for i in range(M)]).astype(np.uint8) * rng.integers(1, 200, size=(M, C)).astype(np.uint8)
    if variant % 2 and C > 1:
        member[:, C - 1] = 0
    return member


def chi2_reference(p, member):
    """scipy's chi2.sf(-2 sum ln p, 2 m) over the testable members, [R, M, E]; NaN where m = 0, and the member's own p where m = 1 (the
    rule returns its bits, a value above 1 included)."""
    from scipy.stats import chi2
    p = p[None] if p.ndim == 2 else p
    with np.errstate(all="ignore"):
        t = np.where(np.isnan(p), 0.0, -np.log(p))
        out = []
        for row in np.asarray(member) != 0:
            s, m = t[:, row].sum(axis=1), (~np.isnan(p[:, row])).sum(axis=1)
            ref = np.where(m > 0, chi2.sf(2.0 * s, 2.0 * np.maximum(m, 1)), np.nan)
            out.append(np.where(m == 1, np.nansum(np.where(row[None, :, None], p, np.nan), axis=1), ref))
    return np.stack(out, axis=1) if out else np.zeros((p.shape[0], 0, p.shape[2]))


def check_against_chi2(got, want):
    assert np.array_equal(np.isnan(got), np.isnan(want))
    big = want >= 1e-250
    with np.errstate(all="ignore"):
        rel = np.abs(got[big] - want[big]) / want[big]
    print("chi2.sf: %d values, %d at or above 1e-250, worst rel %.3g" % (want.size, int(big.sum()), float(rel.max()) if big.any() else 0.0))
    assert (rel <= 1e-6).all()
    assert (got[~big & ~np.isnan(want)] < 1.1e-250).all()


@pytest.mark.parametrize("E,R,C,M,variant", CASES, ids=["E%d-R%d-C%d-M%d" % c[:4] for c in CASES])
def test_device_form_twins_and_statement_agree(E, R, C, M, variant, dev):
    import torch
    from digdriver_amd import engine
    from digdriver_amd.sequence_model import nb_model
    rng = np.random.default_rng(1000 * E + 100 * R + C + M)
    p, member = hostile_plane(rng, R, C, E), group_set(rng, C, M, variant)
    x = np.where(rng.uniform(size=p.shape) < 0.05, np.nan, rng.integers(0, 50, size=p.shape) + rng.uniform(size=p.shape))
    on = lambda a: torch.as_tensor(a, device=dev)
    host = engine.group_fisher(p, member)
    got = engine.group_fisher(on(p), on(member))
    assert got["pval"].is_cuda and got["n_used"].dtype == torch.int32 and tuple(got["pval"].shape) == (R, M, E)
    pval, n = got["pval"].cpu().numpy(), got["n_used"].cpu().numpy()
    assert pval.tobytes() == host["pval"].tobytes() and n.tobytes() == host["n_used"].tobytes()
    assert engine.group_fisher(on(p), on(member), counts=False)["pval"].cpu().numpy().tobytes() == pval.tobytes()
    # exact: the counts, and the groups of up to two testable members
    assert n.tobytes() == S.n_used(p, member).tobytes()
    small, known = S.small_groups(p, member, nb_model.fisher_combine)
    assert pval[known].tobytes() == small[known].tobytes()
    if variant % 2 == 0 and M >= 8 and E > 3 and C > 3:
        assert (n == 0).any() and (n == 1).any() and (n == 2).any() and (n >= 3).any()
        assert pval[:, 3].tobytes() == pval[:, 4].tobytes()                         # two identical groups
    # m >= 3: the special outcomes exactly, the rest against scipy
    with np.errstate(all="ignore"):
        t = np.where(np.isnan(p), 0.0, -np.log(p))
    for g, row in enumerate(member != 0):
        s = np.zeros((R, E))
        for c in np.flatnonzero(row):
            s = s + t[:, c]
        big = n[:, g] >= 3
        assert (pval[:, g][big & np.isinf(s)] == 0.0).all() and (pval[:, g][big & (s < 0)] == 1.0).all()
    check_against_chi2(pval, chi2_reference(p, member))
    # the sums, ungated and gated
    for gate in (None, p):
        want = S.group_sums(x, member, gate)
        a = engine.group_sums(on(x), on(member), gate=None if gate is None else on(gate))
        b = engine.group_sums(x, member, gate=gate)
        assert a.is_cuda and a.cpu().numpy().tobytes() == want.tobytes() and b.tobytes() == want.tobytes()
    if R == 1:                                                                       # a [C, E] plane is R = 1
        flat = engine.group_fisher(on(p[0]), on(member))
        assert tuple(flat["pval"].shape) == (M, E) and flat["pval"].cpu().numpy().tobytes() == pval[0].tobytes()
        assert engine.group_sums(x[0], member).tobytes() == S.group_sums(x, member)[0].tobytes()


@pytest.mark.parametrize("M,at", [(1, 0), (8, 7), (9, 8), (32, 31), (33, 32)], ids=lambda v: str(v))
def test_three_and_more_members_match_the_80_digit_table(M, at, dev):
    """The table's rows as the elements of a [1, 64, N] plane (NaN behind a row's m members), the group of all cohorts at slot `at`
    of M groups: both compiled forms and the engine's second launch, device form and twin."""
    import torch
    from digdriver_amd import engine
    fx = load_fixture()
    p = np.ascontiguousarray(fx["p"].T)[None]                                       # [1, 64, N]
    member = np.zeros((M, 64), np.uint8)
    member[at] = 1
    member[:at, ::3] = 1
    got = engine.group_fisher(torch.as_tensor(p, device=dev), torch.as_tensor(member, device=dev))
    pval, n = got["pval"].cpu().numpy()[0], got["n_used"].cpu().numpy()[0]
    assert np.array_equal(n[at], fx["m"])
    check_group_fisher(pval[at], fx, "dig_group_fisher, slot %d of %d" % (at, M))
    host = engine.group_fisher(p, member)
    assert host["pval"].tobytes() == got["pval"].cpu().numpy().tobytes() and host["n_used"].tobytes() == got["n_used"].cpu().numpy().tobytes()
    assert np.array_equal(pval[at] == 0, fx["want"] == 0)
    check_against_chi2(pval[None, at], chi2_reference(p, member[at:at + 1])[0])


def test_more_than_32_groups_are_the_launches_side_by_side(dev):
    import torch
    from digdriver_amd import engine
    rng = np.random.default_rng(8)
    p, member = hostile_plane(rng, 2, 37, 129), group_set(rng, 37, 70, 0)
    x = rng.uniform(size=p.shape)
    on = lambda a: torch.as_tensor(a, device=dev)
    whole = engine.group_fisher(on(p), on(member))
    sums = engine.group_sums(on(x), on(member), gate=on(p))
    for g0 in (0, 32, 64):
        part = engine.group_fisher(on(p), on(member[g0:g0 + 32]))
        assert torch.equal(whole["n_used"][:, g0:g0 + 32], part["n_used"])
        assert whole["pval"][:, g0:g0 + 32].cpu().numpy().tobytes() == part["pval"].cpu().numpy().tobytes()
        assert sums[:, g0:g0 + 32].cpu().numpy().tobytes() == engine.group_sums(on(x), on(member[g0:g0 + 32]), gate=on(p)).cpu().numpy().tobytes()
    assert sums.cpu().numpy().tobytes() == S.group_sums(x, member, p).tobytes()


def test_fisher_combine_groups_takes_arrays_frames_and_tensors(dev):
    import pandas as pd
    import torch
    from digdriver_amd.sequence_model import nb_model
    rng = np.random.default_rng(9)
    p = rng.uniform(size=(5, 11))
    p[2, 3] = np.nan
    member = np.array([[1, 1, 0, 0, 0], [1, 1, 1, 1, 1], [0, 0, 1, 0, 0]])
    got = nb_model.fisher_combine_groups(p, member)
    assert isinstance(got, np.ndarray) and got.shape == (3, 11)
    assert got[0].tobytes() == np.asarray(nb_model.fisher_combine(p[0], p[1])).tobytes()     # a pair group is fisher_combine
    assert np.array_equal(got[2], p[2], equal_nan=True)
    t = nb_model.fisher_combine_groups(torch.as_tensor(p, device=dev), torch.as_tensor(member, device=dev))
    assert t.is_cuda and t.cpu().numpy().tobytes() == got.tobytes()
    frame = pd.DataFrame(p, index=list("ABCDE"), columns=["e%d" % i for i in range(11)])
    groups = pd.DataFrame(member, index=["ab", "all", "c"], columns=list("ABCDE"))
    f = nb_model.fisher_combine_groups(frame, groups)
    assert isinstance(f, pd.DataFrame) and list(f.index) == ["ab", "all", "c"] and list(f.columns) == list(frame.columns)
    assert f.values.tobytes() == got.tobytes()
    check_against_chi2(got[None], chi2_reference(p, member))
    assert M_G == 32.0
