"""dig_pair_bits / dig_pair_fisher on the GPU (include/dig_hip.h, "pairs of the element route"), through engine.pair_bits and
engine.pair_fisher in both forms.  For every case: the device form and the `_host` twin are byte-equal; the bit matrix, N_ROW and
N_BOTH are byte-equal to the numpy statement (tests/pair_fisher_statement.py); the p-values are within 1e-6 of scipy's hypergeom.sf /
hypergeom.cdf where those are at least 1e-250 and under 1.1e-250 below -- and, on the tables of tests/golden/pair_fisher_golden.npz,
of the exact integer values.  Shapes: the smallest that cross each edge (a tile short / exact / one over, a 3 x 3 tile grid, one and
two words, the LDS chunk's 2 048 bits and one more, cohorts without a pair between cohorts with pairs) and one case at each limit."""
import os

import numpy as np
import pytest

import pair_fisher_statement as S
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "pair_fisher_golden.npz")))


def planted(H, n, seed):
    """A bool [H, n] matrix: random rows of mixed density, then -- as far as H reaches -- an empty row, a full one, two identical ones
    and two complementary ones that are each more than half full (a = lo > 0 against a third row is common; the two themselves have
    a = 0 = lo with r + k = n)."""
    rng = np.random.default_rng(seed)
    m = rng.random((H, n)) < rng.choice([0.02, 0.2, 0.5, 0.9], size=(H, 1))
    if H > 0:
        m[0] = False
    if H > 1:
        m[1] = True
    if H > 3:
        m[3] = m[2]
    if H > 5:
        m[5] = ~m[4]
    if H > 7:                                             # two rows of 3/4 of the samples that overlap as little as they can: a = lo > 0
        m[6], m[7] = np.arange(n) < (3 * n) // 4, np.arange(n) >= n - (3 * n) // 4
    return m


def keys_of(mats, rng=None):
    """The stacked (row, sample) keys of the cohorts' matrices; with rng: shuffled, a tenth repeated, and keys with row -1 mixed in."""
    row, sample, r0 = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], 0
    for m in mats:
        r, s = np.nonzero(m)
        row.append(r + r0), sample.append(s)
        r0 += m.shape[0]
    row, sample = np.concatenate(row), np.concatenate(sample)
    if rng is not None and row.size:
        again = rng.integers(0, row.size, row.size // 10 + 1)
        out = rng.integers(0, 64, 17)
        row, sample = np.concatenate([row, row[again], np.full(17, -1)]), np.concatenate([sample, sample[again], out])
        order = rng.permutation(row.size)
        row, sample = row[order], sample[order]
    return row.astype(np.int32), sample.astype(np.int32)


def run_both(mats, n_samples, dev, what, seed=0):
    """engine.pair_bits + engine.pair_fisher on the device and through the twins; the checks every case shares.  Returns the device
    form's results as numpy arrays, and the tables (n, r, k) per pair."""
    import torch
    from scipy.stats import hypergeom

    from digdriver_amd import engine
    rows = [m.shape[0] for m in mats]
    H_total, W = sum(rows), engine.pair_words(max(n_samples, default=0))
    assert W == S.pair_words(max(n_samples, default=0))
    row, sample = keys_of(mats, np.random.default_rng(seed))
    want_bits = np.concatenate([S.bits_from_bool(m, W) for m in mats]) if mats else np.zeros((0, W), np.uint64)
    if row.size < 20000:                                  # (the statement's loop over the keys is slow on the large cases)
        assert np.array_equal(want_bits, S.bits_from_keys(row, sample, H_total, W))
    got = {}
    for form in ("device", "host"):
        on = (lambda x: torch.as_tensor(x, device=dev)) if form == "device" else (lambda x: x)
        bits = engine.pair_bits(on(row), on(sample), H_total, W)
        res = engine.pair_fisher(bits, rows, n_samples)
        assert form == "host" or (bits.is_cuda and res["n_row"].is_cuda and res["pval_cooccur"].is_cuda)
        host = lambda x: x.cpu().numpy() if form == "device" else x
        got[form] = dict(bits=host(bits).view(np.uint64), **{k: host(res[k]) for k in ("n_row", "n_both", "pval_cooccur", "pval_exclusive")})
        assert np.array_equal(res["pair_ptr"], np.concatenate([[0], np.cumsum([h * (h - 1) // 2 for h in rows])]))
    for k, v in got["device"].items():
        assert v.dtype == got["host"][k].dtype and v.tobytes() == got["host"][k].tobytes(), (what, k)
    g = got["device"]
    assert g["bits"].tobytes() == want_bits.tobytes(), what
    n_row, n_both, nrk = S.pair_counts(want_bits, rows, n_samples)
    assert g["n_row"].dtype == np.int32 and g["n_row"].tobytes() == n_row.tobytes(), what
    assert g["n_both"].dtype == np.int32 and g["n_both"].tobytes() == n_both.tobytes(), what
    if len(n_both):
        n, r, k = nrk.T
        S.check_pvalues(g["pval_cooccur"], hypergeom.sf(n_both - 1, n, k, r), what + ", PVAL_COOCCUR against scipy")
        S.check_pvalues(g["pval_exclusive"], hypergeom.cdf(n_both, n, k, r), what + ", PVAL_EXCLUSIVE against scipy")
        degenerate = (r == 0) | (k == 0) | (r == n) | (k == n)
        assert (g["pval_cooccur"][degenerate] == 1.0).all() and (g["pval_exclusive"][degenerate] == 1.0).all(), what
    return g, nrk


@pytest.mark.parametrize("H", [0, 1, 2, 63, 64, 65, 129])
def test_rows_at_the_tile_edges(H, dev):
    """No pair, one pair, a tile short / exact / one over, a 3 x 3 tile grid with diagonal and off-diagonal tiles; n = 100 observed
    samples in a universe of 131 (n_samples above the observed count)."""
    g, nrk = run_both([planted(H, 100, H)], [131], dev, "H = %d" % H, seed=H)
    assert len(g["n_both"]) == H * (H - 1) // 2


@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129, 2048, 2049])
def test_samples_at_the_word_and_chunk_edges(n, dev):
    """One word, two, three (W rounds up to an even count), and the LDS chunk's 2 048 bits and one more; 66 rows: two tiles a side."""
    from digdriver_amd import engine
    assert engine.PAIR_CHUNK_BITS == 2048
    run_both([planted(66, n, n)], [n], dev, "n = %d" % n, seed=n)


@pytest.mark.parametrize("rows", [(5,), (65, 0, 1, 130), (3, 0, 9)], ids=str)
def test_cohorts_of_different_sizes_in_one_call(rows, dev):
    """C = 1, 3 and 4 with different H and n per cohort, an H = 0 and an H = 1 cohort between two that have pairs."""
    ns = [70, 129, 40, 200][:len(rows)]
    mats = [planted(h, n - 3, 7 * h + n) for h, n in zip(rows, ns)]
    g, nrk = run_both(mats, ns, dev, "rows %r" % (rows,))
    assert len(g["n_both"]) == sum(h * (h - 1) // 2 for h in rows)


def test_every_table_of_the_golden_file(dev, golden):
    """Each table as a cohort of two rows (row A the first r samples, row B a of them and k - a outside), one call per class of n so
    that the small tables share a call with different n_samples: N_BOTH is the table's a, the p-values meet the bound against the
    exact integer values.  Prints the worst relative error."""
    g = golden
    worst = 0.0
    for sel in (g["n"] <= 12,) + tuple(g["n"] == n for n in (64, 100, 2800, 16384, 65536)):
        at = np.nonzero(sel)[0]
        mats = [S.rows_of_table(*(int(g[c][i]) for c in "nrka")) for i in at]
        got, nrk = run_both(mats, [int(x) for x in g["n"][at]], dev, "golden tables with n = %d .. %d" % (g["n"][at].min(), g["n"][at].max()))
        assert np.array_equal(got["n_both"], g["a"][at]) and np.array_equal(nrk, np.stack([g["n"][at], g["r"][at], g["k"][at]], 1))
        worst = max(worst, S.check_pvalues(got["pval_cooccur"], g["pval_cooccur"][at], "PVAL_COOCCUR against the exact values"),
                    S.check_pvalues(got["pval_exclusive"], g["pval_exclusive"][at], "PVAL_EXCLUSIVE against the exact values"))
    print("worst relative error of the kernel over the golden file: %.3g" % worst)
    st = np.array([S.tails(*(int(g[c][i]) for c in "nrka")) for i in range(len(g["n"]))])
    st_worst = max(S.check_pvalues(st[:, 0], g["pval_cooccur"], "statement"), S.check_pvalues(st[:, 1], g["pval_exclusive"], "statement"))
    assert worst <= 10 * max(st_worst, 1e-12), "the kernel and the statement run the same arithmetic: %g against %g" % (worst, st_worst)


def test_the_limit_of_samples(dev):
    """n = 65 536: 1 024 words a row, 32 LDS chunks."""
    g, nrk = run_both([planted(9, 65536, 5)], [65536], dev, "n = 65 536")
    assert g["bits"].shape == (9, 1024)


def test_the_limit_of_rows(dev):
    """H = 8 192 rows of n = 64 samples: 33 550 336 pairs in 8 256 tiles.  Device form and twin byte-equal; N_BOTH by its sum (every
    sample held by c rows is in C(c, 2) intersections) and, with the p-values, on 4 000 pairs against the statement and scipy."""
    import torch
    from scipy.stats import hypergeom

    from digdriver_amd import engine
    H, n = 8192, 64
    m = planted(H, n, 11)
    row, sample = keys_of([m])
    bits = S.bits_from_bool(m, 2)
    d_bits = engine.pair_bits(torch.as_tensor(row, device=dev), torch.as_tensor(sample, device=dev), H, 2)
    assert d_bits.cpu().numpy().view(np.uint64).tobytes() == bits.tobytes()
    d = engine.pair_fisher(d_bits, [H], [n])
    h = engine.pair_fisher(bits, [H], [n])
    for k in ("n_row", "n_both", "pval_cooccur", "pval_exclusive"):
        assert torch.equal(d[k].cpu().view(torch.int32), torch.from_numpy(h[k]).view(torch.int32)), k
    n_row = m.sum(1)
    assert np.array_equal(h["n_row"], n_row) and len(h["n_both"]) == H * (H - 1) // 2 == 33550336
    c = m.sum(0).astype(np.int64)
    assert int(h["n_both"].sum(dtype=np.int64)) == int((c * (c - 1) // 2).sum())
    rng = np.random.default_rng(3)
    i, j = rng.integers(0, H, 4000), rng.integers(0, H, 4000)
    i, j = np.minimum(i, j)[i != j], np.maximum(i, j)[i != j]
    i, j = np.concatenate([i, [0, H - 2, 63, 64]]), np.concatenate([j, [H - 1, H - 1, 64, 8191]])
    at = engine.pair_index(i, j, H)
    a = (m[i] & m[j]).sum(1)
    assert np.array_equal(h["n_both"][at], a)
    S.check_pvalues(h["pval_cooccur"][at], hypergeom.sf(a - 1, n, n_row[j], n_row[i]), "H = 8 192, PVAL_COOCCUR against scipy")
    S.check_pvalues(h["pval_exclusive"][at], hypergeom.cdf(a, n, n_row[j], n_row[i]), "H = 8 192, PVAL_EXCLUSIVE against scipy")
    assert not np.isnan(h["pval_cooccur"]).any() and h["pval_cooccur"].min() > 0 and h["pval_cooccur"].max() <= 1.0


def test_the_public_form_for_one_cohort(dev):
    """nb_model.pair_fisher_exact on a bool array, a frame and a device tensor: the same bits, scipy's fisher_exact on a few pairs."""
    import pandas as pd
    import torch
    from scipy.stats import fisher_exact

    from digdriver_amd.sequence_model import nb_model
    m = planted(12, 90, 2)
    a = nb_model.pair_fisher_exact(m, n_samples=95)
    b = nb_model.pair_fisher_exact(pd.DataFrame(m), n_samples=95)
    c = nb_model.pair_fisher_exact(torch.as_tensor(m, device=dev), n_samples=95)
    for k in ("n_row", "n_both", "pval_cooccur", "pval_exclusive"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes() == getattr(c, k).cpu().numpy().tobytes()
    for i, j in ((2, 3), (4, 5), (6, 7), (8, 11), (11, 9)):
        both = int((m[i] & m[j]).sum())
        table = [[both, int(m[i].sum()) - both], [int(m[j].sum()) - both, 95 - int((m[i] | m[j]).sum())]]
        at = a.pair_index(i, j)
        assert a.n_both[at] == both
        assert abs(a.pval_cooccur[at] - fisher_exact(table, alternative="greater")[1]) <= 1e-6 * a.pval_cooccur[at]
        assert abs(a.pval_exclusive[at] - fisher_exact(table, alternative="less")[1]) <= 1e-6 * a.pval_exclusive[at]
