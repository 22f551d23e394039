"""dig_pair_bits, dig_pair_fisher, dig_pair_counts and their `_host` twins called through `_lib.call` with pointers carved from a guarded
arena (tests/guarded_arena.py; the twin's arena lies in host memory), on a side stream as well: every argument at exactly the alignment
the header states -- bits at 0 (mod 16) and no more, everything else at its element's --, outputs of exactly H_total W, n_max + 1,
H_total and n_pairs elements, 64 KiB of typed poison around every buffer, twice (poison A / B): no band touched, outputs bit-identical
between A and B, equal to the call on ordinary buffers and to the statement.  And engine.pair_bits + engine.pair_fisher inside a side
stream while the default stream is busy."""
import numpy as np
import pytest

import guarded_arena as GA
import pair_fisher_statement as S
from guarded_arena import guarded_runs, inp, out
from test_gpu_pair_fisher import keys_of, planted

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    return torch.device("cuda:0")


# (rows per cohort, samples per cohort): one pair; a tile and one row over, three words; cohorts without a pair between two with pairs,
# the second LDS chunk begun
CASES = [((2,), (1,)), ((65,), (130,)), ((3, 0, 1, 70), (64, 9, 200, 2049))]


@pytest.mark.parametrize("rows,ns", CASES, ids=str)
def test_entry_points_and_twins_at_their_documented_alignments(rows, ns, dev):
    from scipy.stats import hypergeom

    from digdriver_amd import _lib, engine
    mats = [planted(h, n, 3 * h + n) for h, n in zip(rows, ns)]
    plan = engine.pair_plan(rows, ns)
    H_total, W, P, T = plan["H_total"], plan["W"], plan["n_pairs"], len(plan["tiles"])
    row, sample = keys_of(mats, np.random.default_rng(1))
    want_bits = np.concatenate([S.bits_from_bool(m, W) for m in mats])
    n_row, n_both, nrk = S.pair_counts(want_bits, rows, ns)
    results = []
    for suffix, where in (("", dev), ("_host", "cpu")):
        last = (lambda: _lib.stream_ptr()) if where is dev else (lambda: 0)
        got = guarded_runs(dict(row=inp("i32", row, index=(-1, H_total - 1)), sample=inp("i32", sample, index=(0, max(ns) - 1 or 1)),
                                bits=out("i64", (H_total, W), align=16)),
                           lambda a: _lib.call("dig_pair_bits" + suffix, a.ptr("row"), a.ptr("sample"), len(row), H_total, W, a.ptr("bits"), last()),
                           device=where, what="dig_pair_bits" + suffix, plain=True)
        assert got["bits"].view(np.uint64).tobytes() == want_bits.tobytes()
        head = dict(bits=inp("i64", want_bits.view(np.int64), align=16), row_ptr=inp("i64", plan["row_ptr"]), n_samples=inp("i32", plan["n_samples"]),
                    pair_ptr=inp("i64", plan["pair_ptr"]), tiles=inp("i32", plan["tiles"]))
        args = lambda a: (a.ptr("bits"), H_total, W, a.ptr("row_ptr"), a.ptr("n_samples"), a.ptr("pair_ptr"), plan["C"], a.ptr("tiles"), T, P,
                          plan["n_max"], plan["h_max"])
        full = guarded_runs(dict(head, lnfact=out("f64", plan["n_max"] + 1), n_row=out("i32", H_total), n_both=out("i32", P),
                                 pval_cooccur=out("f64", P), pval_exclusive=out("f64", P)),
                            lambda a: _lib.call("dig_pair_fisher" + suffix, *args(a), a.ptr("lnfact"), a.ptr("n_row"), a.ptr("n_both"),
                                                a.ptr("pval_cooccur"), a.ptr("pval_exclusive"), last()),
                            device=where, what="dig_pair_fisher" + suffix, plain=True)
        counts = guarded_runs(dict(head, n_row=out("i32", H_total), n_both=out("i32", P)),
                              lambda a: _lib.call("dig_pair_counts" + suffix, *args(a), a.ptr("n_row"), a.ptr("n_both"), last()),
                              device=where, what="dig_pair_counts" + suffix, plain=True)
        for g in (full, counts):
            assert g["n_row"].tobytes() == n_row.tobytes() and g["n_both"].tobytes() == n_both.tobytes()
        n, r, k = nrk.T
        S.check_pvalues(full["pval_cooccur"], hypergeom.sf(n_both - 1, n, k, r), "dig_pair_fisher%s, guarded, PVAL_COOCCUR" % suffix)
        S.check_pvalues(full["pval_exclusive"], hypergeom.cdf(n_both, n, k, r), "dig_pair_fisher%s, guarded, PVAL_EXCLUSIVE" % suffix)
        x = np.arange(2, plan["n_max"] + 1)
        assert (full["lnfact"][:2] == 0).all() and np.allclose(full["lnfact"][2:], np.cumsum(np.log(x)), rtol=1e-13, atol=0)
        results.append(dict(got, **full))
    assert all(results[0][k].tobytes() == results[1][k].tobytes() for k in results[0])


def test_the_engine_route_works_on_the_current_stream(dev):
    """engine.pair_bits -- the zeroing of the matrix, the kernel -- and engine.pair_fisher -- the upload of the plan, the table, the
    row counts, the tiles -- inside a side stream while the default stream is busy (guarded_arena.side_stream_call)."""
    import torch
    from digdriver_amd import engine
    rows, ns = (70, 1, 5), (300, 10, 64)
    mats = [planted(h, n, h + n) for h, n in zip(rows, ns)]
    row, sample = (torch.as_tensor(x, device=dev) for x in keys_of(mats, np.random.default_rng(2)))

    def route(stream):
        bits = engine.pair_bits(row, sample, sum(rows), engine.pair_words(max(ns)))
        got = engine.pair_fisher(bits, rows, ns)
        return dict(bits=bits, **{k: got[k] for k in ("n_row", "n_both", "pval_cooccur", "pval_exclusive")})

    got = GA.side_stream_call(route, dev, "engine.pair_bits + engine.pair_fisher")
    want_bits = np.concatenate([S.bits_from_bool(m, engine.pair_words(max(ns))) for m in mats])
    n_row, n_both, nrk = S.pair_counts(want_bits, rows, ns)
    assert got["bits"].view(np.uint64).tobytes() == want_bits.tobytes()
    assert got["n_row"].tobytes() == n_row.tobytes() and got["n_both"].tobytes() == n_both.tobytes()
    st = S.pair_fisher(want_bits, rows, ns)
    S.check_pvalues(got["pval_cooccur"], st[2], "engine.pair_fisher on a side stream, against the statement")
    S.check_pvalues(got["pval_exclusive"], st[3], "engine.pair_fisher on a side stream, against the statement")
