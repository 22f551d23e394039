"""Every compiled form of three kernel families whose dispatch tables a command line can reach past what the other tests launch
("Compiled forms and the tests that launch them"):

A. the row walk base_tile_probs_rows_kernel<U, LW, TP, true> (dig_tiles_rows.hip): all twelve (LW, TP) pairs at U = 2 and at
   U = 1, whole and ragged trips, a non-ACGT base in every slot of a trip -- against the float64 oracle of
   tests/test_gpu_tile_cuts.py (1e-12), the general kernel (DIG_TILES_FORM=general, own process; 1e-13 as in
   tests/test_gpu_tiles.py) and, for U = 1, the trinucleotide kernels (1e-12);
B. the gene dot acc_dot_mfma_kernel<4, NT, NQ> at all nine (tiles, quads) cuts and a second chunk, and the no-workspace
   accumulate_kernel<4, WAVES> on both sides of its 16 / 8 / 4-wave switches (dig_accumulate.hip) -- against
   oracle.dig_oracle.accumulate_elements with the bounds of test_genic_accumulation_at_gene_set_size;
C. rbf_cross_kernel<D> for every D = 1 .. 32 and rbf_backward_kernel at both block edges (dig_gp.hip) -- against the definition
   evaluated in np.longdouble, with the bounds of test_rbf_cross_kernels_vs_numpy_and_autograd.

Only the parameter lists are new: oracles, bounds and helpers are those of the modules named above."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, rel_close
from test_gpu_tile_cuts import TRI_C, _check, _oracle, _problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# =====================================================================================================================================
# A. the row walk
# =====================================================================================================================================
ROW_BINSIZES = [10, 9, 19, 30, 12, 11, 35, 25, 49, 73, 7]      # trips of 10 | 12 | 25 | 8 positions
ROW_C = [1, 4, 5, 8, 9, 16, 17, 37]                             # walkers of 2, 4, 8 lanes; full and partial passes; 1 .. 3 launches
ROW_SHORT = {10: 7, 12: 7, 25: 5, 7: 20}                        # binsize -> n_tiles below what the regions hold, one per trip length
ROW_CASES = [(b, 0) for b in ROW_BINSIZES] + sorted(ROW_SHORT.items())      # (binsize, n_tiles; 0: what the longest region needs)
ROW_U1_C = [4, 8, 16]
N_EVERY = 37                                                    # the single-N region: one N every 37 bases
N_REGION = 6                                                    # its index


def _trip_positions(binsize):
    """launch_tile_probs_rows: the candidate that wastes the fewest slots of a tile's last trip; ties go to the earlier one."""
    best, tp = None, None
    for cand in (25, 12, 10, 8):
        waste = -(-binsize // cand) * cand - binsize
        if best is None or waste < best:
            best, tp = waste, cand
    return tp


def _walker_lanes(C):
    """launch_tile_probs_rows: (lanes per walker, cohorts) of every launch of a call with C cohorts."""
    out, c0 = [], 0
    while c0 < C:
        left = C - c0
        lw = 8 if left > 8 else (4 if left > 4 else 2)
        cc = min(left, 2 * lw)
        out.append((lw, cc))
        c0 += cc
    return out


def _row_problem():
    """_problem() of tests/test_gpu_tile_cuts.py (the 40-base N run, the START == 0 region, the region cut by the chromosome end,
    the 300-position region -- a whole number of trips of 10, 12 and 25 -- and the empty region) with a single N every 37 bases
    over 300 positions of chr2, a region over them, one over the same bases from an odd offset, and an N-free region at an odd
    offset.  Every region holds at most 300 positions: the row walk keeps all of them at binsize >= 2."""
    seqs, regions, S3, S5 = _problem()
    chr2 = np.array(list(seqs["chr2"]))
    chr2[np.arange(602, 900, N_EVERY)] = "N"
    seqs = dict(seqs, chr2="".join(chr2))
    regions = list(regions) + [("chr2", 600, 900),              # N_REGION: eight single N
                               ("chr2", 613, 897),              # the same bases from an odd offset, 284 positions
                               ("chr1", 1501, 1790)]            # odd offset, 289 positions, no N
    return seqs, regions, S3, S5


def _region_positions(seqs, regions, n_up):
    """(first position, number of positions) of every region, as _oracle forms them."""
    out = []
    for chrom, start, end in regions:
        first = n_up if start == 0 else start
        out.append((first, max(min(end, len(seqs[chrom]) - n_up) - first, 0)))
    return out


def test_row_walk_cases_reach_every_form_and_trip_kind():
    """No GPU.  The selection rules of launch_tile_probs_rows, mirrored, say what the lists above launch: all twelve (LW, TP)
    pairs; for each of the trip lengths this file adds (10, 12, 25; 8 keeps binsize 7, its other bin sizes are in
    tests/test_gpu_tiles.py) a whole single trip, a ragged single trip and a tile of several trips whose last one is ragged; a
    non-ACGT base at every slot of a trip.  When the rule changes, the assertion that fails names the form that lost its cases."""
    table = {8: [], 10: [], 12: [], 25: []}
    for b in range(1, 51):
        table[_trip_positions(b)].append(b)
    r = lambda *spans: [b for lo, hi in spans for b in range(lo, hi + 1)]
    assert table == {8: r((1, 8), (13, 16), (31, 32)), 10: r((9, 10), (17, 20), (26, 30), (37, 40)),
                     12: r((11, 12), (21, 24), (33, 36), (41, 48)), 25: r((25, 25), (49, 50))}
    for tp, more in ((8, [64]), (12, r((57, 60))), (25, r((73, 75), (97, 100)))):
        assert all(_trip_positions(b) == tp for b in more), tp
    assert [_trip_positions(b) for b in ROW_BINSIZES] == [10, 10, 10, 10, 12, 12, 12, 25, 25, 25, 8]
    assert sorted(_trip_positions(b) for b in ROW_SHORT) == [8, 10, 12, 25]
    assert [_walker_lanes(C) for C in ROW_C] == [[(2, 1)], [(2, 4)], [(4, 5)], [(4, 8)], [(8, 9)], [(8, 16)], [(8, 16), (2, 1)],
                                                 [(8, 16), (8, 16), (4, 5)]]
    pairs = {(lw, _trip_positions(b)) for b in ROW_BINSIZES for C in ROW_C for lw, _ in _walker_lanes(C)}
    assert pairs == {(lw, tp) for lw in (2, 4, 8) for tp in (8, 10, 12, 25)}
    assert {lw for C in ROW_U1_C for lw, _ in _walker_lanes(C)} == {2, 4, 8}
    seqs, regions, _, _ = _row_problem()
    assert len(regions) == 9 and regions[N_REGION] == ("chr2", 600, 900)
    for n_up in (1, 2):
        spans = _region_positions(seqs, regions, n_up)
        assert max(n for _, n in spans) == 300 and sum(n == 300 for _, n in spans) == 2 and sum(n == 0 for _, n in spans) == 1
        assert sum(first % 2 == 1 and n > 0 for first, n in spans) >= 2
        kinds, slots = {}, {}
        for b in ROW_BINSIZES:
            tp = _trip_positions(b)
            n_trips = -(-b // tp)
            for (chrom, _, _), (first, n_pos) in zip(regions, spans):
                lengths = {b} if n_pos >= b else set()
                if n_pos % b:
                    lengths.add(n_pos % b)
                for ln in lengths:
                    if n_trips == 1:
                        kinds.setdefault(tp, set()).add("whole single" if ln == tp else "ragged single")
                    elif ln % tp:
                        kinds.setdefault(tp, set()).add("several, last ragged")
                for j in range(n_pos):
                    if seqs[chrom][first + j] == "N":
                        slots.setdefault(tp, set()).add(j % b % tp)
        assert all(t < -(-300 // b) for b, t in ROW_SHORT.items())     # fewer tiles asked for than the 300-position regions hold
        for tp in (10, 12, 25):
            assert kinds[tp] == {"whole single", "ragged single", "several, last ragged"}, (tp, kinds[tp])
        for tp in (8, 10, 12, 25):
            assert slots[tp] == set(range(tp)) or (tp == 8 and slots[tp] == set(range(7))), (tp, sorted(slots[tp]))


_CHILD = ("import sys, numpy as np, torch; sys.path.insert(0, %r); from digdriver_amd import engine; "
          "from digdriver_amd.data_tools.genome import PackedGenome; d = np.load(sys.argv[1], allow_pickle=True); "
          "g = PackedGenome.from_sequences(d['seqs'].item()); out = {}\n"
          "for k, (binsize, n_tiles, C) in enumerate(d['cases']):\n"
          "    pt, f, nv = engine.base_tile_probs(g, list(d['chroms']), d['starts'], d['ends'], d['S'][:C], int(binsize), "
          "n_tiles=(int(n_tiles) or None), device=0)\n"
          "    out['pt%%d' %% k], out['f%%d' %% k], out['n%%d' %% k] = pt.cpu().numpy(), f.cpu().numpy(), nv.cpu().numpy()\n"
          "np.savez(sys.argv[2], **out)") % ROOT


def _child(tmp, name, form, rp, S, cases):
    """One fresh process with DIG_TILES_FORM=form that computes every case and saves it (started with subprocess; the caller
    waits for it before it starts the next)."""
    src, dst = os.path.join(tmp, name + "_in.npz"), os.path.join(tmp, name + ".npz")
    np.savez(src, seqs=np.array(rp["seqs"], dtype=object), chroms=np.array(rp["chroms"]), starts=rp["starts"], ends=rp["ends"], S=S,
             cases=np.array(cases, np.int64))
    subprocess.check_call([sys.executable, "-c", _CHILD, src, dst], env=dict(os.environ, DIG_TILES_FORM=form))
    d = np.load(dst)
    return {tuple(case): (d["pt%d" % k], d["f%d" % k], d["n%d" % k]) for k, case in enumerate(cases)}


@pytest.fixture(scope="module")
def rp():
    """The row-walk problem on the device, the call, and the oracles (once per case, for all 37 cohorts)."""
    from digdriver_amd import _lib, engine
    from digdriver_amd.data_tools.genome import PackedGenome
    _lib.require_device()
    seqs, regions, S3, S5 = _row_problem()
    genome = PackedGenome.from_sequences(seqs)
    chroms = [r[0] for r in regions]
    starts, ends = np.array([r[1] for r in regions], np.int64), np.array([r[2] for r in regions], np.int64)

    def run(S, binsize, n_tiles):
        pt, first, nval = engine.base_tile_probs(genome, chroms, starts, ends, S, binsize, n_tiles=n_tiles or None, device=0)
        return pt.cpu().numpy(), first.cpu().numpy(), nval.cpu().numpy()

    want = lambda S, n_up: {(b, t): _oracle(seqs, regions, S, n_up, b, t or -(-300 // b)) for b, t in ROW_CASES}
    return dict(seqs=seqs, chroms=chroms, starts=starts, ends=ends, run=run, S5=S5, S3=S3[:max(ROW_U1_C)], want5=want(S5, 2),
                want3=want(S3[:max(ROW_U1_C)], 1))


@pytest.fixture(scope="module")
def general(rp, tmp_path_factory):
    return _child(str(tmp_path_factory.mktemp("general")), "general", "general", rp, rp["S5"], [(b, t, C) for b, t in ROW_CASES for C in ROW_C])


@pytest.fixture(scope="module")
def rows_u1(rp, tmp_path_factory):
    return _child(str(tmp_path_factory.mktemp("rows_u1")), "rows", "rows", rp, rp["S3"], [(b, t, C) for b, t in ROW_CASES for C in ROW_U1_C])


@pytest.mark.gpu
@pytest.mark.parametrize("C", ROW_C)
@pytest.mark.parametrize("binsize,n_tiles", ROW_CASES)
def test_row_walk_forms_against_the_oracle_and_the_general_kernel(rp, general, binsize, n_tiles, C):
    got = rp["run"](rp["S5"][:C], binsize, n_tiles)
    want = rp["want5"][binsize, n_tiles]
    _check(got, want, C)
    assert (got[2] >= 0).all() and got[2].max() == (n_tiles or -(-300 // binsize))      # no region was left to the general kernel
    assert np.isfinite(got[0][:, N_REGION, :got[2][N_REGION]]).all()
    if n_tiles:
        assert np.nansum(got[0][0, 4]) < 0.9                            # positions behind the last tile count for the total only
    gpt, gfirst, gnval = general[binsize, n_tiles, C]
    assert np.array_equal(got[1], gfirst) and np.array_equal(got[2], gnval)
    assert np.array_equal(np.isnan(got[0]), np.isnan(gpt))
    np.testing.assert_allclose(got[0], gpt, rtol=1e-13, equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("C", ROW_U1_C)
@pytest.mark.parametrize("binsize,n_tiles", ROW_CASES)
def test_row_walk_trinucleotide_forms_against_the_matrix_kernels(rp, rows_u1, binsize, n_tiles, C):
    """The twelve U = 1 forms (DIG_TILES_FORM=rows, own process) against what dig_base_tile_probs runs for 64-entry tables, and
    against the oracle."""
    pt, first, nval = rows_u1[binsize, n_tiles, C]
    _check((pt, first, nval), rp["want3"][binsize, n_tiles], C)
    mpt, mfirst, mnval = rp["run"](rp["S3"][:C], binsize, n_tiles)
    assert np.array_equal(first, mfirst) and np.array_equal(nval, mnval)
    assert np.array_equal(np.isnan(pt), np.isnan(mpt))
    np.testing.assert_allclose(pt, mpt, rtol=1e-12, equal_nan=True)


# =====================================================================================================================================
# B. gene accumulation (n_class = 4)
# =====================================================================================================================================
GENE_E = 33                                                     # two 16-row tiles and one row
GENE_NOWS_C = [27, 28, 53, 54, 64, 65]                          # 16 | 8 waves, 8 | 4 waves, one launch of 64 | 64 + 1
ACC_FLOAT, ACC_INT = ("MU", "SIGMA", "P", "P_INDEL"), ("R_OBS", "FLAG", "R_SIZE", "ELT_SIZE")


def _cut(C, chunk=0):
    """chunk_cut of dig_common.hpp: (full 16-cohort tiles, tail quads) of a 48-cohort chunk."""
    rem = min(C - 48 * chunk, 48)
    full, r = rem // 16, rem % 16
    return (full, -(-r // 4)) if r <= 8 else (full + 1, 0)


def _nows_waves(cc, n_class=4):
    """launch_acc_v1: waves of the no-workspace kernel for cc cohorts of a launch."""
    waves = 16
    while waves > 4 and (192 + 64) * cc * 8 + (n_class * 192 + 64) * 8 * waves > 160 * 1024 - 1024:
        waves //= 2
    return waves


def test_gene_cases_reach_every_cut_and_wave_count():
    """No GPU.  TRI_C holds all nine cuts of a chunk in its first chunk and two more in a second one; GENE_NOWS_C stands on both
    sides of the wave-count switches of the four-class no-workspace kernel."""
    nine = {(0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2), (3, 0)}
    assert {_cut(C) for C in TRI_C} == nine
    assert [(_cut(C), _cut(C, 1)) for C in (49, 85)] == [((3, 0), (0, 1)), ((3, 0), (2, 2))]
    assert [_nows_waves(min(C, 64)) for C in GENE_NOWS_C] == [16, 8, 8, 4, 4, 4] and _nows_waves(1) == 16


@functools.lru_cache(maxsize=None)
def _gene_workload(C, zeros=False):
    """make_workload(900, 33, C) turned into a gene workload as test_genic_accumulation_at_gene_set_size does (four classes,
    gene_length), and the oracle's accumulation; computed once per cohort count and left unchanged.  zeros (C = 17): cohort 15 --
    the last of the full tile -- and cohort 16 -- the single cohort of the quad -- hold one zero table entry each, and gene 7
    overlaps no bin, so that its denominators are 0: inf where the table is positive and the class row holds no zero, NaN
    otherwise (genic_driver_tools.py:361-366)."""
    from bench import make_workload
    from oracle import dig_oracle as O
    w = make_workload(n_bins=900, n_elements=GENE_E, n_cohorts=C, seed=11 + C)
    rng = np.random.default_rng(1)
    L1 = w["L"].reshape(GENE_E, -1)[:, :192]
    L4 = np.ascontiguousarray(np.stack([L1] + [rng.poisson(L1 * f).astype(np.int32) for f in (0.7, 0.2, 0.1)], axis=1))
    glen = rng.integers(300, 9000, GENE_E).astype(np.int32)
    if zeros:
        w = dict(w)
        d_pr = w["d_pr"].copy()
        d_pr[15, 100] = 0.0
        d_pr[16, 5] = 0.0
        w["d_pr"] = d_pr
        n7 = int(w["ov_ptr"][8] - w["ov_ptr"][7])
        w["ov_idx"] = np.ascontiguousarray(np.delete(w["ov_idx"], np.arange(w["ov_ptr"][7], w["ov_ptr"][8])))
        ptr = w["ov_ptr"].copy()
        ptr[8:] -= n7
        w["ov_ptr"] = ptr
        L4[7, 0] = np.maximum(L4[7, 0], 1)                      # a class row without a zero
        L4[7, 3, 17] = 0                                        # and one with
    want = O.accumulate_elements(w["bin_mu"], w["bin_std"], w["bin_y"], w["bin_flag"], w["bin_ctx"], w["ov_ptr"], w["ov_idx"], L4,
                                 w["strand_minus"].astype(bool), w["d_pr"], gene_length=glen)
    return w, L4, glen, want


_GENE_RUNS = {}


def _gene_run(C, dev, use_workspace=True, zeros=False):
    """engine.accumulate_elements on device tensors, as host arrays (once per case)."""
    import torch
    key = (C, use_workspace, zeros)
    if key not in _GENE_RUNS:
        from digdriver_amd import engine
        w, L4, glen, _ = _gene_workload(C, zeros)
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
        acc = engine.accumulate_elements(t(w["bin_mu"]), t(w["bin_std"]), t(w["bin_y"]), t(w["bin_flag"]), t(w["bin_ctx"]), t(w["ov_ptr"]),
                                         t(w["ov_idx"]), t(L4), t(w["strand_minus"]), t(w["d_pr"]), gene_length=t(glen),
                                         use_workspace=use_workspace)
        torch.cuda.synchronize()
        _GENE_RUNS[key] = {k: v.cpu().numpy() for k, v in acc.items()}
    return _GENE_RUNS[key]


def _gene_check(got, want, C):
    """The bounds of test_genic_accumulation_at_gene_set_size."""
    assert got["P"].shape == (GENE_E, 4, C)
    np.testing.assert_allclose(got["MU"], want["MU"], rtol=1e-12)
    np.testing.assert_allclose(got["SIGMA"], want["SIGMA"], rtol=1e-12)
    np.testing.assert_allclose(got["P"], want["P"], rtol=1e-11)
    np.testing.assert_allclose(got["P_INDEL"], want["P_INDEL"], rtol=1e-15)
    for name in ACC_INT:
        assert np.array_equal(got[name], want[name]), name


@pytest.fixture(scope="module")
def dev():
    import torch
    from digdriver_amd import _lib
    _lib.require_device()
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("C", TRI_C)
def test_gene_dot_at_every_cohort_cut(dev, C):
    w, L4, glen, want = _gene_workload(C)
    assert np.isfinite(want["P"]).all() and (want["P"][:, 0] > 0).all()
    got = _gene_run(C, dev)
    _gene_check(got, want, C)
    if C in (17, 49):                                           # host arrays in: the bits of the device tensors
        from digdriver_amd import engine
        host = engine.accumulate_elements(w["bin_mu"], w["bin_std"], w["bin_y"], w["bin_flag"], w["bin_ctx"], w["ov_ptr"], w["ov_idx"], L4,
                                          w["strand_minus"], w["d_pr"], gene_length=glen)
        assert sorted(host) == sorted(got)
        for name in got:
            assert isinstance(host[name], np.ndarray) and host[name].tobytes() == got[name].tobytes(), name


@pytest.mark.gpu
@pytest.mark.parametrize("C", GENE_NOWS_C)
def test_gene_accumulation_without_workspace_at_every_wave_count(dev, C):
    """accumulate_kernel<4, 16 | 8 | 4> against the workspace form with the bound of _accumulate_vs_oracle (1e-12, integers exact),
    and against the oracle."""
    got, ref = _gene_run(C, dev, use_workspace=False), _gene_run(C, dev)
    for name in ACC_FLOAT:
        rel_close(got[name], ref[name], 1e-12)
    for name in ACC_INT:
        assert np.array_equal(got[name], ref[name]), name
    want = _gene_workload(C)[3]
    _gene_check(got, want, C)
    _gene_check(ref, want, C)


@pytest.mark.gpu
def test_gene_pipeline_accumulation_equals_the_separate_call(dev):
    """engine.gene_pipeline at C = 17 (one tile and a one-cohort quad): its accumulation outputs are those of
    engine.accumulate_elements bit for bit."""
    import torch
    from digdriver_amd import engine
    C = 17
    w, L4, glen, want = _gene_workload(C)
    rng = np.random.default_rng(6)
    obs = rng.poisson(1.5, (GENE_E, 5, C)).astype(np.int32)
    syn, mis, nons, spl = obs[:, 0], obs[:, 1], obs[:, 2], obs[:, 3]
    per_class = np.stack([syn, mis, nons, spl, nons + spl, mis + nons + spl], axis=1)
    n_samp = rng.binomial(per_class, 0.9).astype(np.int32)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    acc, st = engine.gene_pipeline(t(w["bin_mu"]), t(w["bin_std"]), t(w["bin_y"]), t(w["bin_flag"]), t(w["bin_ctx"]), t(w["ov_ptr"]),
                                   t(w["ov_idx"]), t(L4), t(w["strand_minus"]), t(glen), t(w["d_pr"]), t(obs), t(n_samp), t(w["cj"]),
                                   t(rng.uniform(0.05, 0.3, C)))
    torch.cuda.synchronize()
    sep = _gene_run(C, dev)
    assert sorted(acc) == sorted(sep)
    for name in sep:
        assert acc[name].cpu().numpy().tobytes() == sep[name].tobytes(), name
    _gene_check(sep, want, C)
    assert len(st) == len(engine.GS_PLANES)


def test_oracle_reproduces_the_zero_denominator_golden():
    """No GPU: the premise of the next test.  oracle.dig_oracle.accumulate_elements gives the reference's own NaN pattern and values
    where a cohort's table is zero (tests/golden/accumulate_zero_golden.npz) -- the check of tests/test_oracle_golden.py."""
    from oracle import dig_oracle as O
    d = np.load(os.path.join(GOLDEN, "accumulate_zero_golden.npz"))
    from test_oracle_golden import test_py_oracle_zero_denominators_follow_the_reference as golden_check
    golden_check()
    # and what the next test relies on: gene 7 without a bin, cohorts 15 and 16 with a zero entry
    w, L4, glen, want = _gene_workload(17, True)
    assert w["ov_ptr"][7] == w["ov_ptr"][8] and w["ov_ptr"][-1] == len(w["ov_idx"]) and (np.diff(w["ov_ptr"]) >= 0).all()
    P = want["P"]
    assert np.isfinite(np.delete(P, 7, axis=0)).all()           # a zero entry beside a positive denominator changes nothing
    assert np.isposinf(P[7, 0, :15]).all() and np.isnan(P[7, 0, 15:]).all() and np.isnan(P[7, 3]).all()
    assert want["R_SIZE"][7] == 0 and np.isposinf(want["P_INDEL"][7]) and d["p_sum"].shape[0] == 3


@pytest.mark.gpu
@pytest.mark.parametrize("use_workspace", [True, False])
def test_gene_dot_with_zero_table_entries_gives_the_oracles_nan_and_inf(dev, use_workspace):
    """g_cohort_bad at four classes: the last cohort of the full tile and the single cohort of the quad hold a zero; a gene
    without bins has denominator 0 in every cohort.  NaN and inf exactly where the oracle has them, the rest within the usual
    bounds."""
    C = 17
    want = _gene_workload(C, True)[3]
    got = _gene_run(C, dev, use_workspace=use_workspace, zeros=True)
    for name in ("P", "P_INDEL"):
        assert np.array_equal(np.isnan(got[name]), np.isnan(want[name])), name
        assert np.array_equal(np.isposinf(got[name]), np.isposinf(want[name])), name
        assert not np.isneginf(got[name]).any()
    ok = np.isfinite(want["P"])
    np.testing.assert_allclose(got["P"][ok], want["P"][ok], rtol=1e-11)
    ok = np.isfinite(want["P_INDEL"])
    np.testing.assert_allclose(got["P_INDEL"][ok], want["P_INDEL"][ok], rtol=1e-15)
    np.testing.assert_allclose(got["MU"], want["MU"], rtol=1e-12)
    np.testing.assert_allclose(got["SIGMA"], want["SIGMA"], rtol=1e-12)
    for name in ACC_INT:
        assert np.array_equal(got[name], want[name]), name


# =====================================================================================================================================
# C. the RBF cross-covariance
# =====================================================================================================================================
RBF_OS = 1.7
RBF_M = [1, 15, 16, 17, 33]                                     # around the 16-row group of rbf_cross_kernel
RBF_N = [1, 255, 256, 257, 1023, 1024, 1025, 2049]              # around its 256-column block and the backward's 1 024-column chunk
RBF_DIAGONAL = list(zip(RBF_M, RBF_N))                          # gradients: (1, 1), (15, 255), (16, 256), (17, 257), (33, 1023)


def _rbf_points(m, n, d):
    rng = np.random.default_rng(1000 * d + 7 * m + n)
    return rng.normal(size=(m, d)), rng.normal(size=(n, d)), 0.9 + 0.2 * d ** 0.5


def _rbf_reference(Z, X, ls, osc):
    """os exp(-|z - x|^2 / (2 l^2)) from direct differences in np.longdouble, rounded to float64."""
    Zl, Xl = Z.astype(np.longdouble), X.astype(np.longdouble)
    d2 = ((Zl[:, None, :] - Xl[None, :, :]) ** 2).sum(-1)
    return (np.longdouble(osc) * np.exp(-d2 / (2 * np.longdouble(ls) ** 2))).astype(np.float64)


def _rbf_values(dev, m, n, d):
    import torch
    from digdriver_amd.region_model.trainers import gp_trainer as G
    Zn, Xn, ls = _rbf_points(m, n, d)
    Z, X = torch.tensor(Zn, device=dev, requires_grad=True), torch.tensor(Xn, device=dev)
    lst = torch.tensor(ls, device=dev, dtype=torch.float64, requires_grad=True)
    osc = torch.tensor(RBF_OS, device=dev, dtype=torch.float64, requires_grad=True)
    K = G._RbfCross.apply(Z, X, lst, osc)
    assert K.shape == (m, n)
    np.testing.assert_allclose(K.detach().cpu().numpy(), _rbf_reference(Zn, Xn, ls, RBF_OS), rtol=1e-13, atol=1e-300)
    return K, Z, X, lst, osc


def _rbf_gradients(dev, K, Z, X, lst, osc):
    """The backward kernel against autograd of the elementwise form: rtol 1e-10, atol 1e-12."""
    import torch
    g = torch.tensor(np.random.default_rng(K.shape[1]).normal(size=tuple(K.shape)), device=dev)
    (K * g).sum().backward()
    got = [Z.grad.clone(), lst.grad.clone(), osc.grad.clone()]
    for t in (Z, lst, osc):
        t.grad = None
    ref = osc * torch.exp(-0.5 * ((Z[:, None, :] - X[None, :, :]) ** 2).sum(-1) / lst ** 2)
    (ref * g).sum().backward()
    for a, b in zip(got, (Z.grad, lst.grad, osc.grad)):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-10, atol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("d", range(1, 33))
def test_rbf_cross_at_every_feature_count(dev, d):
    """(m, n) = (17, 1025): a second row group of one row, a fifth column block of one column, a second backward chunk of one."""
    _rbf_gradients(dev, *_rbf_values(dev, 17, 1025, d))


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 16, 32])
@pytest.mark.parametrize("m", RBF_M)
def test_rbf_cross_at_both_block_edges(dev, d, m):
    for n in RBF_N:
        args = _rbf_values(dev, m, n, d)
        if (m, n) in RBF_DIAGONAL:
            _rbf_gradients(dev, *args)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 16, 32])
def test_rbf_cross_end_values(dev, d):
    """A row of Z equal to a row of X: K == outputscale, bit for bit.  A pair with c d^2 < -745: K == 0.0, and in the backward pass
    W == 0 there and finite gradients (the k > 0 branch of rbf_backward_kernel)."""
    import torch
    from digdriver_amd import _lib
    from digdriver_amd.region_model.trainers import gp_trainer as G
    m, n = 17, 1025
    Zn, Xn, ls = _rbf_points(m, n, d)
    Zn[3], Zn[16] = Xn[1024], Xn[0]                             # equal rows, in both row groups and both backward chunks
    Xn[300] = Zn[5] + 40.0 * ls / d ** 0.5                      # |z - x|^2 = 1600 l^2: c d^2 = -800
    Xn[1023] = Zn[16] - 40.0 * ls / d ** 0.5
    Z, X = torch.tensor(Zn, device=dev, requires_grad=True), torch.tensor(Xn, device=dev)
    lst = torch.tensor(ls, device=dev, dtype=torch.float64, requires_grad=True)
    osc = torch.tensor(RBF_OS, device=dev, dtype=torch.float64, requires_grad=True)
    K = G._RbfCross.apply(Z, X, lst, osc)
    Kn = K.detach().cpu().numpy()
    want = _rbf_reference(Zn, Xn, ls, RBF_OS)
    assert want[3, 1024] == RBF_OS and want[16, 0] == RBF_OS and want[5, 300] == 0.0 and want[16, 1023] == 0.0
    assert Kn[3, 1024] == RBF_OS and Kn[16, 0] == RBF_OS
    assert Kn[5, 300] == 0.0 and Kn[16, 1023] == 0.0 and not np.signbit(Kn[5, 300])
    np.testing.assert_allclose(Kn, want, rtol=1e-13, atol=1e-300)
    # the backward kernel itself, for W; then the gradients through autograd
    g = torch.tensor(np.random.default_rng(d).normal(size=(m, n)), device=dev)
    W = torch.full_like(K, float("nan"))
    part = torch.full((m, (n + 1023) // 1024, 2), float("nan"), dtype=torch.float64, device=dev)
    _lib.call("dig_rbf_backward", _lib.dev_ptr(g), _lib.dev_ptr(K.detach()), m, n, ls, RBF_OS, _lib.dev_ptr(W), _lib.dev_ptr(part),
              _lib.stream_ptr())
    torch.cuda.synchronize()
    Wn = W.cpu().numpy()
    assert Wn[5, 300] == 0.0 and Wn[16, 1023] == 0.0 and np.isfinite(Wn).all() and np.isfinite(part.cpu().numpy()).all()
    assert np.array_equal(Wn, g.cpu().numpy() * Kn)
    _rbf_gradients(dev, K, Z, X, lst, osc)
    for t in (Z, lst, osc):
        assert bool(torch.isfinite(t.grad).all())
