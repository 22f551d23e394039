"""Pairs of the many-cohort element route (cohort_batch.run_element_pairs, `DigDriver.py elementCohorts --pairs`) on a synthetic set
built by the recipe of tests/test_gpu_onthefly.py: 3 cohorts of 40, 90 and 130 samples, 200 elements.  Planted in cohorts 0 and 1: a pair
of elements hit in the same samples, a pair hit in disjoint samples, a pair that shares bases (hit by the same mutations), a sample
with more mutations than --max-muts-per-sample (blacklisted); cohort 2 has one mutation per element and no call.
The frames are checked against a pandas / scipy statement built from the mutation files alone (the incidence: a row of the file hits an
element where [START, END) meets one of its blocks), the q-values against nb_model.get_q_vals, the written files by reading them back,
and the command's other files for being the bytes of a run without --pairs."""
import os

import numpy as np
import pandas as pd
import pytest

from test_row_select_host import _cli

pytestmark = pytest.mark.gpu

N_SAMPLES = (40, 90, 130)
MAX_MUTS = 100
CUT = dict(pval_max=1e-3)
SAME, APART, SHARED = ("E001", "E002"), ("E003", "E004"), ("E005", "E199")


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return _build_case(tmp_path_factory.mktemp("element_pairs"))


def _build_case(tmp_path):
    from digdriver_amd import _lib
    from digdriver_amd.io import mapfile
    from digdriver_amd.sequence_model import sequence_tools
    from oracle import dig_oracle as O
    _lib.require_device()
    rng = np.random.default_rng(77)
    window, nbins = 1000, {"1": 300, "2": 220}
    fa = tmp_path / "genome.fa"
    with open(fa, "w") as f:
        for c, n in nbins.items():
            s = rng.choice(np.frombuffer(b"ACGT", np.uint8), n * window).tobytes().decode()
            f.write(">chr%s\n" % c)
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60] + "\n")
    grid = pd.DataFrame([(int(c), b * window, (b + 1) * window) for c, n in nbins.items() for b in range(n)], columns=["CHROM", "START", "END"])
    grid.index = ["chr{}:{}-{}".format(c, s, e) for c, s, e in zip(grid.CHROM, grid.START, grid.END)]
    seq_rows = O.model_rows192()
    # 200 elements of 1 - 3 blocks, 2 500 bases apart so that no two share a base -- but E199, laid over the first block of E005
    elts, lines = [], []
    for i in range(200):
        c, st = ("1", i * 2500 + 100) if i < 115 else ("2", (i - 115) * 2500 + 100)
        blocks, off = [], 0
        for _ in range(int(rng.integers(1, 4))):
            z = int(rng.integers(150, 600))
            blocks.append((off, z))
            off += z + int(rng.integers(10, 150))
        if i == 199:
            c, st, blocks = "1", elts[5][3][0][0] + 40, [(0, 300)]
        name = "E%03d" % i
        lines.append("%s\t%d\t%d\t%s\t0\t%s\t%d\t%d\t.\t%d\t%s,\t%s,\n" % (
            c, st, st + blocks[-1][0] + blocks[-1][1], name, "+-"[i % 2], st, st, len(blocks), ",".join(str(z) for _, z in blocks),
            ",".join(str(o) for o, _ in blocks)))
        elts.append((name, c, "+-"[i % 2], [(st + o, st + o + z) for o, z in blocks]))
    bed = tmp_path / "elts.bed"
    bed.write_text("".join(lines))
    by_name = {e[0]: e for e in elts}
    pres, muts = [], []
    for c, n in enumerate(N_SAMPLES):
        rp = grid.copy()
        rp["Y_TRUE"], rp["Y_PRED"], rp["STD"] = 0, rng.gamma(9.0, 3.0, len(rp)), rng.gamma(4.0, 1.0, len(rp))
        rp["Y_TRUE"] = rng.poisson(rp.Y_PRED.values)
        rp["MAPP"], rp["QUANT"], rp["FLAG"] = 1.0, 0.5, rng.uniform(size=len(rp)) < 0.1
        sm = pd.DataFrame({"MUT_TYPE": [m for m, _ in seq_rows], "CONTEXT": [x for _, x in seq_rows], "COUNT": rng.integers(1, 1000, 192),
                           "FREQ": rng.dirichlet(np.ones(192)) * 1e-3})
        pre = str(tmp_path / ("cohort%d.map" % c))
        mapfile.write_frame(pre, "region_params", rp)
        mapfile.write_frame(pre, "sequence_model_192", sm)
        mapfile.write_array(pre, "idx", rp[["CHROM", "START", "END"]].values.astype(np.int32))
        mapfile.write_attrs(pre, cohort_name="c%d" % c, mappability_threshold=0.5)
        rows = []

        def snv(name, sample, at=None):
            _, ch, _, blocks = by_name[name]
            s, e = blocks[int(rng.integers(0, len(blocks)))]
            p = int(rng.integers(s, e)) if at is None else at
            rows.append((ch, p, p + 1, "A", "T", sample, ".", "Noncoding", "A>T", "CAG"))

        for i, (name, _, _, _) in enumerate(elts):               # the background: one mutation per element, every sample in turn
            snv(name, "S%d" % (i % n))
        if c < 2:
            same = rng.choice(n, 12, replace=False)
            for name in SAME:                                     # hit in the same 12 samples
                for s in same:
                    snv(name, "S%d" % s)
            for k, name in enumerate(APART):                      # hit in 15 samples each, none in common
                for s in range(15 * k, 15 * k + 15):
                    snv(name, "S%d" % s)
            lo = by_name[SHARED[1]][3][0][0]
            for s in rng.choice(n, 10, replace=False):            # one mutation inside both elements of the overlapping pair
                snv(SHARED[0], "S%d" % s, at=lo + int(rng.integers(0, 100)))
            for i in range(6, 14):                                # more called elements, hit in 8 - 14 samples each
                for s in rng.choice(n, int(rng.integers(8, 15)), replace=False):
                    snv("E%03d" % i, "S%d" % s)
            rows.append(("1", by_name["E006"][3][0][0], by_name["E006"][3][0][0] + 3, "AGG", "A", "S1", ".", "INDEL", "DEL", "."))
            for i in range(20, 80):                               # a hypermutator: 120 mutations, two of them in E007
                snv("E%03d" % i, "HYPER"), snv("E%03d" % i, "HYPER")
            snv("E007", "HYPER"), snv("E007", "HYPER")
        for _ in range(60):                                       # mutations outside the elements
            p = int(rng.integers(2400, 2480)) + 2500 * int(rng.integers(0, 80))
            rows.append(("1", p, p + 1, "C", "G", "S%d" % rng.integers(0, n), ".", "Noncoding", "C>G", "ACA"))
        rows += rows[:5]                                          # exact duplicates
        f = tmp_path / ("muts%d.tsv" % c)
        pd.DataFrame(rows).to_csv(f, sep="\t", header=False, index=False)
        pres.append(pre)
        muts.append(str(f))
    gc, ed = str(tmp_path / "gc.map"), str(tmp_path / "ed.map")
    win = sequence_tools.count_contexts_in_bed(str(fa), grid[["CHROM", "START", "END"]], n_up=1, n_down=1)
    mapfile.write_frame(gc, "all_window_genome_counts", win)
    mapfile.write_array(gc, "idx", grid[["CHROM", "START", "END"]].values.astype(np.int32))
    sequence_tools.initialize_nonc_data(ed, gc, window)
    L = sequence_tools.precount_region_contexts_parallel(str(bed), str(fa), 1, window, True)
    sequence_tools.preprocess_nonc(str(bed), ed, pres[0], L, "elts", window)
    return dict(muts=muts, pres=pres, ed=ed, tmp=tmp_path, elts=by_name, kw=dict(max_muts_per_sample=MAX_MUTS))


def _incidence(path, elts):
    """From the mutation file alone: ({element: set of samples with a kept row in it}, the samples that are not blacklisted)."""
    m = pd.read_csv(path, sep="\t", header=None).iloc[:, :6].drop_duplicates()
    m.columns = ["CHROM", "START", "END", "REF", "ALT", "SAMPLE"]
    hit = {name: set() for name in elts}
    load = {}
    for name, (_, ch, _, blocks) in elts.items():
        on = m[m.CHROM.astype(str) == ch]
        inside = np.zeros(len(on), bool)
        for s, e in blocks:
            inside |= (on.START.values < e) & (on.END.values > s)
        for smp, k in on[inside].SAMPLE.value_counts().items():
            load[smp] = load.get(smp, 0) + int(k)
            hit[name].add(smp)
    black = {s for s, k in load.items() if k > MAX_MUTS}
    samples = [s for s in pd.unique(m.SAMPLE) if s not in black]
    return {name: v - black for name, v in hit.items()}, samples


def _share_a_base(a, b):
    return a[1] == b[1] and any(s1 < e2 and s2 < e1 for s1, e1 in a[3] for s2, e2 in b[3])


def _statement(case, c, called, n=None, min_samples=1):
    """Every pair of the called elements (in their order) of cohort c, as the frame's columns, from the mutation file."""
    from scipy.stats import hypergeom

    from digdriver_amd.sequence_model import nb_model
    hit, samples = _incidence(case["muts"][c], case["elts"])
    n = len(samples) if n is None else n
    enter = [e for e in called if len(hit[e]) >= min_samples]
    rows = []
    for i, a in enumerate(enter):
        for b in enter[i + 1:]:
            na, nb_, both = len(hit[a]), len(hit[b]), len(hit[a] & hit[b])
            shared = _share_a_base(case["elts"][a], case["elts"][b])
            odds = np.log2((both + 0.5) * (n - na - nb_ + both + 0.5) / ((na - both + 0.5) * (nb_ - both + 0.5)))
            rows.append(dict(ELT_A=a, ELT_B=b, N_SAMPLES=n, N_A=na, N_B=nb_, N_BOTH=both, N_A_ONLY=na - both, N_B_ONLY=nb_ - both,
                             N_NEITHER=n - na - nb_ + both, LOG2_ODDS=odds,
                             PVAL_COOCCUR=np.nan if shared else hypergeom.sf(both - 1, n, nb_, na),
                             PVAL_EXCLUSIVE=np.nan if shared else hypergeom.cdf(both, n, nb_, na),
                             TENDENCY="overlap" if shared else "co-occurrence" if odds > 0 else "exclusivity"))
    want = pd.DataFrame(rows, columns=["ELT_A", "ELT_B", "N_SAMPLES", "N_A", "N_B", "N_BOTH", "N_A_ONLY", "N_B_ONLY", "N_NEITHER", "LOG2_ODDS",
                                       "PVAL_COOCCUR", "PVAL_EXCLUSIVE", "TENDENCY"]).set_index("ELT_A")
    return want, enter, hit, n


def _check_frame(g, want, what):
    """A frame with every pair in it against the statement; its q-values against get_q_vals over its own testable p-values."""
    from digdriver_amd.driver_model import cohort_batch
    from digdriver_amd.sequence_model import nb_model
    assert list(g.columns) == cohort_batch.PAIR_COLUMNS and g.index.name == "ELT_A", what
    assert list(g.index) == list(want.index) and list(g.ELT_B) == list(want.ELT_B) and list(g.TENDENCY) == list(want.TENDENCY), what
    for col in ("N_SAMPLES", "N_A", "N_B", "N_BOTH", "N_A_ONLY", "N_B_ONLY", "N_NEITHER"):
        assert g[col].dtype == np.int64 and np.array_equal(g[col].values, want[col].values), (what, col)
    assert np.allclose(g.LOG2_ODDS.values, want.LOG2_ODDS.values, rtol=1e-14, atol=0), what
    for col in ("PVAL_COOCCUR", "PVAL_EXCLUSIVE"):
        got, ref = g[col].values, want[col].values
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, col)
        ok = ~np.isnan(ref)
        rel = np.abs(got[ok] - ref[ok]) / ref[ok]
        print("%s, %s: worst relative error %.3g over %d pairs" % (what, col, rel.max() if rel.size else 0.0, ok.sum()))
        assert (ref[ok] >= 1e-250).all() and (rel <= 1e-6).all(), (what, col)
        q = np.full(len(got), np.nan)
        q[ok] = nb_model.get_q_vals(got[ok])
        assert g["QVAL" + col[4:]].values.tobytes() == q.tobytes(), (what, col)


def _exact(a, b):
    """The same frames: index, columns, dtypes and the bits of every number (the text columns by their values)."""
    pd.testing.assert_frame_equal(a, b, check_exact=True)
    for col in a.columns:
        if a[col].dtype != object:
            assert a[col].values.tobytes() == b[col].values.tobytes(), col


def _runs(case, **kw):
    from digdriver_amd.driver_model import cohort_batch
    args = (case["muts"], case["pres"], case["ed"], "elts")
    hits = cohort_batch.run_element_calls(*args, **CUT, **case["kw"])
    return hits, cohort_batch.run_element_pairs(*args, **CUT, **case["kw"], **kw)


def test_every_pair_against_the_statement_from_the_mutation_files(case):
    hits, frames = _runs(case, pair_pval_max=1.0)
    assert len(frames) == 3 and len(hits[2]) == 0 and len(frames[2]) == 0
    assert frames[2].attrs == dict(n_elements=0, n_pairs=0, n_testable=0) and list(frames[2].columns) == list(frames[0].columns)
    for c in (0, 1):
        called = list(hits[c].index)
        assert set(SAME + APART + SHARED) <= set(called) and len(called) >= 14, called
        want, enter, hit, n = _statement(case, c, called)
        assert n == N_SAMPLES[c] and "HYPER" not in set().union(*hit.values())             # (the blacklisted sample is in no row, and not counted)
        _check_frame(frames[c], want, "cohort %d" % c)
        H = len(enter)
        assert frames[c].attrs == dict(n_elements=H, n_pairs=H * (H - 1) // 2, n_testable=H * (H - 1) // 2 - 1)
        # popcount(row) == OBS_SAMPLES of the hits frame
        n_of = dict(zip(frames[c].index, frames[c].N_A))
        n_of.update(zip(frames[c].ELT_B, frames[c].N_B))
        assert all(n_of[e] == int(hits[c].OBS_SAMPLES.loc[e]) == len(hit[e]) for e in called)
        pair = lambda a, b: frames[c][(frames[c].index == a) & (frames[c].ELT_B == b)].iloc[0]
        same, apart, shared = pair(*SAME), pair(*APART), pair(*SHARED)
        assert same.TENDENCY == "co-occurrence" and same.N_BOTH >= 12 and same.QVAL_COOCCUR < 1e-3 and same.PVAL_EXCLUSIVE > 0.99
        assert apart.TENDENCY == "exclusivity" and apart.N_BOTH <= 1 and apart.PVAL_EXCLUSIVE < (1e-2 if c == 0 else 0.2)
        assert shared.TENDENCY == "overlap" and shared.N_BOTH >= 10 and np.isnan(shared[["PVAL_COOCCUR", "PVAL_EXCLUSIVE", "QVAL_COOCCUR",
                                                                                         "QVAL_EXCLUSIVE"]].values.astype(float)).all()
        assert (frames[c].TENDENCY == "overlap").sum() == 1


def test_the_reported_pairs_are_the_full_frames_rows_that_pass(case):
    _, full = _runs(case, pair_pval_max=1.0)
    for kw, passes in ((dict(pair_fdr=0.1), lambda f: (f.QVAL_COOCCUR <= 0.1) | (f.QVAL_EXCLUSIVE <= 0.1)),
                       (dict(pair_pval_max=0.01), lambda f: (f.PVAL_COOCCUR <= 0.01) | (f.PVAL_EXCLUSIVE <= 0.01))):
        _, frames = _runs(case, **kw)
        for f, g in zip(full, frames):
            _exact(g, f[passes(f) | (f.TENDENCY == "overlap")])
            assert g.attrs == f.attrs
        assert 0 < len(frames[0]) < len(full[0]) and SAME[1] in set(frames[0].ELT_B) and "overlap" in set(frames[0].TENDENCY)


def test_a_larger_universe_and_a_minimum_of_samples(case):
    from digdriver_amd.driver_model import cohort_batch
    hits, frames = _runs(case, pair_pval_max=1.0, n_samples=[64, 129, 500], min_samples=10)
    for c in (0, 1):
        want, enter, hit, n = _statement(case, c, list(hits[c].index), n=[64, 129, 500][c], min_samples=10)
        assert 2 < len(enter) < len(hits[c]) and (frames[c].N_SAMPLES == n).all()
        _check_frame(frames[c], want, "cohort %d, n_samples %d, min_samples 10" % (c, n))
    with pytest.raises(ValueError, match=r"n_samples: below the samples of the mutation file that were not blacklisted \(\[40, 90, 130\]\) in cohorts \[1\]"):
        _runs(case, pair_fdr=0.1, n_samples=[40, 89, 130])
    ep = cohort_batch.element_pass(case["muts"], case["pres"], case["ed"], "elts", **case["kw"])
    with pytest.raises(ValueError, match="made without keep_sample_keys=True"):
        cohort_batch.run_element_pairs(case["muts"], case["pres"], case["ed"], "elts", **CUT, pair_fdr=0.1, element_pass=ep)


def test_one_pass_shared_with_the_calls_gives_the_same_bits_and_leaves_them_theirs(case):
    from digdriver_amd.driver_model import cohort_batch
    args = (case["muts"], case["pres"], case["ed"], "elts")
    hits, fresh = _runs(case, pair_fdr=0.1)
    ep = cohort_batch.element_pass(*args, **case["kw"], keep_sample_keys=True)
    assert set(ep[0].sample_keys) == {"keys", "n_samples"} and ep[0].sample_keys["n_samples"].tolist() == list(N_SAMPLES)
    shared_hits = cohort_batch.run_element_calls(*args, **CUT, element_pass=ep)
    shared = cohort_batch.run_element_pairs(*args, **CUT, pair_fdr=0.1, element_pass=ep)
    for a, b in zip(hits + fresh, shared_hits + shared):
        _exact(a, b)


def test_the_written_files_read_back_and_the_commands_other_files_keep_their_bytes(case):
    from digdriver_amd.driver_model import cohort_batch
    cli = _cli()
    out_a, out_b, out_c = (str(case["tmp"] / d) for d in ("cli_plain", "cli_pairs", "written"))
    lists = "--mutation-files %s --maps %s --outpfx A B C --max-muts-per-sample %d" % (" ".join(case["muts"]), " ".join(case["pres"]), MAX_MUTS)
    cli.main("elementCohorts %s elts %s --outdir %s --fdr 0.1" % (case["ed"], lists, out_a))
    cli.main("elementCohorts %s elts %s --outdir %s --fdr 0.1 --pairs --pairs-fdr 0.1" % (case["ed"], lists, out_b))
    assert sorted(os.listdir(out_a)) == ["A.hits.txt", "B.hits.txt", "C.hits.txt"]
    assert sorted(os.listdir(out_b)) == sorted(["A.hits.txt", "B.hits.txt", "C.hits.txt", "A.pairs.txt", "B.pairs.txt", "C.pairs.txt"])
    for pfx in "ABC":
        assert open(os.path.join(out_a, pfx + ".hits.txt"), "rb").read() == open(os.path.join(out_b, pfx + ".hits.txt"), "rb").read()
    frames, paths = cohort_batch.run_and_write_element_pairs(case["muts"], case["pres"], case["ed"], "elts", out_c, ["A", "B", "C"], fdr=0.1,
                                                             pair_fdr=0.1, **case["kw"])
    assert len(frames[0]) > 0
    for pfx, f, path in zip("ABC", frames, paths):
        assert path == os.path.join(out_c, pfx + ".pairs.txt")
        assert open(path, "rb").read() == open(os.path.join(out_b, pfx + ".pairs.txt"), "rb").read()
        back = pd.read_csv(path, sep="\t", index_col=0, float_precision="round_trip")
        assert list(back.columns) == list(f.columns) and list(back.index) == list(f.index) and back.index.name == "ELT_A"
        for col in f.columns:
            if f[col].dtype == object:
                assert list(back[col]) == list(f[col]), (pfx, col)
            else:
                assert back[col].dtype == f[col].dtype or len(f) == 0, (pfx, col)       # (the counts are integers in the file)
                assert np.array_equal(back[col].values.astype(float), f[col].values.astype(float), equal_nan=True), (pfx, col)
