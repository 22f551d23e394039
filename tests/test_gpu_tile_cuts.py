"""The tile-probability entry points on one small problem at every cohort count where their host dispatch or their shared
device helpers take another path: all nine (tiles, quads) cuts of a 48-cohort chunk, both sides of the one-role / two-role
choice and two chunks for the trinucleotide kernels; walker widths 2, 4 and 8, partial last passes and one to three launches
for the row walk, and its deferred regions (general kernel).  The oracle is a float64 numpy evaluation of the definition,
written here: pt = (tile sum of S[c][context]) / (region sum), 0 for a window that holds a non-ACGT base.  Tolerances: those
of tests/test_gpu_tiles.py (1e-12 relative for trinucleotide and penta-nucleotide tables alike)."""
import numpy as np
import pytest

BINSIZE, N_TILES = 7, 20                                # two groups of sixteen tiles, the second ragged
TRI_C = [1, 4, 5, 8, 9, 16, 17, 21, 24, 25, 32, 33, 37, 40, 41, 48, 49, 85]
PENTA_C = [1, 2, 3, 4, 5, 8, 9, 16, 17, 37]
EMPTY = 5                                               # index of the empty region


def _problem():
    rng = np.random.default_rng(31)
    chr1 = rng.choice(list("ACGT"), 2003)
    chr1[600:640] = "N"
    seqs = {"chr1": "".join(chr1), "chr2": "".join(rng.choice(list("ACGT"), 1501))}
    regions = [("chr1", 0, 130),                        # START == 0: the first position is n_up
               ("chr2", 1400, 1600),                    # cut by the chromosome end
               ("chr1", 550, 690),                      # spans the N run; 140 positions = twenty whole tiles
               ("chr1", 1000, 1100),                    # 100 positions: fourteen tiles and two positions
               ("chr1", 1200, 1500),                    # 300 positions: those behind the last tile count for the total only
               ("chr2", 500, 500)]                      # empty
    S3 = rng.uniform(1e-4, 1e-2, (max(TRI_C), 64))
    S5 = rng.uniform(1e-4, 1e-2, (max(PENTA_C), 1024))
    return seqs, regions, S3, S5


def _oracle(seqs, regions, S, n_up, binsize, n_tiles):
    """(pt [C, R, n_tiles], first_pos [R], n_valid [R], region totals [C, R]) in float64, from the definition."""
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    C, R = S.shape[0], len(regions)
    pt = np.full((C, R, n_tiles), np.nan)
    first, nval, totals = np.zeros(R, np.int64), np.zeros(R, np.int32), np.zeros((C, R))
    for r, (chrom, start, end) in enumerate(regions):
        seq = seqs[chrom]
        first[r] = n_up if start == 0 else start
        stop = min(end, len(seq) - n_up)
        n_pos = max(stop - first[r], 0)
        probs = np.zeros((C, n_pos))
        for j in range(n_pos):
            window = seq[first[r] + j - n_up:first[r] + j + n_up + 1]
            if all(b in code for b in window):
                ctx = 0
                for b in window:                        # the leftmost base counts highest (itertools.product('ACGT', ...) order)
                    ctx = 4 * ctx + code[b]
                probs[:, j] = S[:, ctx]
        totals[:, r] = probs.sum(axis=1)
        nval[r] = min(-(-n_pos // binsize), n_tiles)
        for t in range(nval[r]):
            with np.errstate(invalid="ignore"):
                pt[:, r, t] = probs[:, t * binsize:(t + 1) * binsize].sum(axis=1) / totals[:, r]
    return pt, first, nval, totals


def test_problem_and_oracle_before_the_gpu():
    """Only the empty region has a zero total; the oracle gives it n_valid = 0 and NaN tiles; the shapes are what the docstring says."""
    seqs, regions, S3, S5 = _problem()
    for S, n_up in ((S3[:3], 1), (S5[:3], 2)):
        for binsize, n_tiles in ((BINSIZE, N_TILES), (1, 300)):
            pt, first, nval, totals = _oracle(seqs, regions, S, n_up, binsize, n_tiles)
            assert (totals[:, EMPTY] == 0).all() and (np.delete(totals, EMPTY, axis=1) > 0).all()
            assert nval[EMPTY] == 0 and np.isnan(pt[:, EMPTY]).all() and first[EMPTY] == 500
            assert first[0] == n_up
            if binsize == BINSIZE:
                assert nval.tolist() == [19, 15, 20, 15, 20, 0]
                assert (pt[:, 2, :nval[2]] == 0).any() and np.isfinite(pt[:, 2, :nval[2]]).all()      # whole tiles inside the N run
                assert np.nansum(pt[0, 4]) < 0.6                                                        # positions behind the last tile
                assert abs(np.nansum(pt[0, 3]) - 1) < 1e-12


@pytest.fixture(scope="module")
def tiles():
    """The problem on the device, its oracles (computed once) and the call."""
    from digdriver_amd import _lib, engine
    from digdriver_amd.data_tools.genome import PackedGenome
    _lib.require_device()
    seqs, regions, S3, S5 = _problem()
    genome = PackedGenome.from_sequences(seqs)
    chroms = [r[0] for r in regions]
    starts, ends = np.array([r[1] for r in regions], np.int64), np.array([r[2] for r in regions], np.int64)

    def run(S, binsize=BINSIZE, n_tiles=N_TILES):
        pt, first, nval = engine.base_tile_probs(genome, chroms, starts, ends, S, binsize, n_tiles=n_tiles, device=0)
        return pt.cpu().numpy(), first.cpu().numpy(), nval.cpu().numpy()

    want3 = _oracle(seqs, regions, S3, 1, BINSIZE, N_TILES)
    want5 = _oracle(seqs, regions, S5, 2, BINSIZE, N_TILES)
    want5_1 = _oracle(seqs, regions, S5[:5], 2, 1, 300)
    single = [run(S3[c:c + 1])[0][0] for c in range(S3.shape[0])]       # every cohort alone (one quad of the one-role kernel)
    return dict(run=run, S3=S3, S5=S5, want3=want3, want5=want5, want5_1=want5_1, single=single)


def _check(got, want, C):
    pt, first, nval = got
    wpt, wfirst, wnval, _ = want
    assert np.array_equal(first, wfirst) and np.array_equal(nval, wnval)
    assert pt.shape == wpt[:C].shape
    assert np.array_equal(np.isnan(pt), np.isnan(wpt[:C]))
    np.testing.assert_allclose(pt, wpt[:C], rtol=1e-12, atol=0, equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("C", TRI_C)
def test_trinucleotide_tiles_at_every_cut(tiles, C):
    got = tiles["run"](tiles["S3"][:C])
    _check(got, tiles["want3"], C)
    # a cohort's values do not depend on the other cohorts of the call (dig_tiles.hip: the quads sum as the tiles do)
    for c in range(C):
        assert got[0][c].tobytes() == tiles["single"][c].tobytes(), c


@pytest.mark.gpu
@pytest.mark.parametrize("C", PENTA_C)
def test_penta_tiles_at_every_walker_width(tiles, C):
    _check(tiles["run"](tiles["S5"][:C]), tiles["want5"], C)


@pytest.mark.gpu
def test_penta_tiles_of_one_position_take_the_deferred_path(tiles):
    """binsize 1: the 296 tiles of the long region are more than the row walk keeps sums for -- it leaves that region to the
    general kernel -- and the other regions stay with the row walk."""
    _check(tiles["run"](tiles["S5"][:5], binsize=1, n_tiles=300), tiles["want5_1"], 5)
