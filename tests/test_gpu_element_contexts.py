"""engine.element_context_counts (dig_element_context_counts, csrc/dig_eltcontext.hip) against its plain statement
(tests/element_contexts_statement.py) and against the sum of engine.count_contexts rows per block, bit for bit: every edge of the
definition in include/dig_hip.h on a three-chromosome genome, the host twin against the device entry point, both capped grids
past their caps and one call inside a guarded arena (tests/guarded_arena.py)."""
import functools

import numpy as np
import pytest

import guarded_arena as GA
from element_contexts_statement import block_counts, element_counts
from guarded_arena import guarded_runs

pytestmark = pytest.mark.gpu

LENGTHS = {"chr1": 4100, "chr2": 37, "chr3": 70000}
# runs of N (start, end): at a chromosome's first base, across a 16-base word of the packed array (chromosomes start on a word
# boundary), two runs one base apart, a run longer than a word, at a chromosome's last bases
N_RUNS = {"chr1": [(0, 5), (1018, 1035), (2000, 2001), (2002, 2003), (4090, 4100)], "chr2": [(0, 1), (35, 37)],
          "chr3": [(0, 3), (15, 17), (20000, 20500), (33333, 33334), (47995, 48010), (69998, 70000)]}


@functools.lru_cache(maxsize=None)
def sequences():
    rng = np.random.default_rng(101)
    seqs = {}
    for name, n in LENGTHS.items():
        s = rng.choice(np.frombuffer(b"acgt", np.uint8), n).copy()
        s[rng.uniform(size=n) < 0.3] -= 32                                # upper and lower case
        for a, b in N_RUNS[name]:
            s[a:b] = ord("N") if a % 2 else ord("n")
        seqs[name] = s.tobytes().decode()
    return seqs


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    from digdriver_amd import _lib
    from digdriver_amd.data_tools.genome import PackedGenome
    _lib.require_device()
    fa = tmp_path_factory.mktemp("eltctx") / "genome.fa"
    with open(fa, "w") as f:
        for name, s in sequences().items():
            f.write(">%s\n" % name)
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60] + "\n")
    return PackedGenome.from_fasta(str(fa))


@functools.lru_cache(maxsize=None)
def stated_block(chrom, start, end, minus):
    return block_counts(sequences()[chrom], start, end, minus)


def stated(elts):
    """int64 [E, 64] of (chrom, minus, blocks) elements; a block is stated once however often it is listed."""
    out = np.zeros((len(elts), 64), np.int64)
    for e, (chrom, minus, blocks) in enumerate(elts):
        for s, t in blocks:
            out[e] += stated_block(chrom, int(s), int(t), bool(minus))
    return out


def tables(elts):
    chrom = [c for c, _, _ in elts]
    minus = np.array([m for _, m, _ in elts], np.uint8)
    ptr = np.concatenate([[0], np.cumsum([len(b) for _, _, b in elts])]).astype(np.int64)
    start = np.array([s for _, _, b in elts for s, _ in b], np.int64)
    end = np.array([t for _, _, b in elts for _, t in b], np.int64)
    return chrom, minus, ptr, start, end


@functools.lru_cache(maxsize=None)
def edge_elements():
    rng = np.random.default_rng(7)
    many = [(int(s), int(s) + int(z)) for s, z in zip(rng.integers(0, 69000, 70), rng.integers(1, 900, 70))]
    elts = [
        ("chr1", 0, [(100, 900)]),                                        # one block
        ("chr3", 1, many),                                                # 70 blocks: more than a wave's lanes, several tiles
        ("chr1", 0, [(500, 501)]),                                        # one base
        ("chr1", 1, [(0, 50)]),                                           # START == 0
        ("chr2", 0, [(5, 37)]),                                           # ends at chrom_len
        ("chr2", 1, [(5, 60)]),                                           # ends past chrom_len
        ("chr2", 0, [(0, 37)]),                                           # a whole chromosome of 37 bases
        ("chr3", 0, [(20100, 20400)]),                                    # inside a run of N
        ("chr3", 1, [(19990, 20010), (20495, 20505)]),                    # over a run's edges
        ("chr1", 0, [(1010, 1040), (1990, 2010)]),                        # the run over a word boundary; two runs one base apart
        ("chr1", 1, [(300, 700), (300, 700)]),                            # a repeated block
        ("chr1", 0, []),                                                  # no block
        ("chr1", 1, [(300, 200), (200, 200), (150, 160)]),                # inverted, empty, then one that counts
        ("chr3", 0, [(5000, 65000)]),                                     # 60 000 bases: cut across waves
        ("chr3", 1, [(5000, 65000), (10, 40), (69000, 70000)]),           # the same on the other strand, with short blocks
        ("chr3", 1, [(0, 70000)]),                                        # a whole chromosome, runs at both ends
        ("chr1", 0, [(4000, 4100)]),                                      # the chromosome's last bases, all N at the end
        ("chr1", 0, [(0, 4100), (0, 4100)]),
    ]
    for _ in range(30):
        c = ["chr1", "chr3"][int(rng.integers(0, 2))]
        n = LENGTHS[c]
        blocks = [(int(s), int(s) + int(z)) for s, z in zip(rng.integers(0, n - 10, int(rng.integers(1, 5))), rng.integers(1, 3100, 4))]
        elts.append((c, int(rng.integers(0, 2)), blocks))
    return tuple(elts)


def counts_by_rows(genome, elts):
    """The parent's path: one engine.count_contexts row per block, summed per element on the host."""
    from digdriver_amd import engine
    chrom, minus, ptr, start, end = tables(elts)
    owner = np.repeat(np.arange(len(elts)), np.diff(ptr))
    rows = engine.count_contexts(genome, [chrom[e] for e in owner], start, end, minus[owner]).cpu().numpy().astype(np.int64)
    out = np.zeros((len(elts), 64), np.int64)
    np.add.at(out, owner, rows)
    return out


def test_statement_agrees_with_the_plain_loop_of_the_helper():
    """The cached per-block form used below is element_counts of the statement module."""
    elts = edge_elements()[:13]
    chrom, minus, ptr, start, end = tables(elts)
    assert np.array_equal(stated(elts), element_counts(sequences(), chrom, minus, ptr, start, end))


def test_edges_against_statement_and_block_rows(genome):
    import torch
    from digdriver_amd import engine
    elts = edge_elements()
    chrom, minus, ptr, start, end = tables(elts)
    want = stated(elts)
    assert np.array_equal(counts_by_rows(genome, elts), want)            # the two references agree
    assert want[11].sum() == 0 and want[7].sum() == 0 and want[12].sum() > 0 and (want[10] == 2 * stated([elts[10][:2] + ([(300, 700)],)])[0]).all()
    assert want[13].sum() > 59000 and not np.array_equal(want[13], want[14])
    host = engine.element_context_counts(genome, chrom, minus, ptr, start, end)
    assert isinstance(host, np.ndarray) and host.dtype == np.int32 and host.shape == (len(elts), 64)
    assert np.array_equal(host.astype(np.int64), want)
    dev = engine.element_context_counts(genome, chrom, minus, ptr, start, end, on_device=True)
    assert dev.is_cuda and dev.dtype == torch.int32
    assert np.array_equal(dev.cpu().numpy(), host)                       # the host twin and the device entry point: the same bits
    # device tensors in (the genome's chromosome indices), a tensor out
    d = lambda a: torch.as_tensor(a, device="cuda:0")
    dev2 = engine.element_context_counts(genome, d(genome.chrom_index(chrom)), d(minus), d(ptr), d(start), d(end))
    assert dev2.is_cuda and np.array_equal(dev2.cpu().numpy(), host)


def test_no_element(genome):
    from digdriver_amd import engine
    z = np.zeros(0, np.int64)
    for on_device in (False, True):
        out = engine.element_context_counts(genome, [], np.zeros(0, np.uint8), np.zeros(1, np.int64), z, z, on_device=on_device)
        assert tuple(out.shape) == (0, 64)
    out = engine.element_context_counts(genome, ["chr2", "chr1"], [0, 1], [0, 0, 0], z, z)       # elements, no block at all
    assert out.shape == (2, 64) and not out.any()


def test_first_grid_past_its_cap(genome):
    """elt_context_kernel: grid_for(tiles * 64, 256, 8) workgroups of four waves, a tile of 16 blocks per wave and pass.  Two full
    passes and a ragged third of one-block elements of 8 bases, drawn by index from 97 stated cases."""
    import torch
    from digdriver_amd import engine
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    cap = cus * 8 * 4 * 16
    E = 2 * cap + cap // 8 + 37
    rng = np.random.default_rng(3)
    cases = [("chr1", int(s), int(m)) for s, m in zip(rng.integers(0, 4095, 60), rng.integers(0, 2, 60))] + \
            [("chr3", int(s), int(m)) for s, m in zip(rng.integers(0, 69995, 35), rng.integers(0, 2, 35))] + [("chr2", 30, 0), ("chr1", 1020, 1)]
    ref = np.stack([stated_block(c, s, s + 8, bool(m)) for c, s, m in cases])
    pick = rng.integers(0, len(cases), E)
    ci = genome.chrom_index([c for c, _, _ in cases])[pick]
    start = np.array([s for _, s, _ in cases], np.int64)[pick]
    minus = np.array([m for _, _, m in cases], np.uint8)[pick]
    d = lambda a: torch.as_tensor(a, device="cuda:0")
    got = engine.element_context_counts(genome, d(ci), d(minus), d(np.arange(E + 1, dtype=np.int64)), d(start), d(start + 8))
    assert np.array_equal(got.cpu().numpy().astype(np.int64), ref[pick])
    assert ref.sum(axis=1).min() >= 0 and (ref.sum(axis=1) == 8).any()


def test_second_grid_past_its_cap(genome):
    """elt_context_long_kernel: at most 64 listed blocks in flight (grid.y).  70 elements hold a block that is cut across waves."""
    from digdriver_amd import engine
    elts = [("chr3", e % 2, [(100 + e, 40000 + 3 * e)] + ([(5, 25)] if e % 3 == 0 else [])) for e in range(70)]
    chrom, minus, ptr, start, end = tables(elts)
    got = engine.element_context_counts(genome, chrom, minus, ptr, start, end, on_device=True)
    assert np.array_equal(got.cpu().numpy().astype(np.int64), counts_by_rows(genome, elts))
    assert np.array_equal(got[:4].cpu().numpy().astype(np.int64), stated(elts[:4]))


def test_guarded_call(genome):
    """One call with every argument carved from a guarded arena at exactly its documented size and alignment (words2 16, the
    workspace 8 bytes and exactly dig_element_context_counts_workspace(n_blocks) long, everything else its element size): no
    band touched, the same bits under both poisons and on ordinary tensors, and the statement's counts."""
    import torch
    from digdriver_amd import _lib
    elts = edge_elements()
    chrom, minus, ptr, start, end = tables(elts)
    E, nb = len(elts), len(start)
    w2, ns, ne, bk = genome.two_bit()
    total = int(((genome.lengths + 7) // 8 * 8).sum())
    arr = lambda dt, a, **kw: GA.inp(dt, np.ascontiguousarray(a, GA._NP[dt]), **kw)
    n_ws = int(_lib.load().dig_element_context_counts_workspace(nb))
    assert n_ws == 16 + 8 * nb
    lo = int(genome.lengths.min())
    bufs = dict(words2=arr("u32", w2, align=16), nint_start=arr("i64", ns, index=(0, 64 + total)), nint_end=arr("i64", ne, index=(0, 64 + total)),
                nint_bucket=arr("i32", bk, index=(0, len(ns))), chrom_off=arr("i64", genome.offsets, index=(0, int(genome.offsets.max()))),
                chrom_len=arr("i64", genome.lengths, index=(lo, int(genome.lengths.max()))),
                elt_chrom=arr("i32", genome.chrom_index(chrom), index=(0, len(genome.names) - 1)), elt_minus=arr("u8", minus),
                blk_ptr=arr("i64", ptr, index=(0, nb)), blk_start=arr("i64", start, index=(0, lo)), blk_end=arr("i64", end, index=(0, lo)),
                out=GA.out("i32", (E, 64)), ws=GA.ws(n_ws, align=8))

    def invoke(a):
        _lib.call("dig_element_context_counts", a.ptr("words2"), len(w2), a.ptr("nint_start"), a.ptr("nint_end"), len(ns), a.ptr("nint_bucket"),
                  len(bk), a.ptr("chrom_off"), a.ptr("chrom_len"), len(genome.names), a.ptr("elt_chrom"), a.ptr("elt_minus"), a.ptr("blk_ptr"),
                  a.ptr("blk_start"), a.ptr("blk_end"), E, nb, a.ptr("out"), a.ptr("ws"), n_ws, _lib.stream_ptr())

    got = guarded_runs(bufs, invoke, device=torch.device("cuda:0"), what="dig_element_context_counts", plain=True)
    assert np.array_equal(got["out"].astype(np.int64), stated(elts))
