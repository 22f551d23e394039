"""GPU test of engine.overlap_join, the one interval join (dig_overlap_join_count, a cumulative sum, dig_overlap_join_fill) behind
tabulate_gpu.overlap_pairs, engine.window_objectives and mutation_tools._gene_range_join: device tensors and host arrays against
oracle.interval_join_pairs on a block table with nested, back-to-back, zero-length and unsorted blocks.  Integer pairs: exact."""
import numpy as np
import pytest

import overlap_join_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case():
    from digdriver_amd import engine
    from oracle import dig_oracle as O
    blocks, muts = K.block_table(), K.mutation_rows()
    order, start_key, runmax_key, end_eff = engine.join_blocks(*blocks)
    mi, bi = O.interval_join_pairs(*muts, *blocks)
    return dict(blocks=blocks, muts=muts, order=order, table=(start_key, runmax_key, end_eff), want=sorted(zip(mi.tolist(), bi.tolist())))


def _join(case, on_device, **kw):
    from digdriver_amd import engine
    from digdriver_amd._marshal import backend_on
    pm, pb = engine.overlap_join(backend_on(0, on_device), *case["table"], *case["muts"], **kw)
    if on_device:
        assert pm.is_cuda and pb.is_cuda
        pm, pb = pm.cpu().numpy(), pb.cpu().numpy()
    assert pm.dtype == np.int32 and pb.dtype == np.int32 and pm.shape == pb.shape
    return pm, pb


def test_both_backends_give_the_oracles_pairs(case):
    dev, host = _join(case, True), _join(case, False)
    assert np.array_equal(dev[0], host[0]) and np.array_equal(dev[1], host[1])
    pm, pb = dev
    assert len(case["want"]) > 200 and sorted(zip(pm.tolist(), case["order"][pb].tolist())) == case["want"]
    # mutation-major, the blocks of the sorted table ascending within a mutation
    step = np.diff(pm.astype(np.int64)) * len(case["order"]) + np.diff(pb.astype(np.int64))
    assert (np.diff(pm) >= 0).all() and (step > 0).all()
    assert (pm == K.SPANS_THREE).sum() == 3 and (pm == 0).sum() == 0 and (pm == 7).sum() == 0 and (pm == 8).sum() == 0


@pytest.mark.parametrize("on_device", [True, False], ids=["device", "host"])
def test_empty_sides_and_max_pairs(case, on_device):
    from digdriver_amd import engine
    from digdriver_amd._marshal import backend_on
    be = backend_on(0, on_device)
    none = np.zeros(0, np.int64)
    for pm, pb in (engine.overlap_join(be, none, none, none, *case["muts"]), engine.overlap_join(be, *case["table"], none, none, none)):
        assert pm.shape == (0,) and pb.shape == (0,)
    with pytest.raises(ValueError):
        _join(case, on_device, max_pairs=1)
    with pytest.raises(ValueError, match="^%d pairs: the caller's own words$" % len(case["want"])):
        _join(case, on_device, max_pairs=len(case["want"]) - 1, too_many="%d pairs: the caller's own words")
    assert len(_join(case, on_device, max_pairs=len(case["want"]))[0]) == len(case["want"])


def test_the_three_callers_give_the_same_pairs(case):
    import torch
    from digdriver_amd.data_tools import mutation_tools, tabulate_gpu
    pm, pb = _join(case, True)
    chrom, start, end = case["blocks"]
    dev = torch.device("cuda:0")
    eb = tabulate_gpu.ElementBlocks(chrom, start, end, np.arange(len(chrom)), len(chrom), dev)
    tm, tb = tabulate_gpu.overlap_pairs(eb, *[torch.as_tensor(x, device=dev) for x in case["muts"]])
    assert tm.dtype == torch.int32 and np.array_equal(tm.cpu().numpy(), pm) and np.array_equal(tb.cpu().numpy(), pb)
    assert np.array_equal(eb.elt.cpu().numpy(), case["order"])
    # the gene ranges: 1-based closed, chromosome labels, sorted already
    o = case["order"]
    label = lambda c: np.array(["chr%d" % x for x in c], dtype=object)
    mc, ms, me = case["muts"]
    for on_device in (True, False):
        gm, gb = mutation_tools._gene_range_join(label(chrom[o]), start[o] + 1, np.maximum(end[o], start[o] + 1), label(mc), ms + 1,
                                                 np.maximum(me, ms + 1), on_device)
        assert gm.dtype == np.int64 and gb.dtype == np.int64 and np.array_equal(gm, pm) and np.array_equal(gb, pb), on_device
