"""quickDriver for many cohorts, what needs no GPU: the statement of the element context counts on a case whose counts can be read
off, the new entry points' binding and refusals (every one before any device work), the quickCohorts parser and the strict-reference
refusal of a block shared by elements of opposite strands."""
import os
import sys

import numpy as np
import pytest

import quick_cohort_cases as K
from conftest import ROOT
from digdriver_amd import _lib, engine
from digdriver_amd.data_tools.genome import PackedGenome
from digdriver_amd.driver_model import cohort_batch
from element_contexts_statement import block_counts, element_counts

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import DigDriver  # noqa: E402

CTX = ["".join(t) for t in __import__("itertools").product("ACGT", repeat=3)]


def _counts(vec):
    return {CTX[i]: int(n) for i, n in enumerate(vec) if n}


def test_statement_on_a_case_that_can_be_read_off():
    """nonc_elt_context_count's rule (sequence_tools.py:527-566 over :21-29,42-80) on twelve bases:
           0 1 2 3 4 5 6 7 8 9 10 11
           A C G T N A C G T A C  G
    the fetch of (0, 12) is bases 0 .. 11 (START 0 -> 1, truncated at the end): centres 1 .. 10 = ACG CGT GTN TNA NAC ACG CGT GTA TAC
    ACG, the three with the N skipped; the '-' strand reads the reverse complement CGTACGTNACGT: the same triplets reverse-
    complemented (ACG <-> CGT, GTA <-> TAC)."""
    seq = "acgtNACGTACG"
    assert _counts(block_counts(seq, 0, 12, False)) == {"ACG": 3, "CGT": 2, "GTA": 1, "TAC": 1}
    assert _counts(block_counts(seq, 0, 12, True)) == {"CGT": 3, "ACG": 2, "TAC": 1, "GTA": 1}
    assert _counts(block_counts(seq, 1, 11, False)) == _counts(block_counts(seq, 0, 40, False))      # START 0 -> 1; END past the end
    assert _counts(block_counts(seq, 2, 8, False)) == {"CGT": 2, "ACG": 1}                           # centres 2 .. 7
    assert _counts(block_counts(seq, 3, 6, False)) == {} and _counts(block_counts(seq, 8, 8, False)) == {} and \
        _counts(block_counts(seq, 9, 3, True)) == {}                                                 # in the N's reach; empty; inverted
    assert _counts(block_counts(seq, 11, 12, False)) == {}                                           # the last base is no centre
    got = element_counts({"c": seq}, ["c", "c", "c"], [0, 1, 0], [0, 2, 2, 3], [0, 2, 2], [12, 8, 8])
    assert _counts(got[0]) == {"ACG": 4, "CGT": 4, "GTA": 1, "TAC": 1} and not got[1].any() and _counts(got[2]) == {"CGT": 2, "ACG": 1}
    # every substitution column of L holds its context's count (sequence_tools._context_columns)
    from digdriver_amd.sequence_model import sequence_tools
    keys, cols = sequence_tools._context_columns(sequence_tools.mk_trans_idx(n_up=1, n_down=1, collapse=False))
    L = got[0][cols]
    assert len(keys) == 192 and all(L[i] == got[0][CTX.index(k.split(">")[0])] for i, k in enumerate(keys)) and L.sum() == 3 * 10


def test_symbols_are_exported_declared_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dig_hip.h")).read()
    for sym in ("dig_element_context_counts", "dig_element_context_counts_host", "dig_element_context_counts_workspace"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym) and sym + "(" in header
    assert lib.dig_abi_version() == 12 and _lib.ABI_VERSION == 12 and "#define DIG_ABI_VERSION 12" in header
    assert lib.dig_element_context_counts_workspace(0) == 16 and lib.dig_element_context_counts_workspace(1000) == 16 + 8000


GENOME_ARGS = [None, 28, None, None, 0, None, 0, None, None, 0]


def _refused(rc, *words):
    assert rc == -1, rc
    for w in words:
        assert w in _lib.last_error(), _lib.last_error()


def test_library_refusals_come_before_any_device_work():
    """DIG_EINVAL with a message for 2^31 elements or blocks and a misaligned out (both entry points), and in the host twin, which
    can see its arrays, for a blk_ptr that decreases or does not end at the block count and a chromosome id outside the genome.
    (No device is needed to be refused: the checks come first.)"""
    lib = _lib.load()
    big = 1 << 31
    for name, tail in (("dig_element_context_counts", (None, 0, None)), ("dig_element_context_counts_host", (0,))):
        fn = getattr(lib, name)
        _refused(fn(*GENOME_ARGS, None, None, None, None, None, big, 0, None, *tail), name, "< 2^31")
        _refused(fn(*GENOME_ARGS, None, None, None, None, None, 1, big, None, *tail), name, "< 2^31")
        _refused(fn(*GENOME_ARGS, None, None, None, None, None, -1, 0, None, *tail), name, ">= 0")
    g = PackedGenome.from_sequences({"c1": "ACGT" * 20, "c2": "GGCA" * 5})
    head = g.genome2_args(None)
    p = _lib.host_ptr
    chrom, minus = np.zeros(2, np.int32), np.zeros(2, np.uint8)
    ptr, start, end = np.array([0, 1, 2], np.int64), np.array([3, 4], np.int64), np.array([30, 40], np.int64)
    out = np.zeros(2 * 64 + 1, np.int32)
    odd = out.view(np.uint8)[1:1 + 2 * 64 * 4]                             # one byte off
    call = lambda c, q, o, nb=2: lib.dig_element_context_counts_host(*head, p(c), p(minus), p(q), p(start), p(end), 2, nb,
                                                                      o.ctypes.data_as(__import__("ctypes").c_void_p), 0)
    _refused(call(chrom, ptr, odd), "out 4-byte aligned")
    _refused(lib.dig_element_context_counts(*head, p(chrom), p(minus), p(ptr), p(start), p(end), 2, 2,
                                            odd.ctypes.data_as(__import__("ctypes").c_void_p), None, 0, None), "out 4-byte aligned")
    _refused(call(chrom, np.array([0, 3, 2], np.int64), out), "blk_ptr non-decreasing")
    _refused(call(chrom, np.array([0, 1, 1], np.int64), out), "blk_ptr from 0 to n_blocks")
    _refused(call(chrom, np.array([1, 1, 2], np.int64), out), "blk_ptr from 0 to n_blocks")
    _refused(call(np.array([0, 2], np.int32), ptr, out), "chromosome index within [0, n_chrom)")
    _refused(call(np.array([-1, 0], np.int32), ptr, out), "chromosome index within [0, n_chrom)")


def _no_launch(monkeypatch):
    def refuse(name, *args):
        raise AssertionError("library call %s before the refusal" % name)
    monkeypatch.setattr(_lib, "call", refuse)


@pytest.mark.parametrize("bad, match", [
    (dict(blk_ptr=[0, 2, 1]), "without decreasing"), (dict(blk_ptr=[0, 1, 1]), "from 0 to the block count"),
    (dict(blk_ptr=[0, 1]), "disagree"), (dict(elt_chrom=["c1", "c9"]), "c9"), (dict(blk_start=[3, -4]), "negative"),
    (dict(elt_minus=[0]), "disagree"), (dict(blk_end=[30]), "disagree")])
def test_engine_refusals_come_before_any_device_work(monkeypatch, bad, match):
    g = PackedGenome.from_sequences({"c1": "ACGT" * 20, "c2": "GGCA" * 5})
    args = dict(elt_chrom=["c1", "chrc2"], elt_minus=[0, 1], blk_ptr=[0, 1, 2], blk_start=[3, 4], blk_end=[30, 40])
    args.update(bad)
    _no_launch(monkeypatch)
    with pytest.raises(ValueError, match=match):
        engine.element_context_counts(g, **args)


def test_route_refusals_come_before_any_device_work(tmp_path, monkeypatch):
    bed = tmp_path / "e.bed"
    bed.write_text(K.bed12_line("1", 100, "a", "+", [(0, 50)]))
    _no_launch(monkeypatch)
    run = lambda muts, maps, **kw: cohort_batch.run_quick_cohorts(muts, maps, "no.fa", **kw)
    with pytest.raises(ValueError, match="2 mutation files for 1 maps"):
        run(["a", "b"], ["m"], f_elts_bed=str(bed))
    with pytest.raises(ValueError, match="at least one cohort"):
        run([], [], f_elts_bed=str(bed))
    with pytest.raises(ValueError, match="f_elts_bed or region_str"):
        run(["a"], ["m"])
    with pytest.raises(ValueError, match="one value per cohort"):
        run(["a", "b"], ["m", "n"], f_elts_bed=str(bed), scale_by_expectation=False, scale_factors=([1.0, 2.0], [1.0]))
    for scale_type in ("exome", "sample", "MSK_230", "PCAWG_cds"):
        with pytest.raises(NotImplementedError, match=scale_type):
            run(["a"], ["m"], f_elts_bed=str(bed), scale_by_expectation=False, scale_type=scale_type)


def test_strict_reference_refuses_a_block_on_both_strands_and_names_the_pair(tmp_path, monkeypatch):
    lines = [K.bed12_line("2", 100, "plain", "+", [(0, 50)]), K.bed12_line("1", 5000, "fwd", "+", [(0, 400), (900, 300)]),
             K.bed12_line("1", 5000, "same", "+", [(0, 400)]), K.bed12_line("1", 5900, "rev", "-", [(0, 300), (500, 20)]),
             K.bed12_line("1", 5000, "later", "-", [(0, 400)])]
    bed = tmp_path / "pair.bed"
    bed.write_text("".join(lines))
    _no_launch(monkeypatch)
    with pytest.raises(ValueError, match=r"elements fwd and later .* chr1:5000-5400"):
        cohort_batch.run_quick_cohorts(["a"], ["m"], "no.fa", f_elts_bed=str(bed))
    # the same block on ONE strand in two elements is no such pair (the reference's de-duplication then changes nothing)
    bed.write_text("".join(lines[:3]))
    names, chrom, minus, ptr, start, end, n_listed = cohort_batch._quick_elements(str(bed))
    assert n_listed == 3 and list(names) == ["plain", "fwd", "same"] and list(ptr) == [0, 1, 3, 4] and list(minus) == [0, 0, 0]
    assert cohort_batch.opposite_strand_pair(names, chrom, minus, ptr, start, end) is None
    bed.write_text("".join(lines[:4]))
    pair = cohort_batch.opposite_strand_pair(*cohort_batch._quick_elements(str(bed))[:6])
    assert pair == ("fwd", "rev", 1, 5900, 6200)


def test_quick_cohorts_parser():
    a = DigDriver.parse_args("quickCohorts g.fa --mutation-files a.tsv b.tsv --maps a.map b.map --outdir o --outpfx a b --f_elts_bed e.bed")
    assert a.func is DigDriver.cmd_quick_cohorts and a.f_fasta == "g.fa" and a.mutation_files == ["a.tsv", "b.tsv"] and a.maps == ["a.map", "b.map"]
    assert a.outpfx == ["a", "b"] and a.outdir == "o" and a.f_elts_bed == "e.bed" and a.region_str == ""
    assert a.max_muts_per_sample == 3e9 and a.max_muts_per_elt_per_sample == 3e9 and a.scale_type is None and a.panel_dir is None
    assert a.scale_factor_manual is None and a.scale_factor_indel_manual is None and a.skip_pvals is False
    b = DigDriver.parse_args("quickCohorts g.fa --mutation-files a.tsv b.tsv --maps a.map b.map --outdir o --outpfx a b --region_str chr1:5-90 "
                             "--scale-factor-manual 0.5 0.25 --scale-factor-indel-manual 0.1 0.2 --skip_pvals --scale-type genome "
                             "--max-muts-per-sample 40")
    assert b.scale_factor_manual == [0.5, 0.25] and b.scale_factor_indel_manual == [0.1, 0.2] and b.skip_pvals and b.scale_type == "genome"
    assert b.region_str == "chr1:5-90" and b.max_muts_per_sample == 40
    base = "quickCohorts g.fa --mutation-files a.tsv b.tsv --maps a.map b.map --outdir o --f_elts_bed e.bed "
    for text, match in ((base + "--outpfx a", "same number of cohorts"),
                        ("quickCohorts g.fa --mutation-files a.tsv --maps a.map b.map --outdir o --outpfx a b --f_elts_bed e.bed", "same number of cohorts"),
                        (base.replace("--f_elts_bed e.bed ", "") + "--outpfx a b", "--f_elts_bed or --region_str"),
                        (base + "--outpfx a b --scale-factor-manual 0.5 0.25", "must specify both"),
                        (base + "--outpfx a b --scale-factor-indel-manual 0.5 0.25", "must specify both"),
                        (base + "--outpfx a b --scale-factor-manual 0.5 --scale-factor-indel-manual 0.1 0.2", "one value per cohort")):
        args = DigDriver.parse_args(text)
        with pytest.raises(SystemExit, match=match):
            args.func(args)
    # the existing sub-commands keep their parsers
    q = DigDriver.parse_args("quickDriver m.tsv m.map g.fa --outdir o --outpfx p --scale-factor-manual 0.5 --scale-factor-indel-manual 0.1")
    assert q.func is DigDriver.cmd_quick and q.scale_factor_manual == 0.5 and q.scale_factor_indel_manual == 0.1
