"""CPU-only checks: the C-ABI library loads and exports every symbol include/dig_hip.h declares,
host-side index construction matches the reference goldens, and the product path fails loudly
(no CPU fallback) when no GPU is present."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from digdriver_amd import _lib, engine


def _declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "dig_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(dig_[a-z0-9_]+)\s*\(", hdr)))


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    declared = _declared_symbols()
    assert len(declared) >= 20
    for sym in declared:
        assert hasattr(lib, sym), "libdig_hip.so does not export %s" % sym
    assert sorted(_lib.EXPORTED_SYMBOLS) == declared, "python binding table and header disagree"
    assert lib.dig_abi_version() == _lib.ABI_VERSION == 12


def test_library_abi_version_matches_header_and_binding():
    import re
    from digdriver_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dig_hip.h")).read()
    declared = int(re.search(r"#define\s+DIG_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert declared == _lib.ABI_VERSION == _lib.load().dig_abi_version()


def test_two_bit_layout_constants_of_the_packer_match_the_kernels_header():
    """PackedGenome.two_bit writes the layout that csrc/dig_genome2.hpp reads: the pad in front and the bucket size agree."""
    from digdriver_amd.data_tools.genome import PackedGenome
    hpp = open(os.path.join(ROOT, "digdriver_amd", "csrc", "dig_genome2.hpp")).read()
    const = {k: int(v) for k, v in re.findall(r"^constexpr int (kGenome2\w+) = (\d+);", hpp, flags=re.M)}
    assert const["kGenome2PadBases"] == PackedGenome.PAD2_BASES
    assert const["kGenome2BucketShift"] == PackedGenome.BUCKET_SHIFT
    assert const["kGenome2BasesPerWord"] == 16 and const["kGenome2PadWordsBehind"] == 24     # two_bit: 4 + ceil(total / 16) + 24 words


def test_product_never_imports_oracle_or_scipy():
    """The product path must not route through the oracle or any CPU implementation."""
    pkg = os.path.join(ROOT, "digdriver_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if not (f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")) or f == "Makefile"):
                continue
            txt = open(os.path.join(dirpath, f)).read()
            assert "oracle" not in txt, "%s mentions the oracle" % f
            if f.endswith(".py"):
                for line in txt.splitlines():
                    assert not re.match(r"\s*(import|from)\s+scipy", line), "%s imports scipy" % f


def test_ideal_overlaps_host_matches_reference_goldens():
    cases = json.load(open(os.path.join(GOLDEN, "overlaps_golden.json")))
    for c in cases:
        w = c["window"]
        starts, ends = c["intervals"]
        hi = (max(ends) // w + 2)
        bin_start = np.arange(0, hi * w, w, dtype=np.int64)
        bin_chrom = np.full(len(bin_start), c["chrom"], np.int32)
        ptr, idx = engine.ideal_overlaps([c["chrom"]], [0, len(starts)], starts, ends, w, bin_chrom, bin_start)
        got = [int(bin_start[i]) for i in idx]
        assert got == [o[1] for o in c["overlaps"]], c
        assert ptr.tolist() == [0, len(got)]


def test_ideal_overlaps_host_batch_and_missing_bin():
    d = np.load(os.path.join(GOLDEN, "accumulate_golden.npz"))
    bs, be = d["block_starts"], d["block_ends"]
    nblk = (bs >= 0).sum(axis=1)
    blk_ptr = np.concatenate([[0], np.cumsum(nblk)])
    ptr, idx = engine.ideal_overlaps(d["elt_chrom"], blk_ptr, bs[bs >= 0], be[be >= 0], int(d["window"]),
                                     d["bin_idx"][:, 0], d["bin_idx"][:, 1])
    ovp = d["elt_overlap_bins"]
    assert np.array_equal(ptr, np.concatenate([[0], np.cumsum((ovp >= 0).sum(axis=1))]))
    assert np.array_equal(idx, ovp[ovp >= 0])
    # a block beyond the bin table is an error, like the reference's KeyError at df.loc (genic_driver_tools.py:265)
    with pytest.raises(_lib.DigHipError, match="not in the bin table"):
        engine.ideal_overlaps([1], [0, 1], [10 ** 9], [10 ** 9 + 5], int(d["window"]), d["bin_idx"][:, 0], d["bin_idx"][:, 1])
    # empty input
    ptr, idx = engine.ideal_overlaps(np.zeros(0, np.int32), [0], [], [], 10000, d["bin_idx"][:, 0], d["bin_idx"][:, 1])
    assert ptr.tolist() == [0] and len(idx) == 0


def test_no_cpu_fallback_without_gpu():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    from digdriver_amd.sequence_model import nb_model
    with pytest.raises(_lib.DigHipError):
        nb_model.nb_pvalue_greater_midp(np.array([1.0, 2.0]), np.array([2.0, 2.0]), np.array([0.5, 0.5]))
    with pytest.raises(_lib.DigHipError):
        _lib.require_device()


def test_bad_arguments_are_reported_through_dig_last_error():
    lib = _lib.load()
    rc = lib.dig_accumulate_elements_host(None, None, None, None, None, None, None, None, 3, None, None, None, None,
                                          None, None, None, None, None, None, None, 1, 1, 1, 0)
    assert rc == -1
    assert "n_class" in _lib.last_error()


def test_every_host_twin_checks_its_arguments_before_touching_the_device():
    """Each `_host` twin refuses one bad argument (a negative size, a missing pointer, or host data out of range) with
    DIG_EINVAL and its own message, before any HIP call: no device is needed to see it."""
    lib = _lib.load()
    i32 = lambda *v: np.array(v, np.int32)
    i64 = lambda *v: np.array(v, np.int64)
    buf = np.zeros(4096)                                   # any non-null pointer; the checks fail before it is read
    cases = [  # (twin, {argument index: value}, message fragment)
        ("dig_nb_midp_upper_host", {4: -1}, "nb3_host: null pointer or negative n"),
        ("dig_nb_exact_host", {4: -1}, "nb3_host: null pointer or negative n"),
        ("dig_nb_greater_host", {4: -1}, "nb3_host: null pointer or negative n"),
        ("dig_nb_midp_twosided_host", {4: 3}, "nb3_host: null pointer or negative n"),
        ("dig_fisher_host", {3: 3}, "non-null pointers, n >= 0"),
        ("dig_normal_params_to_gamma_host", {4: -1}, "non-null pointers, n >= 0"),
        ("dig_element_stats_host", {13: -1, 14: 2}, "E, C >= 0"),
        ("dig_element_stats_host", {**{i: buf for i in range(13) if i != 6}, 3: None, 13: 2, 14: 2}, "sigma_indel with mu_indel"),
        ("dig_tiled_nb_test_host", {7: 1, 8: 1, 9: 1}, "non-null pointers"),
        ("dig_accumulate_elements_host", {8: 1, 20: -1}, "N, E, C >= 0"),
        ("dig_accumulate_elements_host", {**{i: buf for i in range(20)}, 5: i64(0, 1), 6: i32(5), 8: 1, 20: 4, 21: 1, 22: 1},
         "ov_idx within [0, N)"),
        ("dig_gene_stats_host", {5: 4, 14: -1}, "G, C >= 0"),
        ("dig_scale_suffstats_host", {2: 5, 3: 2, 4: buf}, "non-null inputs"),
        ("dig_gather_bins_host", {2: 1, 3: 0, 4: 1}, "sizes"),
        ("dig_gather_bins_host", {0: buf, 2: 2, 3: 1, 4: 1, 5: i64(7), 6: 1, 8: 1, 9: buf}, "bin_rows within [0, N)"),
        ("dig_count_contexts_host", {1: 4, 9: -1}, "R >= 0, n_words >= 2 (pad words), n_chrom >= 0"),
        ("dig_count_contexts_host", {**{i: buf for i in (0, 2, 3, 6, 7, 8, 10)}, 1: 4, 4: 1, 5: i32(1), 9: 1},
         "region chromosome index within [0, n_chrom)"),
        ("dig_count_contexts2_host", {1: 27, 14: 1}, "R, n_int, n_chrom >= 0, n_words2 >= 28 (pad words)"),
        ("dig_element_pipeline_host", {25: 1, 26: -1, 27: 1}, "N, E, C >= 0"),
        ("dig_gene_pipeline_host", {25: 1, 26: 1, 27: 1}, "non-null accumulation inputs"),
        ("dig_base_tile_probs_host", {1: 1, 8: 1}, "non-negative sizes, n_words >= 2 (pad words)"),
        ("dig_base_tile_probs_ctx_host", {1: 4, 8: 1, 11: 3}, "n_up = n_down = 1 or 2"),
        ("dig_tile_mut_counts_host", {8: 0, 9: 1, 10: 1, 11: 1}, "non-negative sizes, binsize >= 1"),
        ("dig_tile_mut_counts_host", {**{i: buf for i in (3, 5, 6, 7, 12)}, 0: i32(0), 1: i32(3), 2: 1, 4: 1, 8: 1, 9: 1, 10: 2, 11: 1},
         "pairs inside the mutation / region tables"),
        ("dig_overlap_join_count_host", {7: -1}, "sizes >= 0"),
        ("dig_overlap_join_fill_host", {3: 1, 7: 1, 9: -1}, "sizes >= 0"),
    ]
    for name, over, fragment in cases:
        args = [None if t is ctypes.c_void_p else 0 for t in _lib._SIGNATURES[name]]
        for i, v in over.items():
            args[i] = _lib.host_ptr(v) if isinstance(v, np.ndarray) else v
        rc = getattr(lib, name)(*args)
        msg = _lib.last_error()
        assert rc == -1, (name, rc, msg)
        assert fragment in msg, (name, msg)
        assert fragment.startswith("nb3_host") or name in msg, (name, msg)


def test_native_result_writer_writes_the_bytes_pandas_writes(tmp_path):
    """mapfile.write_results_tsv (dig_write_tsv_host: std::to_chars digits + the layout rules of Python's float repr) against
    DataFrame.to_csv(sep="\\t") -- what DigDriver.py writes (DigDriver.py:115-118) -- byte for byte: p-values down to the
    subnormals, whole numbers, 1e-4 / 1e16 switch-overs, NaN, infinities, signed zeros, integers, bools; and the fall-back to
    pandas for frames the writer does not cover."""
    import numpy as np
    import pandas as pd
    from digdriver_amd.io import mapfile
    rng = np.random.default_rng(0)
    n = 20_011
    edge = np.array([0.0, -0.0, 5e-324, 2.2250738585072014e-308, 1e-5, 9.999999999999999e-05, 1e-4, 0.00012345, 0.1, 1 / 3, 1.0, 12.0, 123456.0,
                     1e15, 9999999999999998.0, 1e16, 1.2345e16, 1e22, 1.7976931348623157e308, np.inf, -np.inf, np.nan, -1.5e-7, -2.5, 100.0, 1e-300])
    cols = {
        'ELT_SIZE': rng.integers(200, 9000, n), 'FLAG': rng.uniform(size=n) < 0.1, 'MU': rng.gamma(9, 3, n),
        'PVAL': 10.0 ** rng.uniform(-320, 0, n), 'Z': np.where(rng.uniform(size=n) < 0.01, np.nan, rng.normal(size=n)),
        'WHOLE': rng.integers(0, 50, n).astype(float), 'BIG': rng.uniform(1e15, 1e18, n), 'SMALL': rng.uniform(1e-6, 1e-3, n),
        'BITS': rng.integers(0, 2 ** 63 - 1, n, dtype=np.int64).view(np.float64), 'OBS': rng.integers(-5, 50, n).astype(np.int32),
        'EDGE': np.resize(edge, n)}
    df = pd.DataFrame(cols, index=pd.Index(['ELT%06d' % i for i in range(n)], name='ELT'))
    a, b = tmp_path / "native.txt", tmp_path / "pandas.txt"
    df.to_csv(str(b), header=True, index=True, sep="\t")
    for threads in (8, 1, 3):                             # several threads with their own chunks; one thread streaming chunk by chunk
        mapfile.write_results_tsv(df, str(a), threads=threads)
        assert a.read_bytes() == b.read_bytes(), threads
    back = pd.read_csv(str(a), sep="\t", index_col=0, float_precision="round_trip")
    assert np.array_equal(back.PVAL.values, df.PVAL.values) and np.array_equal(back.BITS.values, df.BITS.values, equal_nan=True)
    # an unnamed integer index, no rows, no columns
    for frame in (df.reset_index(drop=True).iloc[:7], df.iloc[:0], df.iloc[:5, :0]):
        mapfile.write_results_tsv(frame, str(a))
        frame.to_csv(str(b), header=True, index=True, sep="\t")
        assert a.read_bytes() == b.read_bytes()
    # not covered: a string column, a label with a tab -> pandas writes them
    for frame in (df.iloc[:5].assign(NAME=list("abcde")), df.iloc[:3].rename(index={'ELT000001': 'a\tb'})):
        mapfile.write_results_tsv(frame, str(a))
        frame.to_csv(str(b), header=True, index=True, sep="\t")
        assert a.read_bytes() == b.read_bytes()
    # indexes the native path must leave to pandas: an object index of integers FOLLOWED by the equal index of
    # floats (Index.equals says "same": the label cache must not hand 1 / 2 / 3 to a frame that prints 1.0 / 2.0 / 3.0), a None /
    # NaN label, dates, a float index, a nullable integer column with a missing value
    small = df.iloc[:3, :4]
    frames = [small.set_axis(pd.Index([1, 2, 3], dtype=object)), small.set_axis(pd.Index([1.0, 2.0, 3.0], dtype=object)),
              small.set_axis(pd.Index(['a', None, 'c'], dtype=object)), small.set_axis(pd.Index(['a', np.nan, 'c'], dtype=object)),
              small.set_axis(pd.to_datetime(['2020-01-01', '2020-01-02', '2020-01-03'])), small.set_axis(pd.Index([0.5, 1.5, 2.5])),
              small.assign(NA_INT=pd.array([1, None, 3], dtype="Int64")), small.set_axis(pd.Index([7, 8, 9], name='ID'))]
    for frame in frames:
        mapfile.write_results_tsv(frame, str(a))
        frame.to_csv(str(b), header=True, index=True, sep="\t")
        assert a.read_bytes() == b.read_bytes(), frame.index
