"""CPU-only: dig_element_rates_prepare, dig_element_rates_bytes and DIG_PIPE_ELEMENT_RATES are exported, declared and bound, and
bad arguments are refused with a message on the host, before any device call (no device is needed to see it)."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT
from digdriver_amd import _lib

NAME = "dig_element_rates_prepare"


def test_symbols_are_exported_declared_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dig_hip.h")).read()
    assert NAME in _lib.EXPORTED_SYMBOLS and hasattr(lib, NAME) and "int " + NAME + "(" in header
    assert "dig_element_rates_bytes" in _lib.EXPORTED_SYMBOLS and "int64_t dig_element_rates_bytes(" in header
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    assert _lib._SIGNATURES[NAME] == [vp, vp, vp, i64, i64, i64, vp, i64, vp]
    assert getattr(lib, NAME).argtypes == _lib._SIGNATURES[NAME]
    assert _lib.DIG_PIPE_ELEMENT_RATES == 128 == int(re.search(r"#define\s+DIG_PIPE_ELEMENT_RATES\s+(\d+)", header).group(1))
    flags = (_lib.DIG_PIPE_CONTEXTS, _lib.DIG_PIPE_DOT, _lib.DIG_PIPE_STATISTICS, _lib.DIG_PIPE_WORKLIST_CLEAN, _lib.DIG_PIPE_COMPACT_L,
             _lib.DIG_PIPE_RECORDS, _lib.DIG_PIPE_ELEMENT_CTX, _lib.DIG_PIPE_ELEMENT_RATES)
    assert sorted(flags) == [1, 2, 4, 8, 16, 32, 64, 128]
    assert lib.dig_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define\s+DIG_ABI_VERSION\s+(\d+)", header).group(1))


def test_table_size_is_24_bytes_a_pair_in_whole_tiles():
    size = _lib.load().dig_element_rates_bytes
    assert [size(1, 1), size(1, 64), size(1, 65), size(70, 37), size(120_091, 37)] == \
        [1536, 1536, 3072, (70 * 37 + 63) // 64 * 1536, (120_091 * 37 + 63) // 64 * 1536]
    assert size(0, 5) == size(5, 0) == size(-1, 5) == 0


def _refused(rc, fragment):
    msg = _lib.last_error()
    assert rc == -1, (rc, msg)
    assert fragment in msg, msg


def test_rates_prepare_checks_its_arguments_on_the_host():
    lib = _lib.load()
    fn = getattr(lib, NAME)
    raw = np.zeros(8192, np.uint8)
    base = raw.ctypes.data + (-raw.ctypes.data % 256)          # (host memory: every check below fails before it is read)
    big = 1 << 20
    _refused(fn(base, base, base, -1, 1, 1, base, big, None), "N, E, C >= 0")
    _refused(fn(base, base, base, 1, -1, 1, base, big, None), "N, E, C >= 0")
    _refused(fn(base, base, base, 1, 1, -1, base, big, None), "N, E, C >= 0")
    _refused(fn(base, None, base, 1, 1, 1, base, big, None), "non-null")
    _refused(fn(base, base, base, 1, 1, 1, None, big, None), "non-null")
    _refused(fn(None, base, base, 1, 1, 1, base, big, None), "non-null")
    _refused(fn(base, base, None, 1, 1, 1, base, big, None), "non-null")
    _refused(fn(base, base, base, 1, 1, 65, base, 3071, None), "dig_element_rates_bytes")
    _refused(fn(base, base, base, 1, 1 << 20, 1 << 12, base, big, None), "below 2^32 - 1")
    for off in (8, 16, 128):
        _refused(fn(base, base, base, 1, 1, 1, base + off, big, None), "rates 256-byte aligned")
        _refused(fn(base + off, base, base, 1, 1, 1, base, big, None), "bin_records 256-byte aligned")
    assert NAME in _lib.last_error()
    assert fn(None, None, None, 0, 0, 0, None, 0, None) == 0    # no pairs: nothing to do


def test_pipeline_refuses_the_flag_without_packed_records_and_a_bad_table():
    lib = _lib.load()
    sig = _lib._SIGNATURES["dig_element_pipeline"]
    stages_at = len(sig) - 4
    records_at = stages_at - 1
    assert sig[stages_at] is ctypes.c_int and sig[records_at] is ctypes.c_void_p

    def call(stages, table=None, records=None):
        args = [None if t is ctypes.c_void_p else 0 for t in sig]
        args[0], args[25], args[26], args[27], args[records_at], args[stages_at] = table, 1, 1, 1, records, stages
        return lib.dig_element_pipeline(*args)

    raw = np.zeros(1024, np.uint8)
    base = raw.ctypes.data + (-raw.ctypes.data % 256)
    R = _lib.DIG_PIPE_ELEMENT_RATES
    for stages in (7 | R, 4 | R | _lib.DIG_PIPE_COMPACT_L, 4 | R | _lib.DIG_PIPE_RECORDS, R):
        _refused(call(stages, table=base), "DIG_PIPE_ELEMENT_RATES needs the packed bin records")
    _refused(call(7 | R, table=None, records=base), "DIG_PIPE_ELEMENT_RATES needs the rate table")
    for off in (8, 64, 128):
        _refused(call(7 | R, table=base + off, records=base), "256-byte aligned")
