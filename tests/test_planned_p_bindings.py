"""CPU-only: dig_element_p_prepare, dig_element_p_bytes and DIG_PIPE_ELEMENT_P are exported, declared and bound, and bad
arguments are refused with a message on the host, before any device call (no device is needed to see it)."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT
from digdriver_amd import _lib

NAME = "dig_element_p_prepare"


def test_symbols_are_exported_declared_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dig_hip.h")).read()
    assert NAME in _lib.EXPORTED_SYMBOLS and hasattr(lib, NAME) and "int " + NAME + "(" in header
    assert "dig_element_p_bytes" in _lib.EXPORTED_SYMBOLS and "int64_t dig_element_p_bytes(" in header
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    assert _lib._SIGNATURES[NAME] == [vp, vp, vp, vp, i64, i64, vp, i64, vp]
    assert getattr(lib, NAME).argtypes == _lib._SIGNATURES[NAME]
    declared = re.search(r"int " + NAME + r"\(([^;]*)\);", header).group(1)
    assert [a.strip().split()[-1].lstrip("*") for a in declared.split(",")] == \
        ["P", "R_SIZE", "ELT_SIZE", "P_INDEL", "E", "C", "table", "table_bytes", "stream"]
    assert _lib.DIG_PIPE_ELEMENT_P == 256 == int(re.search(r"#define\s+DIG_PIPE_ELEMENT_P\s+(\d+)", header).group(1))
    flags = (_lib.DIG_PIPE_CONTEXTS, _lib.DIG_PIPE_DOT, _lib.DIG_PIPE_STATISTICS, _lib.DIG_PIPE_WORKLIST_CLEAN, _lib.DIG_PIPE_COMPACT_L,
             _lib.DIG_PIPE_RECORDS, _lib.DIG_PIPE_ELEMENT_CTX, _lib.DIG_PIPE_ELEMENT_RATES, _lib.DIG_PIPE_ELEMENT_P)
    assert sorted(flags) == [1, 2, 4, 8, 16, 32, 64, 128, 256]
    assert lib.dig_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define\s+DIG_ABI_VERSION\s+(\d+)", header).group(1))


def test_table_size_is_four_sections_of_whole_256_byte_runs():
    size = _lib.load().dig_element_p_bytes
    up = lambda v: (v + 255) // 256 * 256
    want = lambda E, C: up(8 * E * C) + up(8 * E) + 2 * up(4 * E)
    assert [size(1, 1), size(32, 1), size(33, 1), size(64, 65), size(70, 37), size(120_091, 37)] == \
        [1024, 1024, 1536, want(64, 65), want(70, 37), want(120_091, 37)]
    assert size(0, 5) == size(5, 0) == size(-1, 5) == 0


def _refused(rc, fragment):
    msg = _lib.last_error()
    assert rc == -1, (rc, msg)
    assert fragment in msg, msg


def test_p_prepare_checks_its_arguments_on_the_host():
    lib = _lib.load()
    fn = getattr(lib, NAME)
    raw = np.zeros(8192, np.uint8)
    base = raw.ctypes.data + (-raw.ctypes.data % 256)          # (host memory: every check below fails before it is read)
    big = 1 << 20
    _refused(fn(base, base, base, base, -1, 1, base, big, None), "E, C >= 0")
    _refused(fn(base, base, base, base, 1, -1, base, big, None), "E, C >= 0")
    for hole in range(4):
        args = [base] * 4
        args[hole] = None
        _refused(fn(*args, 1, 1, base, big, None), "non-null")
    _refused(fn(base, base, base, base, 1, 1, None, big, None), "non-null")
    _refused(fn(base, base, base, base, 33, 1, base, 1535, None), "dig_element_p_bytes")            # table too small
    _refused(fn(base, base, base, base, 1, 1, base, 0, None), "dig_element_p_bytes")
    _refused(fn(base, base, base, base, 1 << 20, 1 << 12, base, big, None), "below 2^32 - 1")
    for off in (8, 16, 128):
        _refused(fn(base, base, base, base, 1, 1, base + off, big, None), "table 256-byte aligned")
    _refused(fn(base + 4, base, base, base, 1, 1, base, big, None), "8-byte")
    _refused(fn(base, base + 2, base, base, 1, 1, base, big, None), "4-byte")
    assert NAME in _lib.last_error()
    assert fn(None, None, None, None, 0, 0, None, 0, None) == 0    # no pairs: nothing to do


def test_pipeline_refuses_the_flag_with_a_missing_or_misaligned_table():
    lib = _lib.load()
    sig = _lib._SIGNATURES["dig_element_pipeline"]
    stages_at = len(sig) - 4
    assert sig[stages_at] is ctypes.c_int and sig[10] is ctypes.c_void_p

    def call(stages, table=None):
        args = [None if t is ctypes.c_void_p else 0 for t in sig]
        args[10], args[25], args[26], args[27], args[stages_at] = table, 1, 1, 1, stages
        return lib.dig_element_pipeline(*args)

    raw = np.zeros(1024, np.uint8)
    base = raw.ctypes.data + (-raw.ctypes.data % 256)
    F = _lib.DIG_PIPE_ELEMENT_P
    for stages in (7 | F, 2 | F | _lib.DIG_PIPE_COMPACT_L, 4 | F | _lib.DIG_PIPE_RECORDS, F):
        _refused(call(stages), "DIG_PIPE_ELEMENT_P needs the P table")
    for off in (8, 64, 128):
        _refused(call(7 | F, table=base + off), "element P table (DIG_PIPE_ELEMENT_P) 256-byte aligned")
    # the flag is taken out of the mask like the other form flags: what is left must still name a stage
    _refused(call(F, table=base), "stages: bit mask")
    _refused(call(512 | 7, table=base), "stages: bit mask")
