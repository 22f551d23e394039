"""CPU-only: dig_element_contexts_prepare and DIG_PIPE_ELEMENT_CTX are exported, declared and bound, the ABI is still 12, and
bad arguments are refused with a message on the host, before any device call (no device is needed to see it)."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT
from digdriver_amd import _lib

NAME = "dig_element_contexts_prepare"


def test_symbol_is_exported_declared_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dig_hip.h")).read()
    assert NAME in _lib.EXPORTED_SYMBOLS and hasattr(lib, NAME) and "int " + NAME + "(" in header
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    assert _lib._SIGNATURES[NAME] == [vp, vp, vp, vp, i64, i64, vp, vp]
    assert getattr(lib, NAME).argtypes == _lib._SIGNATURES[NAME]
    assert _lib.DIG_PIPE_ELEMENT_CTX == 64 == int(re.search(r"#define\s+DIG_PIPE_ELEMENT_CTX\s+(\d+)", header).group(1))
    flags = (_lib.DIG_PIPE_CONTEXTS, _lib.DIG_PIPE_DOT, _lib.DIG_PIPE_STATISTICS, _lib.DIG_PIPE_WORKLIST_CLEAN, _lib.DIG_PIPE_COMPACT_L,
             _lib.DIG_PIPE_RECORDS, _lib.DIG_PIPE_ELEMENT_CTX)
    assert sorted(flags) == [1, 2, 4, 8, 16, 32, 64]
    assert lib.dig_abi_version() == _lib.ABI_VERSION == 12
    assert int(re.search(r"#define\s+DIG_ABI_VERSION\s+(\d+)", header).group(1)) == 12


def _refused(rc, fragment):
    msg = _lib.last_error()
    assert rc == -1, (rc, msg)
    assert fragment in msg, msg


def test_contexts_prepare_checks_its_arguments_on_the_host():
    lib = _lib.load()
    fn = getattr(lib, NAME)
    raw = np.zeros(4096, np.uint8)
    base = raw.ctypes.data + (-raw.ctypes.data % 256)          # (host memory: every check below fails before it is read)
    _refused(fn(base, base, base, base, -1, 1, base, None), "N, E >= 0")
    _refused(fn(base, base, base, base, 1, -1, base, None), "N, E >= 0")
    _refused(fn(base, None, base, base, 1, 1, base, None), "non-null")
    _refused(fn(base, base, base, None, 1, 1, base, None), "non-null")
    _refused(fn(base, base, base, base, 1, 1, None, None), "non-null")
    _refused(fn(None, base, base, base, 1, 1, base, None), "non-null")
    _refused(fn(base, base, None, base, 1, 1, base, None), "non-null")
    for off in (4, 16, 128):
        _refused(fn(base, base, base, base, 1, 1, base + off, None), "elt_ctx 256-byte aligned")
    assert NAME in _lib.last_error()
    assert fn(None, None, None, None, 0, 0, None, None) == 0    # no elements: nothing to do


def test_pipeline_refuses_the_flag_without_the_compact_form_and_a_misaligned_table():
    lib = _lib.load()
    sig = _lib._SIGNATURES["dig_element_pipeline"]
    stages_at = len(sig) - 4
    assert sig[stages_at] is ctypes.c_int

    def call(stages, bin_ctx=None, N=1):
        args = [None if t is ctypes.c_void_p else 0 for t in sig]
        args[4], args[25], args[26], args[27], args[stages_at] = bin_ctx, N, 1, 1, stages
        return lib.dig_element_pipeline(*args)

    for stages in (7 | _lib.DIG_PIPE_ELEMENT_CTX, 2 | _lib.DIG_PIPE_ELEMENT_CTX | _lib.DIG_PIPE_RECORDS, _lib.DIG_PIPE_ELEMENT_CTX):
        _refused(call(stages), "DIG_PIPE_ELEMENT_CTX is valid only together with DIG_PIPE_COMPACT_L")
    raw = np.zeros(1024, np.uint8)
    base = raw.ctypes.data + (-raw.ctypes.data % 256)
    _refused(call(7 | _lib.DIG_PIPE_COMPACT_L | _lib.DIG_PIPE_ELEMENT_CTX, bin_ctx=base + 64), "256-byte aligned")
    _refused(call(7 | _lib.DIG_PIPE_COMPACT_L | _lib.DIG_PIPE_ELEMENT_CTX, bin_ctx=base, N=-1), "N >= 1")
