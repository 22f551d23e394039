"""The host half of the backend pair (digdriver_amd/_marshal.py): what every `_host` path of engine.py / nb_model.py now relies on.
No device and no library call: _lib.call is replaced by a recorder."""
import ctypes
import subprocess
import sys

import numpy as np
import pytest

from digdriver_amd import _lib, _marshal


@pytest.fixture
def be():
    return _marshal.HostBackend(3)


def test_arr_copies_only_when_needed(be):
    a = np.arange(12, dtype=np.float64).reshape(3, 4)
    assert be.arr(a, "f64") is a                                     # right dtype, contiguous: the very same array
    assert np.shares_memory(be.arr(a, "f64", (4, 3)), a)             # a reshape of it is a view
    assert be.arr(a) is a                                            # dtype None keeps the array's own
    b = be.arr(a, "i32")
    assert b.dtype == np.int32 and not np.shares_memory(b, a) and np.array_equal(b, a)
    for name, dt in (("f64", np.float64), ("f32", np.float32), ("i64", np.int64), ("i32", np.int32), ("u32", np.uint32),
                     ("i16", np.int16), ("u8", np.uint8)):
        assert be.arr([1, 2, 3], name).dtype == dt and be.empty((2, 3), name).dtype == dt


def test_arr_makes_contiguous(be):
    a = np.arange(24, dtype=np.int32).reshape(4, 6)
    for view in (a.T, a[:, ::2], a[::-1]):
        assert not view.flags["C_CONTIGUOUS"]
        got = be.arr(view, "i32")
        assert got.flags["C_CONTIGUOUS"] and np.array_equal(got, view)
        assert be.ptr(got).value == got.ctypes.data                 # (host_ptr refuses anything else)
    assert be.arr(a.T, "i32", (-1,)).shape == (24,)


def test_broadcast_gives_contiguous_arrays_of_one_shape(be):
    x, y, z = be.broadcast((np.arange(3.0), 2, [[1], [2]]), "f64")
    assert x.shape == y.shape == z.shape == (2, 3)
    assert all(v.dtype == np.float64 and v.flags["C_CONTIGUOUS"] for v in (x, y, z))
    assert np.array_equal(y, np.full((2, 3), 2.0)) and np.array_equal(z, [[1, 1, 1], [2, 2, 2]])
    s, t = be.broadcast((1.5, 2), "f64")                             # scalars stay 0-d: the caller returns floats for them
    assert s.shape == t.shape == () and be.ptr(s).value == s.ctypes.data


def test_none_is_null(be):
    assert be.arr(None, "f64") is None and be.arr(None, "f64", (2, 2)) is None and be.arr(None) is None
    assert be.ptr(None) is None
    assert ctypes.cast(be.ptr(None), ctypes.c_void_p).value is None


def test_call_derives_the_host_name_and_appends_the_device(be, monkeypatch):
    seen = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: seen.append((name, args)))
    be.call("dig_scale_suffstats", 1, 2, workspace=("scratch", 64))  # the workspace of the device form is dropped
    be.call("dig_fisher", 5)
    assert seen == [("dig_scale_suffstats_host", (1, 2, 3)), ("dig_fisher_host", (5, 3))]
    assert _marshal.HostBackend("cuda:0").ordinal == 0                # (as the host paths always did for a non-integer device)


def test_backend_of_and_on_pick_the_host_backend():
    be = _marshal.backend_of(np.zeros(2), None, [1.0], device=2)
    assert isinstance(be, _marshal.HostBackend) and be.ordinal == 2 and not be.is_device and be.dev is None
    assert isinstance(_marshal.backend_on(1, False), _marshal.HostBackend)


def test_host_backend_does_not_import_torch():
    code = ("import sys, numpy as np\n"
            "from digdriver_amd import _marshal, engine\n"
            "from digdriver_amd.sequence_model import nb_model\n"
            "be = _marshal.backend_of(np.zeros(3), device=0)\n"
            "be.arr([[1, 2]], 'f64', (2,)); be.empty((2, 2), 'i32'); be.ptr(be.arr(None)); be.broadcast((1.0, [2.0]), 'f64')\n"
            "assert not _marshal.is_cuda(np.zeros(1))\n"
            "assert 'torch' not in sys.modules, 'the host backend imported torch'\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=_lib._HERE + "/..")
