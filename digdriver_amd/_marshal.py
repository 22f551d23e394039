"""The two ways an operation reaches libdig_hip.so, as two small objects with the same methods.

    HostBackend    numpy arrays -> host pointers -> the `<name>_host` twin, which stages through the device itself
    DeviceBackend  torch CUDA tensors -> device pointers -> `<name>` on torch's current stream, zero copies

An operation in engine.py / nb_model.py is written once against `be.arr / be.empty / be.ptr / be.call`; where the two paths
behave differently on purpose it says so with `be.is_device`.  Dtypes are named once ("f64", "i32", ...) and mapped per backend.
HostBackend never imports torch (the torch-free command lines, _lib.TORCH_FREE, depend on it).
"""
import numpy as np

from . import _lib

_NP = {"f64": np.dtype(np.float64), "f32": np.dtype(np.float32), "i64": np.dtype(np.int64), "i32": np.dtype(np.int32),
       "u32": np.dtype(np.uint32), "i16": np.dtype(np.int16), "u8": np.dtype(np.uint8)}


class HostBackend:
    is_device = False
    dev = None                                   # no torch device (what PackedGenome.genome2_args takes for host pointers)

    def __init__(self, device=0):
        self.ordinal = device if isinstance(device, int) else 0      # the card the `_host` twin stages through

    def arr(self, x, dtype=None, shape=None):
        """C-contiguous array of `dtype` (None: x's own), copying only when needed; reshaped when a shape is given."""
        if x is None:
            return None
        a = np.ascontiguousarray(np.asarray(x), dtype=None if dtype is None else _NP[dtype])
        return a if shape is None else a.reshape(shape)

    def broadcast(self, xs, dtype):
        """The inputs of an element-wise operation at their common shape, each contiguous."""
        return [np.ascontiguousarray(v).reshape(v.shape) for v in np.broadcast_arrays(*[np.asarray(x, dtype=_NP[dtype]) for x in xs])]

    def empty(self, shape, dtype):
        return np.empty(shape, _NP[dtype])

    def cat(self, xs, dtype=None):
        """The arrays one after the other as `dtype` (None: their own); none at all: an empty array of it (i64 without one)."""
        return np.concatenate([self.arr(x, dtype) for x in xs]) if len(xs) else self.empty(0, dtype or "i64")

    ptr = staticmethod(_lib.host_ptr)

    def call(self, name, *args, workspace=None):
        _lib.call(name + "_host", *args, self.ordinal)


class DeviceBackend:
    is_device = True
    _cache = {}                                  # torch.device -> backend

    def __init__(self, dev):
        _lib._need_torch()
        import torch
        self.torch, self.dev, self._tensor = torch, dev, torch.Tensor
        self._dt = {"f64": torch.float64, "f32": torch.float32, "bf16": torch.bfloat16, "i64": torch.int64, "i32": torch.int32,
                    "i16": torch.int16, "u8": torch.uint8}

    def arr(self, x, dtype=None, shape=None):
        if x is None:
            return None
        t = x if isinstance(x, self._tensor) and x.device == self.dev else self.torch.as_tensor(x, device=self.dev)
        if dtype is not None and t.dtype != self._dt[dtype]:
            t = t.to(self._dt[dtype])
        t = t.contiguous()
        return t if shape is None or t.shape == shape else t.reshape(shape)

    def broadcast(self, xs, dtype):
        torch = self.torch
        return [v.contiguous() for v in torch.broadcast_tensors(*[torch.as_tensor(x, dtype=self._dt[dtype], device=self.dev) for x in xs])]

    def empty(self, shape, dtype):
        return self.torch.empty(shape, dtype=self._dt[dtype], device=self.dev)

    def cat(self, xs, dtype=None):
        return self.torch.cat([self.arr(x, dtype) for x in xs]) if len(xs) else self.empty(0, dtype or "i64")

    ptr = staticmethod(_lib.dev_ptr)

    def call(self, name, *args, workspace=None):
        """Enqueue `name` on torch's current stream of the backend's device; workspace: (uint8 tensor or None, bytes) for the
        entry points that take scratch."""
        with self.torch.cuda.device(self.dev):
            if workspace is None:
                _lib.call(name, *args, _lib.stream_ptr())
            else:
                _lib.call(name, *args, _lib.dev_ptr(workspace[0]), workspace[1], _lib.stream_ptr())


def is_cuda(x):
    return type(x).__module__.startswith("torch") and getattr(x, "is_cuda", False)


def resolve_device(device):
    """An ordinal, a string or a torch.device -> torch.device."""
    import torch
    return torch.device("cuda", device) if isinstance(device, int) else torch.device(device)


def device_backend(dev):
    """The one DeviceBackend of a card, however it is named (an ordinal, "cuda:0", torch.device("cuda"): the current card)."""
    be = DeviceBackend._cache.get(dev)           # (a tensor's .device, the usual key, is found at once)
    if be is None:
        import torch
        dev = resolve_device(dev)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device(dev.type, torch.cuda.current_device())
        be = DeviceBackend._cache.get(dev)
        if be is None:
            be = DeviceBackend._cache[dev] = DeviceBackend(dev)
    return be


def backend_of(*xs, device=0):
    """The device backend of the first CUDA tensor among xs; without one the host backend staging through `device`."""
    for x in xs:
        if is_cuda(x):
            return device_backend(x.device)
    return HostBackend(device)


def backend_on(device, on_device):
    """For the operations whose inputs are host arrays either way (on_device=True keeps a genome resident and returns tensors)."""
    return device_backend(device) if on_device else HostBackend(device)
