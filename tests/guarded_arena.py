"""A guarded arena for the device entry points of include/dig_hip.h: where the pointers sit and what lies around them.

The suite's oracles pin what a kernel computes.  This helper pins where it reads and writes.  Every pointer argument of one
call is carved, as a contiguous view, from ONE uint8 slab (a torch tensor: on the GPU for the entry points, on the CPU for the
helper's own tests):

    | front band of a | a | rear band of a | front band of b | b | rear band of b | ...

  * bands: at least BAND = 64 KiB each (more than one 4096-element tile of doubles); the slab's two ends are bands.
  * placement: a buffer starts at EXACTLY the alignment `a` its argument is documented with and no more: address = a (mod 2a).
    The default is the element size (8 f64 / i64, 4 i32 / u32 / f32, 2 i16 / bf16, 1 = an odd address for u8); a test passes the
    documented exceptions (256, 16, 8).  A workspace is carved with exactly the bytes its size query returned: its rear band
    starts at the next byte.
  * typed, in-domain poison: a band holds values of its buffer's type, in two variants A and B that differ in every element:
    NaN / 1e300 for doubles (1e30 for f32 and bf16), 0 / 1 for bytes (flags), 0x00000000 / 0xFFFFFFFF for genome words, and for
    whatever a kernel uses as an index, offset, row, track, chromosome id or key two VALID, different values of that domain
    (`index=(lo, hi)`).  An over-read then shows up as a wrong number and can never become a wild address; a float pattern for
    an argument marked as an index is refused.
  * inputs are copied in; outputs and workspaces are pre-filled with their poison (A or B), so reliance on what a scratch
    buffer held before the call differs between the two runs as well.

After the call (and a synchronize) `violations()` compares every band, on the slab's device, with what was put there and names
the argument, the side and the first byte offset; `guarded_runs` runs both variants and requires bit-identical outputs.

Limit: an over-READ whose value never reaches an output is not detectable this way (and, inside the slab, harmless); an
over-read that does reach one is seen as an A / B difference, not located.  Stores are located exactly, up to a band's width
(a store further than 64 KiB from its buffer lands in a neighbour's band or buffer, or outside the slab).
"""
import bisect

import numpy as np

BAND = 64 * 1024

_NP = {"f64": np.dtype(np.float64), "f32": np.dtype(np.float32), "i64": np.dtype(np.int64), "i32": np.dtype(np.int32),
       "u32": np.dtype(np.uint32), "i16": np.dtype(np.int16), "u8": np.dtype(np.uint8), "bf16": np.dtype(np.uint16)}
_FLOAT = ("f64", "f32", "bf16")
# variant A, variant B by type (bf16 as its bit pattern: NaN / 1e30)
_DEFAULT_POISON = {"f64": (np.nan, 1e300), "f32": (np.nan, 1e30), "bf16": (0x7FC0, 0x714A), "i64": (0, 1 << 40), "i32": (0, 1 << 20),
                   "u32": (0x00000000, 0xFFFFFFFF), "i16": (0, 12345), "u8": (0, 1)}


_TORCH = {"f64": "float64", "f32": "float32", "i64": "int64", "i32": "int32", "u32": "int32", "i16": "int16", "u8": "uint8",
          "bf16": "bfloat16"}                     # (u32 as its int32 bits)


class GuardViolation(AssertionError):
    pass


class Buf:
    """One pointer argument.  role: "in" (data copied in), "out" (shape given, pre-filled with poison) or "ws" (nbytes given,
    dtype u8 unless said otherwise, pre-filled with poison).  align: the documented alignment in bytes (default: the element
    size).  index=(lo, hi): the values are indices / offsets / ids / keys of the closed domain [lo, hi]; the poison is then lo / hi
    (or the explicit pair `poison`, which must lie inside the domain)."""

    def __init__(self, role, dtype, data=None, shape=None, nbytes=None, align=None, index=None, poison=None):
        assert role in ("in", "out", "ws") and dtype in _NP
        self.role, self.dtype, self.np = role, dtype, _NP[dtype]
        if role == "in":
            data = np.ascontiguousarray(data)
            assert data.dtype == self.np, "input of dtype %s given for a %s argument" % (data.dtype, dtype)
            self.data, self.shape, self.nbytes = data, data.shape, data.nbytes
        elif role == "out":
            self.data, self.shape = None, tuple(int(s) for s in (shape if hasattr(shape, "__len__") else (shape,)))
            self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.np.itemsize
        else:
            self.data, self.nbytes = None, int(nbytes)
            assert self.nbytes % self.np.itemsize == 0
            self.shape = (self.nbytes // self.np.itemsize,)
        self.align = int(align) if align is not None else self.np.itemsize
        assert self.align >= self.np.itemsize and self.align & (self.align - 1) == 0 and self.align <= 4096
        self.index = index
        if index is not None:
            lo, hi = index
            pair = poison if poison is not None else (lo, hi)
            for v in pair:
                if dtype in _FLOAT or isinstance(v, (float, np.floating)) or v != v:
                    raise ValueError("a float pattern for an argument marked as an index is refused: %r" % (pair,))
                if not lo <= v <= hi:
                    raise ValueError("index poison %r lies outside the valid domain [%r, %r]" % (v, lo, hi))
            if pair[0] == pair[1]:
                raise ValueError("the two poison variants of an index must differ (a domain of one value cannot tell them apart)")
            self.poison = pair
        else:
            self.poison = poison if poison is not None else _DEFAULT_POISON[dtype]

    def fill(self, variant):
        """The poison element of variant "A" / "B" as a 0-d array of the buffer's type."""
        return np.array(self.poison[0 if variant == "A" else 1]).astype(self.np)


def inp(dtype, data, **kw):
    return Buf("in", dtype, data=data, **kw)


def out(dtype, shape, **kw):
    return Buf("out", dtype, shape=shape, **kw)


def ws(nbytes, dtype="u8", **kw):
    return Buf("ws", dtype, nbytes=nbytes, **kw)


def _round_up(x, m):
    return (x + m - 1) // m * m


class GuardedArena:
    """The slab of one call.  bufs: dict name -> Buf (in argument order); variant "A" or "B"; device: a torch device."""

    def __init__(self, bufs, variant, device="cpu"):
        import torch
        assert variant in ("A", "B")
        self.torch, self.bufs, self.variant = torch, dict(bufs), variant
        total = BAND + sum(2 * BAND + b.nbytes + 2 * 2 * b.align + 16 for b in self.bufs.values()) + BAND
        # the slab starts at a multiple of 8192 (2 a of the largest alignment a buffer may ask for): where a buffer lands in its slab
        # then follows from the buffers alone, not from the address the allocator gave, so two arenas over the same buffers agree
        raw = torch.empty(total + 8192, dtype=torch.uint8, device=device)
        self.slab = raw[-raw.data_ptr() % 8192:][:total]
        self.base = self.slab.data_ptr()
        assert self.base % 8192 == 0
        # placement: front band, buffer at a (mod 2a), rear band from the buffer's last byte + 1
        self.off, self.bands = {}, []               # name -> byte offset; bands: (start, end, name, side)
        cur = 0
        for name, b in self.bufs.items():
            a = b.align
            start = cur + BAND
            start += (a - (self.base + start)) % (2 * a)
            assert (self.base + start) % (2 * a) == a
            self.off[name] = start
            end = start + b.nbytes
            rear_end = _round_up(end + BAND, 8)
            self.bands.append((cur, start, name, "front"))
            self.bands.append((end, rear_end, name, "rear"))
            cur = rear_end
        assert cur + BAND <= total
        s, _, name, side = self.bands[-1]
        self.bands[-1] = (s, total, name, side)     # the slab's far end belongs to the last rear band
        host = np.zeros(total, np.uint8)
        mask = np.zeros(total, np.uint8)
        for s, e, name, side in self.bands:
            b = self.bufs[name]
            self._fill(host, s, e, self.off[name], b)
            mask[s:e] = 1
        for name, b in self.bufs.items():
            s = self.off[name]
            if b.role == "in":
                host[s:s + b.nbytes] = b.data.reshape(-1).view(np.uint8)
            else:
                self._fill(host, s, s + b.nbytes, s, b)
        self.slab.copy_(torch.from_numpy(host))
        self.expected = self.slab.clone()
        self.mask = torch.from_numpy(mask).to(self.slab.device).bool()
        self._starts = [s for s, _, _, _ in self.bands]

    def _fill(self, host, s, e, anchor, b):
        """Bytes [s, e) of the image <- the poison element, laid on the grid of the buffer that starts at `anchor` (so that a
        band reads as an extension of its buffer's array, before and behind it)."""
        w = b.np.itemsize
        pat = np.frombuffer(b.fill(self.variant).tobytes(), np.uint8)
        idx = (np.arange(s, e, dtype=np.int64) - anchor) % w
        host[s:e] = pat[idx]

    # ---- pointers and views ------------------------------------------------------------------------------
    def ptr(self, name):
        """The address of a buffer (an int; None for a name that was not carved: a NULL argument)."""
        return None if name not in self.off else self.base + self.off[name]

    def window(self, name, lo=0, hi=None):
        """Elements [lo, hi) counted from the buffer's first element as a typed torch view of the slab -- pointer arithmetic:
        lo may be negative and hi may pass the end (what a stand-in entry point of the self-tests indexes)."""
        b = self.bufs[name]
        w = b.np.itemsize
        hi = b.nbytes // w if hi is None else hi
        raw = self.slab[self.off[name] + lo * w: self.off[name] + hi * w]
        return raw.view(getattr(self.torch, _TORCH[b.dtype]))

    def tensor(self, name):
        """The carved buffer itself as a typed torch view (u32 as int32 bits), in its shape."""
        return self.window(name).reshape(self.bufs[name].shape)

    def read(self, name):
        """A host copy of a buffer as a numpy array of its type and shape (bf16 as uint16 bit patterns)."""
        b = self.bufs[name]
        raw = self.slab[self.off[name]: self.off[name] + b.nbytes].cpu().numpy()
        return raw.view(b.np).reshape(b.shape).copy()

    # ---- the check ---------------------------------------------------------------------------------------
    def violations(self, limit=8):
        """[(argument, side, first byte offset into that band)] of every band that no longer holds what was put there.  The
        comparison runs on the slab's device; the rear band's offsets count from the buffer's last byte + 1, the front band's
        back from the buffer's first byte (offset 0 = the element just in front of it); both are rounded down to the element of the
        buffer's type that holds the first changed byte."""
        torch = self.torch
        if self.slab.is_cuda:
            torch.cuda.synchronize(self.slab.device)
        bad = (self.slab != self.expected) & self.mask
        if not bool(bad.any()):
            return []
        pos = torch.nonzero(bad).reshape(-1).cpu().numpy()
        found = {}
        for p in pos:
            s, e, name, side = self.bands[bisect.bisect_right(self._starts, int(p)) - 1]
            assert s <= p < e
            o = int(p) - s if side == "rear" else e - 1 - int(p)
            o -= o % self.bufs[name].np.itemsize          # the first byte of the ELEMENT touched (a store may leave low bytes as they were)
            key = (name, side)
            found[key] = min(found.get(key, o), o)
        return [(n, s, o) for (n, s), o in sorted(found.items(), key=lambda kv: self.off[kv[0][0]])][:limit]

    def assert_intact(self, what=""):
        v = self.violations()
        if v:
            raise GuardViolation("%s touched memory outside its arguments: %s" % (
                what or "the call", "; ".join("%s band of `%s`, byte offset %d" % (s, n, o) for n, s, o in v)))


class PlainBuffers:
    """The same interface on ordinary tensors, one allocation per argument (the allocator's own alignment, outputs and
    workspaces zeroed): the call every guarded run must equal bit for bit."""

    def __init__(self, bufs, device="cpu"):
        import torch
        self.torch, self.bufs, self.t = torch, dict(bufs), {}
        for name, b in self.bufs.items():
            if b.role == "in":
                self.t[name] = torch.from_numpy(b.data.reshape(-1).view(np.uint8).copy()).to(device)
            else:
                self.t[name] = torch.zeros(max(b.nbytes, 1), dtype=torch.uint8, device=device)

    def ptr(self, name):
        return None if name not in self.t else self.t[name].data_ptr()

    def window(self, name, lo=0, hi=None):
        b = self.bufs[name]
        return self.t[name][:b.nbytes].view(getattr(self.torch, _TORCH[b.dtype]))[lo:hi]

    def read(self, name):
        b = self.bufs[name]
        return self.t[name][:b.nbytes].cpu().numpy().view(b.np).reshape(b.shape).copy()

    def assert_intact(self, what=""):
        if self.t and next(iter(self.t.values())).is_cuda:
            self.torch.cuda.synchronize()


def same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.reshape(-1).view(np.uint8), y.reshape(-1).view(np.uint8))


def guarded_runs(bufs, invoke, device="cpu", what="", plain=False):
    """Run `invoke(arena)` on a variant-A and a variant-B arena.  Checks (a) every band intact after each run and (b) every
    output bit-identical between the two; with plain=True also on PlainBuffers, whose outputs must carry the same bits.  Returns
    dict name -> numpy array of the outputs (role "out") for the caller's comparison with the reference, check (c)."""
    res = {}
    for variant in ("A", "B"):
        arena = GuardedArena(bufs, variant, device)
        invoke(arena)
        arena.assert_intact("%s (poison %s)" % (what or "the call", variant))
        res[variant] = {n: arena.read(n) for n, b in bufs.items() if b.role == "out"}
    for n in res["A"]:
        if not same_bits(res["A"][n], res["B"][n]):
            d = np.flatnonzero(res["A"][n].reshape(-1).view(np.uint8) != res["B"][n].reshape(-1).view(np.uint8))
            raise GuardViolation("%s: output `%s` depends on what lies around its arguments or in its scratch: poison A and B give "
                                 "different bits, first at byte offset %d (element %d)" %
                                 (what or "the call", n, int(d[0]), int(d[0]) // bufs[n].np.itemsize))
    if plain:
        pb = PlainBuffers(bufs, device)
        invoke(pb)
        pb.assert_intact()
        for n in res["A"]:
            got = pb.read(n)
            if not same_bits(res["A"][n], got):
                d = np.flatnonzero(res["A"][n].reshape(-1).view(np.uint8) != got.reshape(-1).view(np.uint8))
                raise GuardViolation("%s: output `%s` at the documented minimum alignment differs from the call on ordinary tensors, "
                                     "first at element %d" % (what or "the call", n, int(d[0]) // bufs[n].np.itemsize))
    return res["A"]
