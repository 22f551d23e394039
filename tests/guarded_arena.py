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

On a GPU `guarded_runs` adds a fourth run that pins on which QUEUE the call works: the same call inside a side stream while the
default stream is held busy (`side_stream_run`; `side_stream_call` is the same protocol for a route of the package, used by
tests/test_gpu_side_streams.py).  `judge_side_run` is its verdict, a pure function tested on the CPU.  DESIGN.md section 5.6.
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


# ---- the side-stream run ----------------------------------------------------------------------------------------------------------
# On the null stream a kernel, memset, copy or host wait issued on the wrong queue still gives the right answer.  Here the call
# runs on a side stream while the default stream is held busy by a delay enqueued in front of everything else on it:
#   reading R1 (after side.synchronize() alone, copied on the side stream) still holds poison where a PRODUCER went to the default stream;
#   reading R2 (after the device is idle) differs where a memset or copy went there and CLOBBERED the result after the fact;
#   the default stream must still be busy when R1 has been read: otherwise the call waited for it (or for the device), or the delay
#   was too short, and the case is INCONCLUSIVE -- a failure, never a pass or a skip.
MIN_DELAY_MS, DELAY_FACTOR, MAX_DELAY_MS = 20.0, 10.0, 2000.0
SIDE = {"streams": [], "tried": 0, "cycles_per_ms": None, "muls_per_ms": None, "busy": None, "runs": 0}       # one per process


class SideStreamViolation(GuardViolation):
    pass


def _first_difference(x, y):
    """The first element at which two arrays of one type and shape differ in their bits (None: none)."""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    if x.shape != y.shape or x.dtype != y.dtype:
        return 0
    w = max(x.dtype.itemsize, 1)
    d = np.flatnonzero(x.reshape(-1).view(np.uint8) != y.reshape(-1).view(np.uint8))
    return int(d[0]) // w if d.size else None


def judge_side_run(r1, r2, plain, still_busy, what=""):
    """The verdict of one side-stream run, a pure function of its four observations: r1, r2, plain are dicts output name -> numpy
    array (R1 read on the side stream after its synchronisation alone, R2 after the device went idle, the same call on the default
    stream), still_busy whether the default stream was still busy once R1 had been read.  Raises SideStreamViolation under one of
    three names -- "inconclusive", "late producer", "late clobber" -- with the output, the reading and the first element."""
    what = what or "the call"
    if not still_busy:
        raise SideStreamViolation("%s: inconclusive: the default stream was idle once the side stream's results had been read -- the call "
                                  "waited for the default stream or for the whole device, or the delay in front of it was too short" % what)
    for name in plain:
        e = _first_difference(r1[name], plain[name])
        if e is not None:
            raise SideStreamViolation("%s: late producer: output `%s` was not ready when the side stream was (something that produces it "
                                      "was issued on another stream): reading R1 differs from the default-stream run, first at element %d"
                                      % (what, name, e))
    for name in plain:
        e = _first_difference(r2[name], plain[name])
        if e is not None:
            raise SideStreamViolation("%s: late clobber: output `%s` changed after the side stream had finished (a memset or copy was "
                                      "issued on another stream): reading R2 differs from the default-stream run, first at element %d"
                                      % (what, name, e))


def _timed_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _calibrate(torch, dev):
    """Once per process, two events around a delay on an idle device: spin cycles of torch.cuda._sleep per millisecond (it touches
    no memory, so it does not compete for HBM with the call under test); without that attribute the multiplications of a 256 MiB
    tensor per millisecond, the loop of tests/test_gpu_backend_forms.py test_scale_factors_land_on_the_current_stream."""
    if SIDE["cycles_per_ms"] or SIDE["muls_per_ms"]:
        return
    torch.cuda.synchronize(dev)
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(1000)                                                        # (loads the kernel)
        torch.cuda.synchronize(dev)
        cycles = 1_000_000
        while True:
            ms = _timed_ms(torch, lambda: torch.cuda._sleep(cycles))
            if ms >= 5.0 or cycles >= 1 << 36:
                break
            cycles *= 8
        SIDE["cycles_per_ms"] = cycles / ms
    else:
        SIDE["busy"] = busy = torch.ones(1 << 26, dtype=torch.float32, device=dev)
        busy.mul_(1.0001)
        torch.cuda.synchronize(dev)
        SIDE["muls_per_ms"] = 50 / _timed_ms(torch, lambda: [busy.mul_(1.0001) for _ in range(50)])


def enqueue_delay(torch, dev, ms):
    """About `ms` milliseconds of work on the CURRENT stream that nothing else waits for."""
    _calibrate(torch, dev)
    if SIDE["cycles_per_ms"]:
        torch.cuda._sleep(int(ms * SIDE["cycles_per_ms"]))
    else:
        for _ in range(int(ms * SIDE["muls_per_ms"]) + 1):
            SIDE["busy"].mul_(1.0001)


def side_streams(torch, dev, n=1):
    """The process's n (1 or 2) side streams, made once.  A stream may share a hardware queue with the null stream and then runs
    behind it, so each is probed when it is made: a delay on the default stream, a one-element kernel on the candidate, its
    synchronisation, and the default stream must still be busy.  A candidate that fails is dropped for the next stream of torch's
    pool (32 streams handed out in turn), at most 8 draws in all: a draw that returns a stream already kept counts as one."""
    assert n in (1, 2)
    _calibrate(torch, dev)
    default = torch.cuda.default_stream(dev)
    while len(SIDE["streams"]) < n:
        if SIDE["tried"] >= 8:
            raise SideStreamViolation("no stream independent of the default stream among the first 8 of torch's pool: each ran behind "
                                      "a delay enqueued on the default stream (do they all share its hardware queue?)")
        SIDE["tried"] += 1
        cand = torch.cuda.Stream(device=dev)
        if any(cand.cuda_stream == s.cuda_stream for s in SIDE["streams"]):
            continue
        one = torch.zeros(1, device=dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(default):
            enqueue_delay(torch, dev, MIN_DELAY_MS)
        with torch.cuda.stream(cand):
            one.add_(1.0)
        cand.synchronize()
        independent = default.query() is False
        torch.cuda.synchronize(dev)
        if independent and float(one) == 1.0:
            SIDE["streams"].append(cand)
    return SIDE["streams"][:n]


def delay_for(plain_ms, what=""):
    """The delay in front of a case: 10 times the host wall time of its default-stream run (enqueue to synchronize; the factor covers
    host jitter and a stream's first use), at least 20 ms.  More than 2 s: the case is too large for a side-stream run."""
    ms = max(MIN_DELAY_MS, DELAY_FACTOR * plain_ms)
    if ms > MAX_DELAY_MS:
        raise SideStreamViolation("%s: its default-stream run took %.0f ms on the host, so its side-stream run would need a delay of "
                                  "%.0f ms: shrink the case (limit %.0f ms)" % (what or "the call", plain_ms, ms, MAX_DELAY_MS))
    SIDE["runs"] += 1
    return ms


def side_stream_run(bufs, invoke, device, what, plain_out, plain_ms):
    """The fourth run of guarded_runs: `invoke` on a variant-B arena inside torch.cuda.stream(side), the default stream busy."""
    import torch
    dev = torch.device(device)
    side, = side_streams(torch, dev, 1)
    default = torch.cuda.default_stream(dev)
    names = [n for n, b in bufs.items() if b.role == "out"]
    ms = delay_for(plain_ms, what)
    arena = GuardedArena(bufs, "B", dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(default):
        enqueue_delay(torch, dev, ms)
    with torch.cuda.stream(side):
        invoke(arena)
        side.synchronize()
        r1 = {n: arena.read(n) for n in names}                                         # (copied on `side` as well)
    still_busy = default.query() is False
    torch.cuda.synchronize(dev)
    r2 = {n: arena.read(n) for n in names}
    arena.assert_intact("%s (side stream)" % (what or "the call"))
    judge_side_run(r1, r2, plain_out, still_busy, "%s (side stream)" % (what or "the call"))


def _host_copy(torch, x):
    """A tensor, or a dict / list / tuple of tensors, host values and None -> the same with every tensor as a numpy array (its
    bits: bf16 and bool through integers), copied on the current stream."""
    if isinstance(x, dict):
        return {k: _host_copy(torch, v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_host_copy(torch, v) for v in x]
    if isinstance(x, torch.Tensor):
        if x.dtype == torch.bfloat16:
            x = x.view(torch.int16)
        return x.cpu().numpy().copy()
    return x


def _flatten(x, prefix, into):
    if isinstance(x, dict):
        for k, v in x.items():
            _flatten(v, "%s.%s" % (prefix, k) if prefix else str(k), into)
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            _flatten(v, "%s[%d]" % (prefix, i), into)
    elif x is not None:
        into[prefix or "result"] = np.asarray(x)
    return into


def _spoil(torch, x):
    """Overwrite every tensor of a result (or of a plan's scratch) so that neither it nor the allocator's next block holds a right answer."""
    if isinstance(x, dict):
        x = list(x.values())
    if isinstance(x, (list, tuple)):
        for v in x:
            _spoil(torch, v)
    elif isinstance(x, torch.Tensor) and x.numel():
        # (bytes -- a workspace -- get the arena's poison B, which every guarded entry point has run on; other integers are outputs only)
        x.fill_(float("nan") if x.dtype.is_floating_point else (False if x.dtype == torch.bool else 1 if x.dtype == torch.uint8 else 85))


def side_stream_call(fn, device, what, explicit=False, scratch=(), restore=None):
    """The same protocol one level up, for a route of the package: fn(stream) returns its results (tensors, or a dict / list of
    tensors and host values).  The reference is fn(None) on the default stream, compared bit for bit.

    scratch: tensors that outlive a call and that the call writes before it reads them -- a plan's intermediates, its workspace.  They
    are overwritten between the reference run and the side run together with the reference's outputs: otherwise they would still
    hold the reference run's (equal) values, and a kernel or copy that fills them on the wrong queue could not be seen.  restore: called
    behind that on the default stream, for what a plan wrote into its scratch when it was built and never writes again.

    explicit=False, the current-stream form: fn(None) runs inside torch.cuda.stream(side).
    explicit=True: fn(side) runs with the busy default stream current; only the reads are issued inside torch.cuda.stream(side).
    Returns the reference's host arrays (flattened: name -> numpy array)."""
    import time
    import torch
    dev = torch.device(device)
    side, = side_streams(torch, dev, 1)
    default = torch.cuda.default_stream(dev)
    _spoil(torch, fn(None))                     # (untimed: the first call of a route loads kernels and uploads what it keeps resident)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    ref_dev = fn(None)
    torch.cuda.synchronize(dev)
    ms = delay_for((time.perf_counter() - t0) * 1e3, what)
    plain = _flatten(_host_copy(torch, ref_dev), "", {})
    _spoil(torch, ref_dev)                      # outputs that persist (a plan's) must be produced again; freed ones hold no right answer
    _spoil(torch, list(scratch))
    if restore is not None:
        restore()
    del ref_dev
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(default):
        enqueue_delay(torch, dev, ms)
    if explicit:
        got = fn(side)
        side.synchronize()
        with torch.cuda.stream(side):
            r1 = _flatten(_host_copy(torch, got), "", {})
    else:
        with torch.cuda.stream(side):
            got = fn(None)
            side.synchronize()
            r1 = _flatten(_host_copy(torch, got), "", {})
    still_busy = default.query() is False
    torch.cuda.synchronize(dev)
    r2 = _flatten(_host_copy(torch, got), "", {})
    _spoil(torch, got)
    torch.cuda.synchronize(dev)
    assert set(r1) == set(plain) == set(r2), (what, sorted(plain), sorted(r1))
    judge_side_run(r1, r2, plain, still_busy, "%s (%s)" % (what, "stream=side" if explicit else "side stream current"))
    return plain


def guarded_runs(bufs, invoke, device="cpu", what="", plain=False, side_stream=True):
    """Run `invoke(arena)` on a variant-A and a variant-B arena.  Checks (a) every band intact after each run and (b) every
    output bit-identical between the two; with plain=True also on PlainBuffers, whose outputs must carry the same bits.  On a GPU
    and with side_stream=True a fourth run follows (side_stream_run): the call on a side stream while the default stream is busy,
    against the PlainBuffers run (made for it where plain=False).  Returns dict name -> numpy array of the outputs (role "out") for
    the caller's comparison with the reference, check (c)."""
    import time
    on_gpu = str(device).startswith("cuda")
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
    side_stream = side_stream and on_gpu
    if plain or side_stream:
        pb = PlainBuffers(bufs, device)
        pb.assert_intact()                                       # (the copies in are done: the time below is the call's own)
        t0 = time.perf_counter()
        invoke(pb)
        pb.assert_intact()
        plain_ms = (time.perf_counter() - t0) * 1e3
        plain_out = {n: pb.read(n) for n in res["A"]}
        for n in res["A"] if plain else ():
            got = plain_out[n]
            if not same_bits(res["A"][n], got):
                d = np.flatnonzero(res["A"][n].reshape(-1).view(np.uint8) != got.reshape(-1).view(np.uint8))
                raise GuardViolation("%s: output `%s` at the documented minimum alignment differs from the call on ordinary tensors, "
                                     "first at element %d" % (what or "the call", n, int(d[0]) // bufs[n].np.itemsize))
    if side_stream:
        side_stream_run(bufs, invoke, device, what, plain_out, plain_ms)
    return res["A"]
