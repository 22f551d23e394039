"""The guarded arena's own teeth (tests/guarded_arena.py), on a CPU slab: stand-in "entry points" written in Python that
misbehave in the four ways the arena exists to catch, and one that does not.  A stand-in sees what a kernel sees: a base pointer
per argument (`arena.window(name, lo, hi)` is pointer arithmetic on it) and the sizes it was told."""
import numpy as np
import pytest

from guarded_arena import BAND, GuardViolation, GuardedArena, SideStreamViolation, guarded_runs, inp, judge_side_run, out, ws

N = 1000


def _bufs(n=N):
    rng = np.random.default_rng(5)
    return {"x": inp("f64", rng.uniform(1.0, 2.0, n)), "idx": inp("i32", rng.integers(0, n, n).astype(np.int32), index=(0, n - 1)),
            "flag": inp("u8", (rng.uniform(size=n) < 0.5).astype(np.uint8)), "scratch": ws(4 * n + 4, "i32", align=256),
            "y": out("f64", n), "total": out("f64", 1)}


def _correct(a, n=N):
    x, idx, flag = a.window("x"), a.window("idx").long(), a.window("flag")
    s = a.window("scratch")
    s[:n] = idx.int()                                            # (scratch is written before it is read)
    a.window("y")[:] = x[s[:n].long()] * (1 + flag.double())
    a.window("total")[0] = x.sum()


def _store_past_output(a, n=N):
    _correct(a, n)
    a.window("y", 0, n + 1)[n] = 3.0


def _store_before_output(a, n=N):
    _correct(a, n)
    a.window("y", -1, n)[0] = 3.0


def _sum_one_too_many(a, n=N):
    _correct(a, n)
    a.window("total")[0] = a.window("x", 0, n + 1).sum()


def _stale_scratch(a, n=N):
    _correct(a, n)
    a.window("y")[7] += a.window("scratch")[n].double()          # the word behind the part the call itself wrote


def test_correct_stand_in_passes_and_returns_its_outputs():
    b = _bufs()
    got = guarded_runs(b, _correct, what="correct", plain=False)
    x, idx, flag = b["x"].data, b["idx"].data, b["flag"].data
    assert np.array_equal(got["y"], x[idx] * (1 + flag)) and got["total"].shape == (1,)
    assert set(got) == {"y", "total"}


@pytest.mark.parametrize("fn, arg, side", [(_store_past_output, "y", "rear"), (_store_before_output, "y", "front")])
def test_a_store_outside_an_output_is_reported_with_argument_side_and_offset(fn, arg, side):
    for variant in ("A", "B"):
        a = GuardedArena(_bufs(), variant)
        fn(a)
        v = a.violations()
        assert v == [(arg, side, 0)], v
    with pytest.raises(GuardViolation, match=r"%s band of `%s`, byte offset 0" % (side, arg)):
        guarded_runs(_bufs(), fn, what="stand-in")


def test_a_store_further_out_reports_its_byte_offset():
    a = GuardedArena(_bufs(), "A")
    _correct(a)
    a.window("total", 0, 4)[3] = 1.0                              # 16 bytes behind the one-element output
    assert a.violations() == [("total", "rear", 16)]


def test_an_over_read_that_reaches_an_output_is_an_a_b_difference():
    for variant in ("A", "B"):                                   # no band is written: check (a) alone does not see it
        a = GuardedArena(_bufs(), variant)
        _sum_one_too_many(a)
        assert a.violations() == []
    with pytest.raises(GuardViolation, match=r"output `total` depends on what lies around"):
        guarded_runs(_bufs(), _sum_one_too_many, what="stand-in")


def test_reliance_on_stale_scratch_is_an_a_b_difference():
    with pytest.raises(GuardViolation, match=r"output `y` depends on .* \(element 7\)"):
        guarded_runs(_bufs(), _stale_scratch, what="stand-in")


def test_placement_every_buffer_at_a_mod_2a_and_bands_of_64_kib():
    b = _bufs()
    b["g"] = inp("u32", np.arange(40, dtype=np.uint32), align=16)
    b["rec"] = ws(5120, align=256)
    b["h"] = inp("i16", np.arange(7, dtype=np.int16))
    b["bf"] = out("bf16", 3)
    b["w8"] = ws(24, align=8)
    for variant in ("A", "B"):
        a = GuardedArena(b, variant)
        want = {"x": 8, "idx": 4, "flag": 1, "scratch": 256, "y": 8, "total": 8, "g": 16, "rec": 256, "h": 2, "bf": 2, "w8": 8}
        for name, al in want.items():
            assert a.ptr(name) % (2 * al) == al, name
        assert a.ptr("flag") % 2 == 1
        assert a.ptr("missing") is None
        bands = {(n, s): (lo, hi) for lo, hi, n, s in a.bands}
        prev_end = 0
        for name, buf in b.items():
            (flo, fhi), (rlo, rhi) = bands[name, "front"], bands[name, "rear"]
            assert flo == prev_end and fhi == a.off[name] and fhi - flo >= BAND                  # front band up to the first byte
            assert rlo == a.off[name] + buf.nbytes and rhi - rlo >= BAND                        # rear band from the next byte
            prev_end = rhi
        assert bands["x", "front"][0] == 0 and prev_end == a.slab.numel()                        # the slab's ends are bands
        # a workspace holds exactly the declared bytes: the byte behind it is the first byte of its rear band
        assert bands["scratch", "rear"][0] - a.off["scratch"] == 4 * N + 4


def test_typed_poison_differs_everywhere_and_stays_in_domain():
    b = _bufs()
    b["g"] = inp("u32", np.arange(8, dtype=np.uint32), align=16)
    A, B = GuardedArena(b, "A"), GuardedArena(b, "B")
    n = BAND // 8
    xa, xb = A.window("x", -n, 0).numpy(), B.window("x", N, N + n).numpy()
    assert np.isnan(xa).all() and (xb == 1e300).all()
    ia, ib = A.window("idx", N, N + 64).numpy(), B.window("idx", -64, 0).numpy()
    assert (ia == 0).all() and (ib == N - 1).all()                                              # valid indices, both
    assert (A.window("flag", -64, 0).numpy() == 0).all() and (B.window("flag", -64, 0).numpy() == 1).all()
    assert (A.window("g", 8, 72).numpy() == 0).all() and (B.window("g", 8, 72).numpy() == -1).all()       # 0xFFFFFFFF
    assert np.isnan(A.read("y")).all() and (B.read("y") == 1e300).all()                         # outputs and scratch pre-filled
    assert (A.read("scratch") == 0).all() and (B.read("scratch") == 1 << 20).all()
    # every band byte-for-element different between the variants
    for (lo, hi, name, side) in A.bands:
        w = b[name].np.itemsize
        lo2 = lo + (A.off[name] - lo) % w
        ea = A.slab[lo2:lo2 + (hi - lo2) // w * w].numpy().view(b[name].np)
        off_b = B.off[name] + (lo2 - A.off[name])
        eb = B.slab[off_b:off_b + ea.nbytes].numpy().view(b[name].np)
        assert ea.size and not (ea.view("u%d" % w) == eb.view("u%d" % w)).any(), (name, side)


def test_a_float_pattern_for_an_index_argument_is_refused():
    idx = np.zeros(4, np.int32)
    with pytest.raises(ValueError, match="float pattern"):
        inp("i32", idx, index=(0, 3), poison=(np.nan, 1e300))
    with pytest.raises(ValueError, match="float pattern"):
        inp("i32", idx, index=(0, 3), poison=(0, 2.0))
    with pytest.raises(ValueError, match="float pattern"):
        inp("f64", idx.astype(np.float64), index=(0, 3))
    with pytest.raises(ValueError, match="outside the valid domain"):
        inp("i32", idx, index=(0, 3), poison=(0, 4))
    with pytest.raises(ValueError, match="must differ"):
        inp("i32", idx, index=(2, 2))
    assert inp("i64", idx.astype(np.int64), index=(0, 3)).poison == (0, 3)


def test_plain_buffers_run_the_same_call_and_a_difference_from_them_is_reported():
    got = guarded_runs(_bufs(), _correct, plain=True)
    assert got["y"].shape == (N,)

    def depends_on_alignment(a):
        _correct(a)
        a.window("y")[0] = float(a.ptr("x") % 16)                 # 8 in every arena, 0 on an ordinary allocation

    with pytest.raises(GuardViolation, match="differs from the call on ordinary tensors"):
        guarded_runs(_bufs(), depends_on_alignment, plain=True)


# ---- the side-stream verdict: a pure function of (R1, R2, plain, still_busy), here on what four stand-ins would leave behind ---------
def _readings(kind):
    """What the side-stream run of guarded_runs observes of a call that fills `y` (pre-filled with poison B, 1e300) and zeroes `n`."""
    plain = {"y": np.arange(1.0, 9.0), "n": np.zeros(3, np.int32)}
    r1, r2, busy = {k: v.copy() for k, v in plain.items()}, {k: v.copy() for k, v in plain.items()}, True
    if kind == "late producer":              # the kernel that writes y went to the default stream: R1 still holds the poison
        r1["y"][:] = 1e300
    elif kind == "late clobber":             # the memset of n went to the default stream and ran after the side stream's kernel
        plain["n"][:] = r1["n"][:] = [4, 0, 7]
    elif kind == "inconclusive":             # the call waited for the default stream: right values, nothing shown
        busy = False
    return r1, r2, plain, busy


def test_side_stream_verdict_passes_a_correct_call():
    assert judge_side_run(*_readings("correct"), what="stand-in") is None


@pytest.mark.parametrize("kind, detail", [("late producer", r"output `y` .* reading R1 differs .* first at element 0$"),
                                          ("late clobber", r"output `n` .* reading R2 differs .* first at element 0$"),
                                          ("inconclusive", r"the default stream was idle")])
def test_side_stream_verdict_names_what_went_wrong(kind, detail):
    with pytest.raises(SideStreamViolation, match=r"stand-in: %s: %s" % (kind, detail)):
        judge_side_run(*_readings(kind), what="stand-in")


def test_side_stream_verdict_reports_the_first_element_and_puts_inconclusive_first():
    r1, r2, plain, busy = _readings("correct")
    r2["y"][5] = np.nan                                          # one element, late
    with pytest.raises(SideStreamViolation, match=r"late clobber: output `y` .* first at element 5$"):
        judge_side_run(r1, r2, plain, busy)
    r1["y"][6] = -plain["y"][6]
    with pytest.raises(SideStreamViolation, match=r"late producer: output `y` .* first at element 6$"):
        judge_side_run(r1, r2, plain, busy)
    with pytest.raises(SideStreamViolation, match=r"inconclusive"):       # wrong values prove nothing about an idle default stream
        judge_side_run(r1, r2, plain, False)
    assert issubclass(SideStreamViolation, GuardViolation)
    zero, minus = {"y": np.array([0.0])}, {"y": np.array([-0.0])}         # bits, not values
    with pytest.raises(SideStreamViolation, match=r"late producer"):
        judge_side_run(minus, zero, zero, True)


def test_cpu_callers_get_no_side_stream_run():
    """device="cpu" (the helper's own tests, the `_host` twins): three runs as before, whatever side_stream says."""
    calls = []
    guarded_runs(_bufs(), lambda a: (calls.append(type(a).__name__), _correct(a)), plain=True, side_stream=True)
    assert calls == ["GuardedArena", "GuardedArena", "PlainBuffers"]
