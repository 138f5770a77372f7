"""A queued launch keeps its cached tables across streams ("Across streams").

Every launch that reads a table cached in the context ends with note_launch(stream) (an event on its stream); every place that replaces such
a table calls drain_launch_streams() first (waits for those events) and then uploads into the same buffer, in place.  Nothing but that
protocol keeps a launch queued on one stream from reading a table a later call on another stream has rewritten, and the rest of the suite
never holds a stream busy while it changes a key.  Here each reader of each table is queued on stream A behind a torch.cuda._sleep, the
table is replaced from another stream (a second torch stream, and the context's own), and the replacing call must return only once the held
launch has finished; both outputs must be the library's own undisturbed outputs bit for bit (the feature files pin those to their numpy
restatements).  One control per table repeats the scenario with a cache hit in place of the replacement: that call must return, and finish
on the device, while stream A is still held.

In every case the second table is no larger than the first, so DeviceBuffer::reserve keeps the buffer and no hipFree synchronises the device
on the protocol's behalf: a broken protocol shows as a wrong pixel, never as a read of freed memory.  For the same reason no case frees,
unbinds or destroys under a queued launch."""
import time

import numpy as np
import pytest

from test_gpu_mandel_equalise import six_views
import mandel_perturb_deep_ref as D
import mandel_perturb_ref as R

pytestmark = pytest.mark.gpu

W, H, M = 48, 32, 200
K1 = (0.1, 0.7, 0.6, 0.0)
K2 = (0.6, 0.1, 0.7, 0.0)
HOLD_FLOOR_MS, HOLD_FACTOR = 20.0, 20.0      # hold = max(20 ms, 20 x the replacing call's host time): margin for host jitter
PROBE_MS = 5.0
MAP1 = (np.arange(M + 1, dtype=np.uint32) * 7) % (M + 1)
MAP2 = (M - np.arange(M + 1)).astype(np.uint32)
QMAP1 = np.arange(M + 1, dtype=np.uint32) * 256
QMAP2 = ((np.arange(M + 1, dtype=np.uint64) ** 2 // M) * 256).astype(np.uint32)
LEVELS = 255
OTHERS = ["stream", "context"]               # the replacing call's stream: a second torch stream, the context's own (stream=0)


def raw(t):
    return t.cpu().numpy().view(np.uint32)


class Call:
    """One library call into a fresh output: run(out, stream, returned) issues it on `stream` (0: the context's own) and calls returned()
    as soon as the call that may replace a table has come back; prepare() (optional) restores what the call's key stands on."""

    def __init__(self, shape, fn, int32=False, prepare=None, run=None):
        self.shape, self.int32, self.prepare = shape, int32, prepare or (lambda: None)
        self.run = run or (lambda out, stream, returned: (fn(out.data_ptr(), stream), returned()))

    def alloc(self, torch):
        return torch.zeros(self.shape, dtype=torch.int32 if self.int32 else torch.float32, device="cuda")


class Rig:
    """The module's own context, its calibration, three streams on separate hardware queues and the device planes the readers take."""

    def __init__(self, B):
        import torch
        self.B, self.torch = B, torch
        self.ctx = B.Context(0)
        self.t2 = {}
        self.keep = []
        self.calibrate()
        self.planes()
        self.orbits = {}
        self.bound = None
        self.pick_streams()

    # ---- the hold -------------------------------------------------------------------------------------------------------------------
    def calibrate(self):
        torch = self.torch
        torch.cuda._sleep(1_000_000)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 20_000_000
        e0.record()
        torch.cuda._sleep(n)
        e1.record()
        torch.cuda.synchronize()
        self.cycles_per_ms = n / e0.elapsed_time(e1)
        print(f"\n[stream tables] torch.cuda._sleep: {self.cycles_per_ms:.0f} cycles per millisecond")

    def hold(self, stream, ms):
        with self.torch.cuda.stream(stream):
            self.torch.cuda._sleep(int(ms * self.cycles_per_ms))

    def idle(self):
        self.torch.cuda.synchronize()
        self.ctx.synchronize()

    # ---- streams ----------------------------------------------------------------------------------------------------------------------
    def shares_queue(self, holder, poke):
        """True when work issued by poke() (which waits for it) cannot finish while `holder` is held: the two share a hardware queue, and
        an upload from the one would wait behind the hold of the other whatever the protocol does."""
        self.idle()
        self.hold(holder, PROBE_MS)
        poke()
        shared = holder.query()
        holder.synchronize()
        return shared

    def pick_streams(self):
        torch, ctx, B = self.torch, self.ctx, self.B
        scratch = torch.zeros(64, dtype=torch.int32, device="cuda")
        tiny = torch.zeros((8, 8), dtype=torch.int32, device="cuda")
        p8 = B.mandelbrot_params(8, 8, max_iter=16)

        def poke_stream(s):
            def poke():
                with torch.cuda.stream(s):
                    scratch.add_(1)
                s.synchronize()
            return poke

        def poke_context():
            ctx.mandelbrot_device(p8, 0, tiny.data_ptr())
            ctx.synchronize()

        cands = [torch.cuda.Stream() for _ in range(8)]
        for s in cands:
            poke_stream(s)()
        poke_context()
        for a in cands:
            if self.shares_queue(a, poke_context):
                continue
            free = [s for s in cands if s is not a and not self.shares_queue(a, poke_stream(s))]
            if len(free) >= 2:
                self.A, self.S2, self.S3 = a, free[0], free[1]
                return
        pytest.fail("no torch stream whose hold leaves the context's stream and two further torch streams running: the streams share "
                    "hardware queues, and no case of this file could tell a missing drain from a queue's own order")

    # ---- inputs -------------------------------------------------------------------------------------------------------------------------
    def P(self, w=W, h=H, **kw):
        kw.setdefault("max_iter", M)
        return self.B.mandelbrot_params(w, h, **kw)

    def planes(self):
        torch, ctx, B = self.torch, self.ctx, self.B
        z32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")   # noqa: E731
        self.counts32, self.counts16 = z32(H, W), torch.zeros((H, W), dtype=torch.int16, device="cuda")
        self.deep32, self.smoothq, self.deepq = z32(H, W), z32(H, W), z32(H, W)
        self.samples32, self.ssmooth = z32(2 * H, 2 * W), z32(2 * H, 2 * W)
        torch.cuda.synchronize()
        half = dict(scale=(1.17, 1.17))
        SM = B.MANDEL_COLOUR_SMOOTH
        ctx.mandelbrot_device(self.P(), 0, self.counts32.data_ptr())
        ctx.mandelbrot_device(self.P(flags=B.MANDEL_ITERS_U16), 0, self.counts16.data_ptr())
        ctx.mandelbrot_device(self.P(**half), 0, self.deep32.data_ptr())
        ctx.mandelbrot_smooth_device(self.P(flags=SM), 0, 0, self.smoothq.data_ptr())
        ctx.mandelbrot_smooth_device(self.P(flags=SM, **half), 0, 0, self.deepq.data_ptr())
        ctx.mandelbrot_device(B.supersample_params(self.P(supersample=2)), 0, self.samples32.data_ptr())
        ctx.mandelbrot_smooth_device(B.supersample_params(self.P(flags=SM, supersample=2, smooth_samples=True)), 0, 0, self.ssmooth.data_ptr())
        # the exchange's tiles: two ranks' interleaved 16-bit counts, laid out as a gather leaves them (test_gpu_multi.py)
        self.blk, self.n_tiles = B.lib().mc_row_block(), 2
        self.padded = len([r for r in range(H) if (r // self.blk) % self.n_tiles == 0])
        self.tiles = torch.zeros((self.n_tiles, self.padded, W, 2), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for rank in range(self.n_tiles):
            p = self.P(row_begin=rank * self.blk, row_end=H, row_block=self.blk, row_stride=self.n_tiles * self.blk, flags=B.MANDEL_ITERS_U16)
            ctx.mandelbrot_device(p, 0, self.tiles[rank].data_ptr())
        rng = np.random.default_rng(48)
        self.density = [torch.from_numpy(rng.integers(0, 2 * LEVELS + 2, (H, W)).astype(np.uint32).view(np.int32)).cuda() for _ in range(3)]
        self.tone1 = [B.buddhabrot_sqrt_map(LEVELS), rng.integers(0, LEVELS + 1, LEVELS + 1).astype(np.uint32), np.arange(LEVELS + 1, dtype=np.uint32)]
        self.tone2 = [self.tone1[2], self.tone1[0], self.tone1[1]]
        self.scene1 = B.default_scene()
        spheres2 = self.scene1[1].copy()
        spheres2[8:11] = (0.5, 0.9, 0.3)             # the mirror sphere's colour
        self.scene2 = (self.scene1[0], spheres2)
        self.pixel_list = torch.arange(W * H, dtype=torch.int32, device="cuda")
        self.idle()
        assert len(np.unique(raw(self.counts32))) >= 10 and len(np.unique(raw(self.smoothq))) >= 10

    # ---- orbits -------------------------------------------------------------------------------------------------------------------------
    def orbit(self, name):
        """The four orbits of the perturbation cases, made once: "k4" and "k4b" (its centre 1e-21 further: the same length, no more BLA
        entries), both with the BLA table; "m33" and "m33b" (the deep view's centre 5e-1002 and 7e-1002 further), both with the deep one.
        The two of a pair carry the same tables, so that binding the one after the other releases nothing."""
        if name in self.orbits:
            return self.orbits[name]
        from decimal import Decimal, getcontext
        getcontext().prec = 1200
        B = self.B
        K4 = R.DEEP_CENTRE
        c33, m33, e33 = D.view(D.M33, "1e-1000")
        if name in ("k4", "k4b"):
            cx = K4[0] if name == "k4" else str(Decimal(K4[0]) + Decimal("1e-21"))
            o = B.Orbit(cx, K4[1], 1e-20, 1e-20, 20000)
            o.entries = o.bla()[1]
        else:
            cx = str(Decimal(c33[0]) + Decimal("5e-1002" if name == "m33" else "7e-1002"))
            o = B.Orbit(cx, c33[1], m33[0], m33[1], 6000, e33)
            o.entries = o.bla_deep()[1]
        self.orbits[name] = o
        return o

    def bind(self, name):
        """At idle only: binds the named orbit unless it is the bound one already."""
        if self.bound != name:
            self.idle()
            self.ctx.bind_mandelbrot_orbit(self.orbit(name))
            self.bound = name

    def close(self):
        self.idle()
        if self.bound is not None:
            self.ctx.bind_mandelbrot_orbit(None)
        for o in self.orbits.values():
            o.close()
        self.ctx.close()
        if self.t2:
            worst = max(self.t2, key=self.t2.get)
            print(f"\n[stream tables] {self.cycles_per_ms:.0f} cycles per millisecond; largest t2 {1e3 * self.t2[worst]:.3f} ms ({worst})")


@pytest.fixture(scope="module")
def rig(B):
    r = Rig(B)
    yield r
    r.close()


# ---- the scenario ----------------------------------------------------------------------------------------------------------------------
def alone(rig, call):
    """The call on an idle context, on the context's stream: (its output, its host time)."""
    out = call.alloc(rig.torch)
    rig.idle()
    t0 = time.perf_counter()
    call.run(out, 0, lambda: None)
    t = time.perf_counter() - t0
    rig.idle()
    return raw(out), t


def scenario(rig, name, read, replace, other, between=None, control=False):
    """Steps 1 to 7 of the protocol's one scenario.  control: `replace` carries the reader's own key (a cache hit), and the window must
    still be open when it has returned and finished.  between(A): further work issued while A is held, before the replacing call."""
    torch, A = rig.torch, rig.A
    other_stream = {"stream": rig.S2, "third": rig.S3, "context": None}[other]
    handle = other_stream.cuda_stream if other_stream is not None else 0
    # 1. undisturbed outputs, the replacing call's host time, K1's table the cached one
    read.prepare()
    want1, _ = alone(rig, read)
    want2, _ = alone(rig, replace)                     # (first use: the runtime may load a kernel here; not the call that is timed)
    read.prepare()
    assert np.array_equal(alone(rig, read)[0], want1)
    again2, t2 = alone(rig, replace)                   # K1's table is the cached one: this call replaces it, as step 4's will
    assert np.array_equal(again2, want2)
    read.prepare()
    assert np.array_equal(alone(rig, read)[0], want1)  # primed: step 2 is a cache hit and synchronises nothing
    rig.t2[name] = t2
    hold_ms = max(HOLD_FLOOR_MS, HOLD_FACTOR * 1e3 * t2)
    print(f"[stream tables] {name}: t2 {1e3 * t2:.3f} ms, hold {hold_ms:.1f} ms")
    out1, out2 = read.alloc(torch), replace.alloc(torch)
    rig.idle()
    seen = {}
    try:
        # 2. the reader, queued behind the hold
        rig.hold(A, hold_ms)
        read.run(out1, A.cuda_stream, lambda: None)
        seen["queued"] = not A.query()                 # 3. the window is open
        if between:
            between(A, seen)
        # 4. the other call, from another stream; 5. what stream A says the moment it has returned
        replace.run(out2, handle, lambda: seen.__setitem__("drained", A.query()))
        if control and other_stream is not None:
            other_stream.synchronize()
            seen["hit finished under the hold"] = not A.query()
    finally:
        rig.idle()
    assert seen["queued"], "step 3: the held launch had finished before the second call was issued (the hold was too short)"
    assert seen.get("between", True), "the launch run to completion on a second stream did not finish under the hold"
    if control:
        assert not seen["drained"], "control: a cache hit waited for the held launch (or the hold did not outlast the call)"
        assert seen.get("hit finished under the hold", True), "control: the hit's launch could not finish under the hold: the streams share a queue"
        assert np.array_equal(raw(out1), want1) and np.array_equal(raw(out2), want1)
    else:
        assert not np.array_equal(want1, want2), "the case cannot tell the two tables apart"
        wrong = []                                     # (steps 5 and 6 reported together: a missing drain names its wrong pixels too)
        if not seen["drained"]:
            wrong.append("step 5: the replacing call returned while the held launch was still queued: no drain")
        # 6. both images are their own
        bad1, bad2 = int((raw(out1) != want1).sum()), int((raw(out2) != want2).sum())
        if bad1:
            wrong.append(f"step 6: the held launch read a replaced table ({bad1} of {want1.size} words differ)")
        if bad2:
            wrong.append(f"step 6: the replacing call's output differs ({bad2} of {want2.size} words)")
        assert not wrong, "; ".join(wrong)
    # 7. the key followed the table
    read.prepare()
    assert np.array_equal(alone(rig, read)[0], want1), "step 7"


# ---- the calls -------------------------------------------------------------------------------------------------------------------------
def lut_readers(rig):
    """Every _device_async reader of the colour table, at (max_iter M, k_color K1)."""
    B, ctx, P = rig.B, rig.ctx, rig.P
    SM, SQ, DI = B.MANDEL_COLOUR_SMOOTH, B.MANDEL_COLOUR_SMOOTH_EQUALISED, B.MANDEL_COLOUR_DISTANCE
    rgba = (H, W, 4)
    c32, d32, sq, dq = (t.data_ptr() for t in (rig.counts32, rig.deep32, rig.smoothq, rig.deepq))
    AREA = B.ZOOM_FILTER_AREA
    return {
        "render": Call(rgba, lambda o, s: ctx.mandelbrot_device(P(), o, 0, s)),
        "smooth": Call(rgba, lambda o, s: ctx.mandelbrot_smooth_device(P(flags=SM), o, 0, 0, s)),
        "distance": Call(rgba, lambda o, s: ctx.mandelbrot_distance_device(P(flags=DI), sq, 1.0, 0, o, s)),
        "resolve": Call(rgba, lambda o, s: ctx.mandelbrot_resolve_device(P(supersample=2), rig.samples32.data_ptr(), 4, None, o, s)),
        "resolve-smooth": Call(rgba, lambda o, s: ctx.mandelbrot_resolve_smooth_device(P(flags=SM, supersample=2, smooth_samples=True),
                                                                                       rig.ssmooth.data_ptr(), None, o, s)),
        "smooth-remap": Call(rgba, lambda o, s: ctx.mandelbrot_smooth_remap_device(P(flags=SQ), sq, QMAP1, 0, o, s)),
        "zoom-plain": Call(rgba, lambda o, s: ctx.zoom_compose_counts_device(P(), c32, d32, None, 0.75, o, 0, s)),
        "zoom-smooth": Call(rgba, lambda o, s: ctx.zoom_compose_counts_device(P(flags=SM), sq, dq, None, 0.75, o, 0, s)),
        "zoom-plain-area": Call(rgba, lambda o, s: ctx.zoom_compose_counts_filtered_device(P(), c32, d32, None, 0.75, AREA, o, 0, s)),
        "zoom-smooth-area": Call(rgba, lambda o, s: ctx.zoom_compose_counts_filtered_device(P(flags=SM), sq, dq, None, 0.75, AREA, o, 0, s)),
        "assemble": Call(rgba, lambda o, s: ctx.mandelbrot_assemble_device(P(), rig.tiles.data_ptr(), 2, rig.n_tiles, rig.blk, rig.padded, o, 0, s)),
    }


LUT_READERS = ["render", "smooth", "distance", "resolve", "resolve-smooth", "smooth-remap", "zoom-plain", "zoom-smooth", "zoom-plain-area",
               "zoom-smooth-area", "assemble"]


def lut_replacement(rig, **kw):
    return Call((H, W, 4), lambda o, s: rig.ctx.mandelbrot_device(rig.P(**kw), o, 0, s))


def c_views(rig):
    """(params keywords, a second centre a few pixels away) of the three c-table precisions: the views of six_views."""
    views = {name: kw for name, kw, _ in six_views(rig.B)[:3]}
    k4 = views["ds"]["centre"]
    return {"f32": (dict(views["f32"], max_iter=M), (-0.6, 0.1)),
            "ds": (views["ds"], (k4[0] + 1e-7, k4[1])),
            "f64": (views["f64"], (k4[0] + 1e-13, k4[1]))}


def c_reader(rig, which):
    """mc_mandelbrot_render_device_async with the count plane only (no colour table is involved), or the smooth render's q plane only."""
    ctx, P = rig.ctx, rig.P
    if which == "smooth":
        return Call((H, W), lambda o, s: ctx.mandelbrot_smooth_device(P(flags=rig.B.MANDEL_COLOUR_SMOOTH), 0, 0, o, s), int32=True)
    kw = c_views(rig)[which][0]
    return Call((H, W), lambda o, s: ctx.mandelbrot_device(P(**kw), 0, o, s), int32=True)


def c_replacement(rig, which):
    kw, centre = c_views(rig)["f32" if which == "smooth" else which]
    return Call((H, W), lambda o, s: rig.ctx.mandelbrot_device(rig.P(**dict(kw, centre=centre)), 0, o, s), int32=True)


PERTURB = {  # reader: (orbit, the pair's second orbit, precision name, max_iter): the views of six_views, the deep one moved off its nucleus
    "perturb": ("k4", "k4b", "PRECISION_PERTURB", 20000),
    "perturb-bla": ("k4", "k4b", "PRECISION_PERTURB_BLA", 20000),
    "perturb-deep": ("m33", "m33b", "PRECISION_PERTURB", 6000),
    "perturb-bla-deep": ("m33", "m33b", "PRECISION_PERTURB_BLA_DEEP", 6000),
}


def perturb_params(rig, which, w=W, h=H):
    _, _, precision, max_iter = PERTURB[which]
    return rig.P(w, h, max_iter=max_iter, precision=getattr(rig.B, precision), centre=(0.0, 0.0), scale=(0.0, 0.0))


def perturb_reader(rig, which):
    first = PERTURB[which][0]
    return Call((H, W), lambda o, s: rig.ctx.mandelbrot_device(perturb_params(rig, which), 0, o, s), int32=True, prepare=lambda: rig.bind(first))


def perturb_smaller(rig, which):
    """Replacement (a): the same binding rendered at a smaller W x H, which rewrites the dc table in place."""
    return Call((24, 40), lambda o, s: rig.ctx.mandelbrot_device(perturb_params(rig, which, 40, 24), 0, o, s), int32=True)


def perturb_rebind(rig, which):
    """Replacement (b): the pair's second orbit bound (a host call: step 5 applies to its return), then a render that shows its image."""
    first, second = PERTURB[which][:2]
    o1, o2 = rig.orbit(first), rig.orbit(second)
    assert (o2.length, o2.max_iter) == (o1.length, o1.max_iter) and o2.entries <= o1.entries, "the second orbit's tables must fit the first's"
    assert not np.array_equal(o1.table(), o2.table())

    def run(out, stream, returned):
        rig.ctx.bind_mandelbrot_orbit(o2)
        rig.bound = second
        returned()
        rig.ctx.mandelbrot_device(perturb_params(rig, which), 0, out.data_ptr(), stream)

    return Call((H, W), None, int32=True, run=run)


def composed_readers(rig):
    B, ctx, P = rig.B, rig.ctx, rig.P
    rgba = (H, W, 4)
    return {
        "recolour-u16": Call(rgba, lambda o, s: ctx.mandelbrot_recolour_device(P(), rig.counts16.data_ptr(), 2, MAP1, o, s)),
        "recolour-u32": Call(rgba, lambda o, s: ctx.mandelbrot_recolour_device(P(), rig.counts32.data_ptr(), 4, MAP1, o, s)),
        "resolve-map": Call(rgba, lambda o, s: ctx.mandelbrot_resolve_device(P(supersample=2), rig.samples32.data_ptr(), 4, MAP1, o, s)),
        "zoom-equalised": Call(rgba, lambda o, s: ctx.zoom_compose_counts_device(P(flags=B.MANDEL_COLOUR_EQUALISED), rig.counts32.data_ptr(),
                                                                                 rig.deep32.data_ptr(), MAP1, 0.75, o, 0, s)),
    }


COMPOSED_READERS = ["recolour-u16", "recolour-u32", "resolve-map", "zoom-equalised"]


def composed_replacement(rig):
    return Call((H, W, 4), lambda o, s: rig.ctx.mandelbrot_recolour_device(rig.P(), rig.counts32.data_ptr(), 4, MAP2, o, s))


def pair_readers(rig):
    B, ctx, P = rig.B, rig.ctx, rig.P
    SQ = B.MANDEL_COLOUR_SMOOTH_EQUALISED
    rgba = (H, W, 4)
    sq, dq = rig.smoothq.data_ptr(), rig.deepq.data_ptr()
    return {
        "smooth-remap": Call(rgba, lambda o, s: ctx.mandelbrot_smooth_remap_device(P(flags=SQ), sq, QMAP1, 0, o, s)),
        "resolve-smooth-ranked": Call(rgba, lambda o, s: ctx.mandelbrot_resolve_smooth_device(P(flags=SQ, supersample=2, smooth_samples=True),
                                                                                              rig.ssmooth.data_ptr(), QMAP1, o, s)),
        "zoom-smooth-equalised": Call(rgba, lambda o, s: ctx.zoom_compose_counts_device(P(flags=SQ), sq, dq, QMAP1, 0.75, o, 0, s)),
    }


PAIR_READERS = ["smooth-remap", "resolve-smooth-ranked", "zoom-smooth-equalised"]


def pair_replacement(rig):
    """Another qmap through the remap stage's ranked plane alone: no colour table is touched."""
    SQ = rig.B.MANDEL_COLOUR_SMOOTH_EQUALISED
    return Call((H, W), lambda o, s: rig.ctx.mandelbrot_smooth_remap_device(rig.P(flags=SQ), rig.smoothq.data_ptr(), QMAP2, o, 0, s), int32=True)


def tonemap_call(rig, maps):
    d = [t.data_ptr() for t in rig.density]
    return Call((H, W, 4), lambda o, s: rig.ctx.buddhabrot_tonemap_device(W, H, d[0], d[1], d[2], LEVELS, maps[0], maps[1], maps[2], o, s))


def scene_params(rig):
    return rig.B.pathtrace_params(W, H, 4, math_mode=rig.B.PT_MATH_STRICT, flags=rig.B.PT_GENERIC_KERNEL)


def scene_call(rig, which, scene):
    ctx, p = rig.ctx, scene_params(rig)
    if which == "render":
        return Call((H, W, 4), lambda o, s: ctx.pathtrace_device(p, o, scene[0], scene[1], s))
    return Call((H, W, 4), lambda o, s: ctx.pathtrace_list_device(p, rig.pixel_list.data_ptr(), W * H, 1.0, o, scene[0], scene[1], s))


# ---- 1. the colour table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("other", OTHERS)
@pytest.mark.parametrize("reader", LUT_READERS)
def test_colour_table_replaced_under_a_queued_reader(rig, reader, other):
    scenario(rig, f"colour/{reader}/{other}", lut_readers(rig)[reader], lut_replacement(rig, k_color=K2), other)


@pytest.mark.parametrize("other", OTHERS)
def test_colour_table_replaced_by_one_of_a_smaller_max_iter(rig, other):
    scenario(rig, f"colour/smaller-max-iter/{other}", lut_readers(rig)["render"], lut_replacement(rig, max_iter=150), other)


def test_colour_table_control(rig):
    readers = lut_readers(rig)
    scenario(rig, "colour/control", readers["render"], readers["render"], "stream", control=True)


# ---- 2. the c table ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("other", OTHERS)
@pytest.mark.parametrize("reader", ["f32", "ds", "f64", "smooth"])
def test_c_table_replaced_under_a_queued_reader(rig, reader, other):
    scenario(rig, f"c/{reader}/{other}", c_reader(rig, reader), c_replacement(rig, reader), other)


@pytest.mark.parametrize("other", OTHERS)
def test_c_table_of_f64_replaced_by_an_f32_one(rig, other):
    """Half the bytes in the same buffer."""
    scenario(rig, f"c/f64-by-f32/{other}", c_reader(rig, "f64"), c_reader(rig, "f32"), other)


def test_c_table_control(rig):
    scenario(rig, "c/control", c_reader(rig, "ds"), c_reader(rig, "ds"), "stream", control=True)


# ---- 3. the dc table and the orbit binding -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("other", OTHERS)
@pytest.mark.parametrize("reader", list(PERTURB))
def test_dc_table_replaced_under_a_queued_reader(rig, reader, other):
    scenario(rig, f"dc/{reader}/{other}", perturb_reader(rig, reader), perturb_smaller(rig, reader), other)


@pytest.mark.parametrize("other", OTHERS)
@pytest.mark.parametrize("reader", list(PERTURB))
def test_orbit_rebound_under_a_queued_reader(rig, reader, other):
    scenario(rig, f"orbit/{reader}/{other}", perturb_reader(rig, reader), perturb_rebind(rig, reader), other)


def test_dc_table_control(rig):
    scenario(rig, "dc/control", perturb_reader(rig, "perturb-bla"), perturb_reader(rig, "perturb-bla"), "stream", control=True)


# ---- 4. the composed table -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("other", OTHERS)
@pytest.mark.parametrize("reader", COMPOSED_READERS)
def test_composed_table_replaced_under_a_queued_reader(rig, reader, other):
    scenario(rig, f"composed/{reader}/{other}", composed_readers(rig)[reader], composed_replacement(rig), other)


def test_composed_table_control(rig):
    readers = composed_readers(rig)
    scenario(rig, "composed/control", readers["recolour-u32"], readers["recolour-u32"], "stream", control=True)


# ---- 5. the pair table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("other", OTHERS)
@pytest.mark.parametrize("reader", PAIR_READERS)
def test_pair_table_replaced_under_a_queued_reader(rig, reader, other):
    scenario(rig, f"pairs/{reader}/{other}", pair_readers(rig)[reader], pair_replacement(rig), other)


def test_pair_table_control(rig):
    readers = pair_readers(rig)
    scenario(rig, "pairs/control", readers["smooth-remap"], readers["smooth-remap"], "stream", control=True)


# ---- 6. the Buddhabrot's tone-map table ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("other", OTHERS)
def test_tone_map_table_replaced_under_a_queued_reader(rig, other):
    scenario(rig, f"tonemap/{other}", tonemap_call(rig, rig.tone1), tonemap_call(rig, rig.tone2), other)


def test_tone_map_table_control(rig):
    scenario(rig, "tonemap/control", tonemap_call(rig, rig.tone1), tonemap_call(rig, rig.tone1), "stream", control=True)


# ---- 7. the generic path tracer's scene records ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("other", OTHERS)
@pytest.mark.parametrize("reader", ["render", "list"])
def test_scene_records_replaced_under_a_queued_reader(rig, reader, other):
    info = rig.B.pathtrace_select_kernel(scene_params(rig), *rig.scene1)
    assert info.kernel == rig.B.PT_KERNEL_GENERIC, "the generic kernel is the one that reads the cached records"
    scenario(rig, f"scene/{reader}/{other}", scene_call(rig, reader, rig.scene1), scene_call(rig, "render", rig.scene2), other)


def test_scene_records_control(rig):
    scenario(rig, "scene/control", scene_call(rig, "render", rig.scene1), scene_call(rig, "render", rig.scene1), "stream", control=True)


# ---- 8. all events, not the last one -----------------------------------------------------------------------------------------------------------
def test_drain_waits_for_every_stream_not_the_last_one(rig):
    """Stream A holds a queued reader; a second reader runs to completion on a second stream (its event is the last one recorded); the
    replacement comes from a third.  The drain must still wait for A."""
    readers = lut_readers(rig)
    second = readers["resolve"]
    extra = second.alloc(rig.torch)

    def between(A, seen):
        second.run(extra, rig.S2.cuda_stream, lambda: None)
        rig.S2.synchronize()
        seen["between"] = not A.query()

    scenario(rig, "colour/all-events", readers["render"], lut_replacement(rig, k_color=K2), "third", between=between)
