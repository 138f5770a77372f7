"""Zoom sequences on the MI355X: the compose kernel alone on uploaded keyframes against tests/mandel_zoom_ref.py bit for bit (every shape
of the host test and one that crosses block boundaries in both axes, each output alone and both, deep absent), the sequence object against
the blocking render's own bits in every precision and colouring, every refusal, the timing record, the app."""
import os
import subprocess

import numpy as np
import pytest

import mandel_perturb_deep_ref as D
import mandel_perturb_ref as R
import mandel_zoom_ref as Z
from test_mandel_zoom_host import SHAPES as HOST_SHAPES, bits, keyframes, ratios

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "mandelbrot")
INVALID = 1
SHAPES = HOST_SHAPES + [(257, 130)]        # (W, H); the last: 5 blocks of 64 columns and 33 of 4 rows, both with a partial last block
K4 = R.DEEP_CENTRE
K4F = (float(K4[0]), float(K4[1]))
ZERO = dict(centre=(0.0, 0.0), scale=(0.0, 0.0))


class Stage:
    """mc_mandelbrot_zoom_compose_device_async on two uploaded keyframes.  Each output lies between two guard rows, which must come back
    untouched; an output that was not asked for must come back untouched as a whole."""

    def __init__(self, ctx, wide, deep):
        import torch
        self.torch, self.ctx = torch, ctx
        self.H, self.W = wide.shape[:2]
        self.d_wide = torch.from_numpy(np.array(wide, np.float32)).cuda()
        self.d_deep = torch.from_numpy(np.array(deep, np.float32)).cuda()

    def __call__(self, r, with_deep=True, want_rgba=True, want_rgba8=True):
        torch, H, W = self.torch, self.H, self.W
        d_f = torch.full((H + 2, W, 4), -7.0, dtype=torch.float32, device="cuda")
        d_8 = torch.full((H + 2, W, 4), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.ctx.zoom_compose_device(W, H, self.d_wide.data_ptr(), self.d_deep.data_ptr() if with_deep else 0, r,
                                     d_f[1:].data_ptr() if want_rgba else 0, d_8[1:].data_ptr() if want_rgba8 else 0)
        self.ctx.synchronize()
        f, b = d_f.cpu().numpy(), d_8.cpu().numpy()
        assert (f[0] == -7.0).all() and (f[-1] == -7.0).all() and (b[0] == 7).all() and (b[-1] == 7).all(), "a write outside the frame"
        if not want_rgba:
            assert (f == -7.0).all()
        if not want_rgba8:
            assert (b == 7).all()
        return (f[1:-1] if want_rgba else None), (b[1:-1] if want_rgba8 else None)


@pytest.mark.parametrize("W,H", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_stage_is_the_restatement(ctx, B, W, H):
    wide, deep = keyframes(W, H)
    stage = Stage(ctx, wide, deep)
    for r in ratios(B):
        for with_deep in (True, False):
            want, _ = Z.compose(wide, deep if with_deep else None, r)
            want8 = Z.rgba8(want)
            f, b = stage(r, with_deep)
            bad = (bits(f) != bits(want)).any(axis=-1)
            assert not bad.any(), (W, H, r, with_deep, int(bad.sum()), f[bad][:2], want[bad][:2])
            assert np.array_equal(b, want8), (W, H, r, with_deep)
            f, b = stage(r, with_deep, want_rgba8=False)
            assert b is None and np.array_equal(bits(f), bits(want)), (W, H, r, with_deep, "vec4 only")
            f, b = stage(r, with_deep, want_rgba=False)
            assert f is None and np.array_equal(b, want8), (W, H, r, with_deep, "RGBA8 only")
    assert np.array_equal(bits(stage(1.0, False)[0]), bits(wide))
    assert np.array_equal(bits(stage(0.5)[0]), bits(deep))


def refused(B, call, says=None):
    with pytest.raises(B.McError) as e:
        call()
    assert e.value.status == INVALID, e.value
    for s in ([says] if isinstance(says, str) else says or []):
        assert s in str(e.value), e.value


def test_stage_refusals(ctx, B):
    import torch
    W, H = 8, 8
    k = torch.zeros((3, H, W, 4), dtype=torch.float32, device="cuda")
    out8 = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    w, d, o = k[0].data_ptr(), k[1].data_ptr(), k[2].data_ptr()
    call = lambda *a, **kw: (lambda: ctx.zoom_compose_device(*a, **kw))
    refused(B, call(W, H, w + 4, d, 0.75, o), "aligned")
    refused(B, call(W, H, w, d + 8, 0.75, o), "aligned")
    refused(B, call(W, H, w, d, 0.75, o + 4), "aligned")
    refused(B, call(W, H, w, d, 0.75, 0, out8.data_ptr() + 2), "aligned")
    refused(B, call(W, H, w, d, 0.75, w), "overlaps")                     # in place
    refused(B, call(W, H, w, d, 0.75, d), "overlaps")
    refused(B, call(W, H, w, d, 0.75, w + 16 * W), "overlaps")            # one row further: still inside the wide keyframe
    refused(B, call(W, H, w, d, 0.75, 0, d + 16), "overlaps")
    refused(B, call(W, H, w, d, 0.75, o, o), "overlaps")                  # the two outputs on each other
    refused(B, call(W, H, 0, d, 0.75, o), "NULL")
    refused(B, call(W, H, w, d, 0.75), "at least one output")
    refused(B, call(0, H, w, d, 0.75, o), "above 0")
    refused(B, call(W, H, w, d, 0.4999, o), "outside [0.5, 1]")
    refused(B, call(W, H, w, d, float("nan"), o), "outside [0.5, 1]")
    ctx.zoom_compose_device(W, H, w, w, 1.0, o)                           # (an input may be both keyframes; nothing is written to it)
    ctx.synchronize()


# ---- the sequence object ----------------------------------------------------------------------------------------------------------------
def render(ctx, p):
    return ctx.mandelbrot(p, want_iters=False)[0]


def test_sequence_reference_view(ctx, B):
    W, H, Mv = 96, 64, 128
    ps = [B.mandelbrot_params(W, H, max_iter=Mv, scale=(s, s)) for s in (2.34, 1.17, 0.585)]
    before = render(ctx, ps[0])
    k = [render(ctx, p) for p in ps]
    r13 = B.zoom_ratio(1, 3)
    with ctx.zoom(W, H) as z:
        z.push(ps[0])
        kms, cms = ctx.last_timing()
        assert kms > 0 and cms == 0
        f, f8 = z.frame(1.0, want_rgba8=True)
        assert np.array_equal(bits(f), bits(k[0])), "one keyframe, r = 1: the blocking render's bits"
        assert np.array_equal(f8, ctx.convert_rgba8(k[0], 255.0))
        kms, cms = ctx.last_timing()
        assert kms > 0 and cms >= 0
        assert np.array_equal(bits(z.frame(r13)[0]), bits(Z.compose(k[0], None, r13)[0])), "one keyframe alone"
        z.push(ps[1])
        assert np.array_equal(bits(z.frame(0.5)[0]), bits(k[1])), "r = 0.5: the deeper keyframe's bits"
        for r in (r13, 1.0, B.zoom_ratio(2, 3)):
            want = Z.compose(k[0], k[1], r)[0]
            f, f8 = z.frame(r, want_rgba8=True)
            assert np.array_equal(bits(f), bits(want)), r
            assert np.array_equal(f8, Z.rgba8(want)), r
            assert np.array_equal(z.frame(r, want_rgba=False, want_rgba8=True)[1], f8), r
        # two keyframes held: a refused push (its own refusals, the blocking render's, the scale) leaves BOTH where they were
        bad = [B.mandelbrot_params(W, H, max_iter=Mv, scale=(0.585, 0.585), flags=B.MANDEL_COLOUR_SMOOTH, supersample=2),
               B.mandelbrot_params(W, H, max_iter=Mv, precision=B.PRECISION_PERTURB, **ZERO),
               B.mandelbrot_params(W, H, max_iter=Mv, scale=(0.585, 0.585), row_begin=8),
               B.mandelbrot_params(W, H, max_iter=Mv, scale=(0.6, 0.6))]
        for p in bad:
            refused(B, lambda: z.push(p))
            assert np.array_equal(bits(z.frame(r13)[0]), bits(Z.compose(k[0], k[1], r13)[0])), "a refused push left both keyframes"
        z.push(ps[2])                                                      # the slots rotate: wide = keyframe 1, deep = keyframe 2
        assert np.array_equal(bits(z.frame(0.5)[0]), bits(k[2]))
        assert np.array_equal(bits(z.frame(r13)[0]), bits(Z.compose(k[1], k[2], r13)[0]))
        assert not np.array_equal(bits(k[1]), bits(k[2]))
    after = render(ctx, ps[0])
    assert np.array_equal(bits(after), bits(before)), "a plain render on the same context afterwards is unchanged"


def orbit_pair(B, cx, cy, mx, my, e, Mv, tables):
    def make(ee):
        o = B.Orbit(cx, cy, mx, my, Mv, ee)
        for t in tables:
            getattr(o, t)()
        return o
    return lambda: make(e), lambda: make(e - 1)


def precision_pairs(B, Mv):
    """(name, (params keywords, orbit factory or None) for the wide and the deep keyframe) per precision."""
    c33, m33, e33 = D.view(D.M33, "1e-1000")
    sm, se = B.scale_from_text("1e-20")
    def words(prec, centre, s):
        return [(dict(max_iter=Mv, precision=prec, centre=centre, scale=(x, x)), None) for x in (s, s / 2)]
    def orbits(prec, cx, cy, m, e, tables=()):
        return [(dict(max_iter=Mv, precision=prec, **ZERO), mk) for mk in orbit_pair(B, cx, cy, m[0], m[1], e, Mv, tables)]
    return [("f32", words(B.PRECISION_F32, (-0.445, 0.0), 2.34)),
            ("ds", words(B.PRECISION_DS, K4F, 1e-6)),
            ("f64", words(B.PRECISION_F64, K4F, 1e-12)),
            ("perturb", orbits(B.PRECISION_PERTURB, K4[0], K4[1], (sm, sm), se)),
            ("perturb-bla", orbits(B.PRECISION_PERTURB_BLA, K4[0], K4[1], (sm, sm), se, ("bla",))),
            ("perturb-bla-deep", orbits(B.PRECISION_PERTURB_BLA_DEEP, c33[0], c33[1], m33, e33, ("bla_deep",))),
            ("deep-orbit", orbits(B.PRECISION_PERTURB, c33[0], c33[1], m33, e33)),
            ("f32-then-f64", [words(B.PRECISION_F32, (-0.445, 0.0), 2.34)[0], words(B.PRECISION_F64, (-0.445, 0.0), 2.34)[1]])]


@pytest.mark.parametrize("which", range(8), ids=["f32", "ds", "f64", "perturb", "perturb-bla", "perturb-bla-deep", "deep-orbit", "f32-then-f64"])
def test_pair_in_every_precision(ctx, B, which):
    W, H, Mv = 64, 48, 300
    name, pair = precision_pairs(B, Mv)[which]
    r = B.zoom_ratio(1, 2)
    held = []
    try:
        with ctx.zoom(W, H) as z:
            k = []
            for kw, make in pair:
                if make:
                    o = make()
                    held.append(o)
                    ctx.bind_mandelbrot_orbit(o)
                p = B.mandelbrot_params(W, H, **kw)
                k.append(render(ctx, p))
                z.push(p)
            if name == "deep-orbit" or name == "perturb-bla-deep":
                assert held[0].deep and held[1].deep and held[1].scale_exp2 == held[0].scale_exp2 - 1 < -960
            assert np.array_equal(bits(z.frame(0.5)[0]), bits(k[1])), name
            want = Z.compose(k[0], k[1], r)[0]
            f, f8 = z.frame(r, want_rgba8=True)
            assert np.array_equal(bits(f), bits(want)), name
            assert np.array_equal(f8, Z.rgba8(want)), name
    finally:
        ctx.bind_mandelbrot_orbit(None)
        for o in held:
            o.close()


@pytest.mark.parametrize("mode", ["smooth", "distance", "equalised", "supersample2", "adaptive4"])
def test_keyframe_in_every_colouring(ctx, B, mode):
    W, H, Mv = 96, 64, 128
    kw = dict(smooth=dict(flags=B.MANDEL_COLOUR_SMOOTH), distance=dict(flags=B.MANDEL_COLOUR_DISTANCE),
              equalised=dict(flags=B.MANDEL_COLOUR_EQUALISED), supersample2=dict(supersample=2),
              adaptive4=dict(supersample=4, adaptive=True))[mode]
    p = B.mandelbrot_params(W, H, max_iter=Mv, **kw)
    plain = render(ctx, B.mandelbrot_params(W, H, max_iter=Mv))
    want = render(ctx, p)
    assert not np.array_equal(bits(want), bits(plain)), mode
    with ctx.zoom(W, H) as z:
        z.push(p)
        kms, cms = ctx.last_timing()
        assert kms > 0 and cms == 0
        f, f8 = z.frame(1.0, want_rgba8=True)
        assert np.array_equal(bits(f), bits(want)), mode
        assert np.array_equal(f8, ctx.mandelbrot_rgba8(p)), mode
    assert np.array_equal(bits(render(ctx, p)), bits(want)), mode


def test_sequence_refusals(ctx, B):
    W, H, Mv = 96, 64, 128
    P = lambda **kw: B.mandelbrot_params(W, H, max_iter=Mv, **kw)
    with ctx.zoom(W, H) as z:
        refused(B, lambda: z.frame(1.0), "no keyframe has been pushed")
        refused(B, lambda: z.push(B.mandelbrot_params(W, H + 1, max_iter=Mv)), ["96 x 65", "96 x 64"])
        refused(B, lambda: z.push(B.mandelbrot_params(W // 2, H, max_iter=Mv)), "48 x 64")
        refused(B, lambda: z.push(P(row_begin=0, row_end=8)), "whole image")
        refused(B, lambda: z.push(P(row_begin=8)), "whole image")
        refused(B, lambda: z.push(P(row_block=8, row_stride=16)), "whole image")
        refused(B, lambda: z.push(P(flags=B.MANDEL_ITERS_U16)), "MC_MANDEL_ITERS_U16")
        # the blocking render's own refusals pass through
        refused(B, lambda: z.push(P(flags=B.MANDEL_COLOUR_SMOOTH, supersample=2)), "MC_MANDEL_COLOUR_SMOOTH does not combine")
        refused(B, lambda: z.push(P(adaptive=True)), "MC_MANDEL_SUPERSAMPLE_ADAPTIVE")
        refused(B, lambda: z.push(P(precision=B.PRECISION_PERTURB, **ZERO)), "no orbit bound")
        refused(B, lambda: z.frame(1.0), "no keyframe has been pushed")    # (none of those left a keyframe behind)
        z.push(P(scale=(2.34, 2.34)))
        for s in ((2.34, 2.34), (1.17, 2.34), (1.17, 1.1700001), (1.0, 1.0), (4.68, 4.68)):
            refused(B, lambda: z.push(P(scale=s)), ["not exactly half", "2^2", "the centre is the caller's"])
        k0 = render(ctx, P(scale=(2.34, 2.34)))
        assert np.array_equal(bits(z.frame(1.0)[0]), bits(k0)), "a refused push leaves the sequence as it was"
        refused(B, lambda: z.frame(1.5), "outside [0.5, 1]")
        refused(B, lambda: z.frame(0.75, want_rgba=False, want_rgba8=False), "at least one output")
        # the orbit form: the bound orbit's scale against the previous keyframe's words, and against a previous orbit's
        sm, se = B.scale_from_text("1e-20")
        with B.Orbit(K4[0], K4[1], sm, sm, Mv, se) as o:
            ctx.bind_mandelbrot_orbit(o)
            try:
                refused(B, lambda: z.push(P(precision=B.PRECISION_PERTURB, **ZERO)), ["not exactly half", f"2^{se}"])
            finally:
                ctx.bind_mandelbrot_orbit(None)
    with ctx.zoom(W, H) as z:
        sm, se = B.scale_from_text("1e-20")
        try:
            with B.Orbit(K4[0], K4[1], sm, sm, Mv, se) as o:
                ctx.bind_mandelbrot_orbit(o)
                z.push(P(precision=B.PRECISION_PERTURB, **ZERO))
                refused(B, lambda: z.push(P(precision=B.PRECISION_PERTURB, **ZERO)), ["not exactly half", f"2^{se}"])   # the same orbit again
            with B.Orbit(K4[0], K4[1], sm, sm, Mv, se - 2) as o:
                ctx.bind_mandelbrot_orbit(o)
                refused(B, lambda: z.push(P(precision=B.PRECISION_PERTURB, **ZERO)), ["not exactly half", f"2^{se - 2}"])
            with B.Orbit(K4[0], K4[1], sm, sm, Mv, se - 1) as o:
                ctx.bind_mandelbrot_orbit(o)
                z.push(P(precision=B.PRECISION_PERTURB, **ZERO))
        finally:
            ctx.bind_mandelbrot_orbit(None)
    with pytest.raises(B.McError):
        B.Zoom(ctx, 0, 8)


# ---- the app --------------------------------------------------------------------------------------------------------------------------------
def run_app(tmp_path, args):
    return subprocess.run([APP, "--quiet"] + [str(a) for a in args], capture_output=True, text=True, cwd=tmp_path, timeout=180)


def binding_sequence(ctx, B, W, H, K, F, key):
    """The K * F + 1 frames (float32, RGBA8) of the app's scheme through the binding; key(j) pushes nothing itself: it returns keyframe
    j's params after binding whatever they need."""
    frames = []
    with ctx.zoom(W, H) as z:
        for j in range(K + 1):
            z.push(key(j))
            for r in ([1.0] if j == 0 else [B.zoom_ratio(s, F) for s in range(1, F + 1)]):
                frames.append(z.frame(r, want_rgba8=True))
    return frames


@pytest.mark.parametrize("extra", [[], ["--gpu-postprocess"]], ids=["host-convert", "gpu-postprocess"])
def test_app_zoom_f64(ctx, B, tmp_path, extra):
    from PIL import Image
    W, H, Mv, K, F = 96, 64, 200, 2, 3
    centre, s = (-0.745, 0.11), 0.05
    key = lambda j: B.mandelbrot_params(W, H, max_iter=Mv, precision=B.PRECISION_F64, centre=centre, scale=(s * 2 ** (K - j),) * 2)
    frames = binding_sequence(ctx, B, W, H, K, F, key)
    assert len(frames) == K * F + 1
    r = run_app(tmp_path, ["--out", tmp_path / "dive.png", "--zoom", K, F, "--width", W, "--height", H, "--max-iter", Mv, "--precision", "f64",
                           "--centre", centre[0], centre[1], "--scale", s, s, "--streamed-save"] + extra)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "--streamed-save has no effect" in r.stdout and r.stdout.count("keyframe ") == K + 1 and "zoom: 3 keyframes" in r.stdout, r.stdout
    files = sorted(p.name for p in tmp_path.glob("dive_*.png"))
    assert files == [f"dive_{i:05d}.png" for i in range(K * F + 1)], files
    for i, name in enumerate(files):
        got = np.asarray(Image.open(tmp_path / name).convert("RGBA"))
        assert np.array_equal(got, frames[i][1]), (i, extra)
        assert np.array_equal(frames[i][1], ctx.convert_rgba8(frames[i][0], 255.0)), i
        if i % F == 0:
            assert np.array_equal(got, ctx.mandelbrot_rgba8(key(i // F))), (i, "a keyframe's frame is the plain render of its scale")
    assert not np.array_equal(frames[0][1], frames[F][1])


def app_scale(text):
    """(mantissa, exponent) of a --scale text as the app forms it for a zoom's orbits: long double from text, split by frexp, the
    mantissa rounded to double."""
    m, e = np.frexp(np.longdouble(text))
    return float(m), int(e)


# 2^-40 exactly; a scale that is no power of two; the default view (no --centre / --scale at all) in a perturbation precision
@pytest.mark.parametrize("text,centre,precision", [("9.094947017729282379150390625e-13", K4, "perturb"), ("1e-20", K4, "perturb"),
                                                   ("3e-9", K4, "perturb-bla"), (None, ("-0.445", "0"), "perturb"),
                                                   (None, ("-0.445", "0"), "perturb-bla-deep")],
                         ids=["2^-40", "1e-20", "3e-9-bla", "default-view", "default-view-bla-deep"])
def test_app_zoom_perturb(ctx, B, tmp_path, text, centre, precision):
    from PIL import Image
    W, H, Mv, K, F = 64, 48, 300, 1, 2
    sm, se = app_scale(text or "2.34")
    prec, tables = {"perturb": (B.PRECISION_PERTURB, ()), "perturb-bla": (B.PRECISION_PERTURB_BLA, ("bla",)),
                    "perturb-bla-deep": (B.PRECISION_PERTURB_BLA_DEEP, ("bla_deep",))}[precision]
    P = lambda: B.mandelbrot_params(W, H, max_iter=Mv, precision=prec, **ZERO)
    held = []

    def key(j):
        o = B.Orbit(centre[0], centre[1], sm, sm, Mv, se + (K - j))
        for t in tables:
            getattr(o, t)()
        held.append(o)
        ctx.bind_mandelbrot_orbit(o)
        return P()

    try:
        frames = binding_sequence(ctx, B, W, H, K, F, key)
        ends = []
        for j in (0, K):
            ctx.bind_mandelbrot_orbit(held[j])
            ends.append(ctx.mandelbrot_rgba8(P()))
    finally:
        ctx.bind_mandelbrot_orbit(None)
        for o in held:
            o.close()
    view = ["--centre", centre[0], centre[1], "--scale", text, text] if text else []
    r = run_app(tmp_path, ["--zoom", K, F, "--width", W, "--height", H, "--max-iter", Mv, "--precision", precision] + view)
    assert r.returncode == 0, r.stdout + r.stderr
    files = sorted(p.name for p in tmp_path.glob("mandelbrot_*.png"))
    assert files == [f"mandelbrot_{i:05d}.png" for i in range(K * F + 1)], files
    for i, name in enumerate(files):
        assert np.array_equal(np.asarray(Image.open(tmp_path / name).convert("RGBA")), frames[i][1]), i
    assert np.array_equal(frames[0][1], ends[0]) and np.array_equal(frames[K * F][1], ends[1])


def test_app_zoom_default_view_f32(ctx, B, tmp_path):
    """No --centre / --scale: the deepest keyframe is the still the app renders without --zoom (the default params' float words)."""
    from PIL import Image
    W, H, K, F = 64, 48, 1, 2
    r = run_app(tmp_path, ["--zoom", K, F, "--width", W, "--height", H])
    assert r.returncode == 0, r.stdout + r.stderr
    last = np.asarray(Image.open(tmp_path / f"mandelbrot_{K * F:05d}.png").convert("RGBA"))
    assert np.array_equal(last, ctx.mandelbrot_rgba8(B.mandelbrot_params(W, H)))
    r = run_app(tmp_path, ["--zoom", 200, 1, "--width", W, "--height", H])
    assert r.returncode != 0 and "beyond what a view holds" in r.stdout, r.stdout


def test_context_closes_its_zooms(B):
    with B.Context(0) as c2:
        z = c2.zoom(16, 8)
        z.push(B.mandelbrot_params(16, 8))
        z2 = B.Zoom(c2, 8, 8)
        del z2                                                             # (collected: its weak reference is dead by the time of close)
    assert not z._h and not c2._h
    z.close()


def test_app_zoom_usage(tmp_path):
    for bad in (["--zoom", 0, 3], ["--zoom", 2, 0]):
        r = run_app(tmp_path, bad + ["--width", 16, "--height", 16])
        assert r.returncode != 0 and "usage: --zoom K F" in r.stdout, r.stdout
    assert not list(tmp_path.glob("*.png"))
