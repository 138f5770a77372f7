"""Zoom sequences from count keyframes on the MI355X: the compose kernel alone on uploaded planes against
tests/mandel_zoom_counts_ref.py bit for bit (four colourings, each output alone and both, deep absent, widths one off the block), the
table kernel through the sequence object (its maps and a mid-octave frame against the planes the blocking renders return), the identities
in every precision, every device refusal and the state it leaves, the app."""
import os
import subprocess

import numpy as np
import pytest

import mandel_equalise_ref as E
import mandel_smooth_equalise_ref as SE
import mandel_zoom_counts_ref as ZC
import mandel_zoom_ref as Z
from test_gpu_mandel_zoom import ZERO, precision_pairs, refused
from test_mandel_zoom_counts_host import KCOLOR, SHAPES as HOST_SHAPES, frame_map, planes
from test_mandel_zoom_host import bits, ratios

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "mandelbrot")
INVALID = 1
# (W, H); the added ones: one column short of a block, one past it, and 5 x 33 blocks with a partial last block on both axes
SHAPES = HOST_SHAPES + [(63, 5), (65, 5), (257, 130)]
MAX_ITERS = (1, 128, 300)


def device_planes(W, H, M, smooth):
    """The host test's keyframes; the smooth ones with counts above 256 M added, which the device takes as interior."""
    wide, deep = (np.array(a) for a in planes(W, H, M, smooth))
    if smooth and W * H >= 4:
        wide.reshape(-1)[1] = 256 * M + 1
        deep.reshape(-1)[2] = 0xffffffff
    return wide, deep


class Stage:
    """mc_mandelbrot_zoom_compose_counts_device_async on two uploaded count keyframes.  Each output lies between two guard rows, which must
    come back untouched; an output that was not asked for must come back untouched as a whole."""

    def __init__(self, ctx, p, wide, deep, table):
        import torch
        self.torch, self.ctx, self.p, self.table = torch, ctx, p, table
        self.H, self.W = wide.shape
        self.d_wide = torch.from_numpy(wide.view(np.int32)).cuda()
        self.d_deep = torch.from_numpy(deep.view(np.int32)).cuda()

    def __call__(self, r, with_deep=True, want_rgba=True, want_rgba8=True):
        torch, H, W = self.torch, self.H, self.W
        d_f = torch.full((H + 2, W, 4), -7.0, dtype=torch.float32, device="cuda")
        d_8 = torch.full((H + 2, W, 4), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.ctx.zoom_compose_counts_device(self.p, self.d_wide.data_ptr(), self.d_deep.data_ptr() if with_deep else 0, self.table, r,
                                            d_f[1:].data_ptr() if want_rgba else 0, d_8[1:].data_ptr() if want_rgba8 else 0)
        self.ctx.synchronize()
        f, b = d_f.cpu().numpy(), d_8.cpu().numpy()
        assert (f[0] == -7.0).all() and (f[-1] == -7.0).all() and (b[0] == 7).all() and (b[-1] == 7).all(), "a write outside the frame"
        if not want_rgba:
            assert (f == -7.0).all()
        if not want_rgba8:
            assert (b == 7).all()
        return (f[1:-1] if want_rgba else None), (b[1:-1] if want_rgba8 else None)


@pytest.mark.parametrize("mode", ZC.MODES)
@pytest.mark.parametrize("which", range(len(SHAPES)), ids=[f"{w}x{h}" for w, h in SHAPES])
def test_stage_is_the_restatement(ctx, B, which, mode):
    W, H = SHAPES[which]
    M = MAX_ITERS[which % 3]
    wide, deep = device_planes(W, H, M, mode.startswith("smooth"))
    lut = B.colour_lut(M, KCOLOR)
    p = B.mandelbrot_params(W, H, max_iter=M, k_color=KCOLOR, flags=ZC.flag(B, mode))
    table = frame_map(mode, wide, deep, M)
    stage = Stage(ctx, p, wide, deep, table)
    for r in ratios(B):
        for with_deep in (True, False):
            want, _ = ZC.frame(mode, wide, deep if with_deep else None, M, lut, table, r)
            want8 = Z.rgba8(want)
            f, b = stage(r, with_deep)
            bad = (bits(f) != bits(want)).any(axis=-1)
            assert not bad.any(), (W, H, M, mode, r, with_deep, int(bad.sum()), f[bad][:2], want[bad][:2])
            assert np.array_equal(b, want8), (W, H, M, mode, r, with_deep)
            f, b = stage(r, with_deep, want_rgba8=False)
            assert b is None and np.array_equal(bits(f), bits(want)), (W, H, mode, r, with_deep, "vec4 only")
            f, b = stage(r, with_deep, want_rgba=False)
            assert f is None and np.array_equal(b, want8), (W, H, mode, r, with_deep, "RGBA8 only")
    # ... and the host form runs the same source
    host = B.zoom_compose_counts(p, np.minimum(wide, 256 * M) if mode.startswith("smooth") else wide, None, table, 0.75)[0]
    assert np.array_equal(bits(stage(0.75, False)[0]), bits(host))


def test_stage_refusals(ctx, B):
    import torch
    W, H, M = 8, 8, 128
    k = torch.zeros((2, H, W), dtype=torch.int32, device="cuda")
    o = torch.zeros((H + 1, W, 4), dtype=torch.float32, device="cuda")
    out8 = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    w, d, f, b = k[0].data_ptr(), k[1].data_ptr(), o.data_ptr(), out8.data_ptr()
    P = lambda **kw: B.mandelbrot_params(W, H, max_iter=kw.pop("max_iter", M), **kw)
    ident = np.arange(M + 1, dtype=np.uint32)
    knots = (256 * np.arange(M + 1)).astype(np.uint32)
    EQ, SM, SQ, DI = B.MANDEL_COLOUR_EQUALISED, B.MANDEL_COLOUR_SMOOTH, B.MANDEL_COLOUR_SMOOTH_EQUALISED, B.MANDEL_COLOUR_DISTANCE
    who = "mc_mandelbrot_zoom_compose_counts_device_async"
    call = lambda *a, **kw: (lambda: ctx.zoom_compose_counts_device(*a, **kw))
    refused(B, call(P(), w + 2, d, None, 0.75, f), [who, "aligned"])
    refused(B, call(P(), w, d + 1, None, 0.75, f), "aligned")
    refused(B, call(P(), w, d, None, 0.75, f + 4), "aligned")
    refused(B, call(P(), w, d, None, 0.75, 0, b + 2), "aligned")
    refused(B, call(P(), w, d, None, 0.75, 0, w), [who, "overlaps"])       # in place: an RGBA8 frame is as large as a keyframe
    refused(B, call(P(), w, d, None, 0.75, 0, d), "overlaps")
    refused(B, call(P(), w, d, None, 0.75, 0, d + 4 * W), "overlaps")
    refused(B, call(P(), w, d, None, 0.75, f, f + 16 * W), "overlaps")     # the two outputs on each other
    refused(B, call(P(), 0, d, None, 0.75, f), "NULL")
    refused(B, call(P(), w, d, None, 0.75), "at least one output")
    refused(B, call(P(), w, d, None, 0.4999, f), "outside [0.5, 1]")
    refused(B, call(P(), w, d, None, float("nan"), f), "outside [0.5, 1]")
    refused(B, call(P(flags=EQ | SM), w, d, ident, 0.75, f), [who, "more than one colouring"])
    refused(B, call(P(flags=DI), w, d, None, 0.75, f), "MC_MANDEL_COLOUR_DISTANCE")
    refused(B, call(P(supersample=2), w, d, None, 0.75, f), "MC_MANDEL_SUPERSAMPLE")
    refused(B, call(P(supersample=2, adaptive=True), w, d, None, 0.75, f), "MC_MANDEL_SUPERSAMPLE")
    refused(B, call(P(flags=B.MANDEL_FMA), w, d, None, 0.75, f), "MC_MANDEL_FMA")
    refused(B, call(P(flags=B.MANDEL_ITERS_U16), w, d, None, 0.75, f), "MC_MANDEL_ITERS_U16")
    refused(B, call(P(row_begin=2), w, d, None, 0.75, f), "whole image")
    refused(B, call(P(row_block=8, row_stride=16), w, d, None, 0.75, f), "whole image")
    refused(B, call(P(), w, d, ident, 0.75, f), "take none")
    refused(B, call(P(flags=SM), w, d, knots, 0.75, f), "take none")
    refused(B, call(P(flags=EQ), w, d, None, 0.75, f), "need a map")
    refused(B, call(P(flags=SQ), w, d, None, 0.75, f), "need a map")
    bad = ident.copy(); bad[7] = M + 1
    refused(B, call(P(flags=EQ), w, d, bad, 0.75, f), "a map entry exceeds max_iter")
    bad = knots.copy(); bad[7] = bad[8] + 1
    refused(B, call(P(flags=SQ), w, d, bad, 0.75, f), "must not decrease")
    refused(B, call(P(flags=SM, max_iter=1 << 24), w, d, None, 0.75, f), "2^24 - 1")
    ctx.zoom_compose_counts_device(P(flags=SQ), w, w, knots, 1.0, f, b)   # (an input may be both keyframes; nothing is written to it)
    ctx.synchronize()


# ---- the sequence object ----------------------------------------------------------------------------------------------------------------
def still(ctx, p):
    return ctx.mandelbrot(p, want_iters=False)[0]


def count_plane(ctx, B, mode, kw, W, H):
    """The plane a keyframe holds, through the blocking renders: n of mc_mandelbrot_render, or q of mc_mandelbrot_render_smooth."""
    if mode.startswith("smooth"):
        return ctx.mandelbrot_smooth(B.mandelbrot_params(W, H, flags=B.MANDEL_COLOUR_SMOOTH, **kw), want_rgba=False, want_iters=False)[2]
    return ctx.mandelbrot(B.mandelbrot_params(W, H, **kw), want_rgba=False)[1]


def host_map(B, mode, plane, M):
    if mode == "equalised":
        return B.equalise_map(M, E.histogram(plane, M))
    if mode == "smooth-equalised":
        return B.smooth_equalise_map(M, SE.histogram(plane, M))
    return None


@pytest.mark.parametrize("mode", ZC.MODES)
def test_sequence_maps_and_frames(ctx, B, mode):
    W, H, M, S = 96, 64, 128, 4
    kws = [dict(max_iter=M, k_color=KCOLOR, scale=(s, s)) for s in (2.34, 1.17, 0.585)]
    ps = [B.mandelbrot_params(W, H, flags=ZC.flag(B, mode), **kw) for kw in kws]
    before = still(ctx, ps[0])
    pl = [count_plane(ctx, B, mode, kw, W, H) for kw in kws]
    maps = [host_map(B, mode, a, M) for a in pl]
    lut = B.colour_lut(M, KCOLOR)
    ranked = maps[0] is not None
    with ctx.zoom_counts(W, H) as z:
        refused(B, lambda: z.frame(0, S), "no keyframe has been pushed")
        refused(B, lambda: z.maps(), "mc_mandelbrot_zoom_counts_maps")
        z.push(ps[0])
        kms, cms = ctx.last_timing()
        assert kms > 0 and cms == 0
        if ranked:
            mw, md = z.maps()
            assert np.array_equal(mw, maps[0]) and np.array_equal(md, maps[0]), "one keyframe held: its map, twice"
        else:
            refused(B, lambda: z.maps(), "no map")
        f, f8 = z.frame(0, S, want_rgba8=True)
        assert np.array_equal(bits(f), bits(still(ctx, ps[0]))), "one keyframe, step 0: the blocking render's bits"
        assert np.array_equal(f8, ctx.mandelbrot_rgba8(ps[0]))
        kms, cms = ctx.last_timing()
        assert kms > 0 and cms >= 0
        want = ZC.frame(mode, pl[0], None, M, lut, maps[0], B.zoom_ratio(1, S))[0]
        assert np.array_equal(bits(z.frame(1, S)[0]), bits(want)), "one keyframe alone, with its own map at any step"
        z.push(ps[1])
        if ranked:
            mw, md = z.maps()
            assert np.array_equal(mw, maps[0]) and np.array_equal(md, maps[1])
            assert not np.array_equal(maps[0], maps[1])
        assert np.array_equal(bits(z.frame(S, S)[0]), bits(still(ctx, ps[1]))), "step S: the deeper keyframe's own image"
        for step in range(S + 1):
            table = ZC.blend(maps[0], maps[1], step, S) if ranked else None
            want = ZC.frame(mode, pl[0], pl[1], M, lut, table, B.zoom_ratio(step, S))[0]
            f, f8 = z.frame(step, S, want_rgba8=True)
            assert np.array_equal(bits(f), bits(want)), (mode, step)
            assert np.array_equal(f8, Z.rgba8(want)), (mode, step)
            assert np.array_equal(z.frame(step, S, want_rgba=False, want_rgba8=True)[1], f8), (mode, step)
        # two keyframes held: a refused push leaves BOTH where they were, with their maps
        other = [m for m in ZC.MODES if m != mode][0]
        bad = [B.mandelbrot_params(W, H, flags=ZC.flag(B, mode), max_iter=M, k_color=KCOLOR, scale=(0.6, 0.6)),           # not half
               B.mandelbrot_params(W, H, flags=ZC.flag(B, other), max_iter=M, k_color=KCOLOR, scale=(0.585, 0.585)),      # another colouring
               B.mandelbrot_params(W, H, flags=ZC.flag(B, mode), max_iter=M + 1, k_color=KCOLOR, scale=(0.585, 0.585)),
               B.mandelbrot_params(W, H, flags=ZC.flag(B, mode), max_iter=M, scale=(0.585, 0.585)),                      # another k_color
               B.mandelbrot_params(W, H, flags=ZC.flag(B, mode), max_iter=M, k_color=KCOLOR, scale=(0.585, 0.585), row_begin=8),
               B.mandelbrot_params(W, H, flags=ZC.flag(B, mode) | B.MANDEL_COLOUR_DISTANCE, max_iter=M, k_color=KCOLOR, scale=(0.585, 0.585)),
               B.mandelbrot_params(W, H, flags=ZC.flag(B, mode), max_iter=M, k_color=KCOLOR, supersample=2, scale=(0.585, 0.585)),
               B.mandelbrot_params(W, H, flags=ZC.flag(B, mode), max_iter=M, k_color=KCOLOR, precision=B.PRECISION_PERTURB, **ZERO),
               B.mandelbrot_params(W + 1, H, flags=ZC.flag(B, mode), max_iter=M, k_color=KCOLOR, scale=(0.585, 0.585))]
        table = ZC.blend(maps[0], maps[1], 1, S) if ranked else None
        mid = ZC.frame(mode, pl[0], pl[1], M, lut, table, B.zoom_ratio(1, S))[0]
        for p in bad:
            refused(B, lambda: z.push(p))
            assert np.array_equal(bits(z.frame(1, S)[0]), bits(mid)), "a refused push left both keyframes"
        refused(B, lambda: z.frame(S + 1, S), ["mc_mandelbrot_zoom_counts_frame", "steps per octave"])
        refused(B, lambda: z.frame(0, 0), "steps per octave")
        refused(B, lambda: z.frame(1, S, want_rgba=False, want_rgba8=False), "at least one output")
        z.push(ps[2])                                                      # the slots rotate: wide = keyframe 1, deep = keyframe 2
        assert np.array_equal(bits(z.frame(S, S)[0]), bits(still(ctx, ps[2])))
        table = ZC.blend(maps[1], maps[2], 3, S) if ranked else None
        assert np.array_equal(bits(z.frame(3, S)[0]), bits(ZC.frame(mode, pl[1], pl[2], M, lut, table, B.zoom_ratio(3, S))[0]))
    assert np.array_equal(bits(still(ctx, ps[0])), bits(before)), "a render on the same context afterwards is unchanged"
    plain = B.mandelbrot_params(W, H, max_iter=M)
    assert np.array_equal(ctx.mandelbrot(plain)[1], ctx.mandelbrot(plain, want_rgba=False)[1])


@pytest.mark.parametrize("which", range(8), ids=["f32", "ds", "f64", "perturb", "perturb-bla", "perturb-bla-deep", "deep-orbit", "f32-then-f64"])
def test_identities_in_every_precision(ctx, B, which):
    (W, H), Mv = ((40, 24), (67, 35))[which % 2], (128, 200, 300)[which % 3]
    name, pair = precision_pairs(B, Mv)[which]
    S = 2
    held = []
    try:
        orbits = []
        for kw, make in pair:
            o = make() if make else None
            if o:
                held.append(o)
            orbits.append(o)
        for mode in ZC.MODES:
            with ctx.zoom_counts(W, H) as z:
                stills = []
                for (kw, _), o in zip(pair, orbits):
                    if o:
                        ctx.bind_mandelbrot_orbit(o)
                    p = B.mandelbrot_params(W, H, flags=ZC.flag(B, mode), **kw)
                    stills.append(still(ctx, p))
                    z.push(p)
                    if len(stills) == 1:
                        assert np.array_equal(bits(z.frame(0, S)[0]), bits(stills[0])), (name, mode, "frame(0) with one keyframe")
                f, f8 = z.frame(S, S, want_rgba8=True)
                assert np.array_equal(bits(f), bits(stills[1])), (name, mode, "frame(S) is the deep keyframe's own render")
                assert np.array_equal(f8, Z.rgba8(stills[1])), (name, mode)
                assert np.isfinite(z.frame(1, S)[0]).all(), (name, mode)
    finally:
        ctx.bind_mandelbrot_orbit(None)
        for o in held:
            o.close()


def test_first_push_refusals_leave_nothing(ctx, B):
    W, H, M = 40, 24, 128
    P = lambda **kw: B.mandelbrot_params(W, H, max_iter=M, **kw)
    with ctx.zoom_counts(W, H) as z:
        refused(B, lambda: z.push(P(row_begin=0, row_end=8)), ["mc_mandelbrot_zoom_counts_push", "whole image"])
        refused(B, lambda: z.push(P(flags=B.MANDEL_ITERS_U16)), "MC_MANDEL_ITERS_U16")
        refused(B, lambda: z.push(P(flags=B.MANDEL_COLOUR_SMOOTH | B.MANDEL_COLOUR_EQUALISED)), "more than one colouring")
        refused(B, lambda: z.push(P(adaptive=True)), "MC_MANDEL_SUPERSAMPLE")
        refused(B, lambda: z.push(P(flags=B.MANDEL_FMA)), "MC_MANDEL_FMA")
        refused(B, lambda: z.push(P(precision=B.PRECISION_PERTURB, **ZERO)), "no orbit bound")
        refused(B, lambda: z.push(B.mandelbrot_params(W, H + 1, max_iter=M)), ["40 x 25", "40 x 24"])
        refused(B, lambda: z.frame(0, 1), "no keyframe has been pushed")    # (none of those left a keyframe behind)
        z.push(P(flags=B.MANDEL_COLOUR_EQUALISED))
        for s in ((2.34, 2.34), (1.17, 2.34), (1.0, 1.0)):
            refused(B, lambda: z.push(P(flags=B.MANDEL_COLOUR_EQUALISED, scale=s)), ["not exactly half", "the centre is the caller's"])
        assert np.array_equal(bits(z.frame(0, 1)[0]), bits(still(ctx, P(flags=B.MANDEL_COLOUR_EQUALISED))))
    with pytest.raises(B.McError):
        B.ZoomCounts(ctx, 0, 8)
    with B.Context(0) as c2:                                               # closing the context closes its sequences first
        z = c2.zoom_counts(16, 8)
        z.push(B.mandelbrot_params(16, 8))
    assert not z._h and not c2._h
    z.close()


# ---- the app --------------------------------------------------------------------------------------------------------------------------------
def run_app(tmp_path, args):
    return subprocess.run([APP, "--quiet"] + [str(a) for a in args], capture_output=True, text=True, cwd=tmp_path, timeout=180)


@pytest.mark.parametrize("extra", [[], ["--gpu-postprocess"]], ids=["host-convert", "gpu-postprocess"])
@pytest.mark.parametrize("colour", ["equalised", "smooth-equalised"])
def test_app_zoom_counts(ctx, B, tmp_path, colour, extra):
    from PIL import Image
    W, H, Mv, K, F = 96, 64, 200, 2, 3
    centre, s = (-0.745, 0.11), 0.05
    kw = lambda j: dict(max_iter=Mv, precision=B.PRECISION_F64, centre=centre, scale=(s * 2 ** (K - j),) * 2)
    key = lambda j: B.mandelbrot_params(W, H, flags=ZC.flag(B, colour), **kw(j))
    r = run_app(tmp_path, ["--out", tmp_path / "dive.png", "--zoom", K, F, "--zoom-keyframes", "counts", "--colour", colour, "--width", W,
                           "--height", H, "--max-iter", Mv, "--precision", "f64", "--centre", centre[0], centre[1], "--scale", s, s] + extra)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("keyframe ") == K + 1 and "zoom: 3 keyframes" in r.stdout, r.stdout
    files = sorted(p.name for p in tmp_path.glob("dive_*.png"))
    assert files == [f"dive_{i:05d}.png" for i in range(K * F + 1)], files
    img = lambda i: np.asarray(Image.open(tmp_path / files[i]).convert("RGBA"))
    for j in range(K + 1):
        assert np.array_equal(img(j * F), ctx.mandelbrot_rgba8(key(j))), (j, "a keyframe's frame is the still of its view")
    pl = [count_plane(ctx, B, colour, kw(j), W, H) for j in (0, 1)]
    maps = [host_map(B, colour, a, Mv) for a in pl]
    want = ZC.frame(colour, pl[0], pl[1], Mv, B.colour_lut(Mv), ZC.blend(maps[0], maps[1], 2, F), B.zoom_ratio(2, F))[0]
    assert np.array_equal(img(2), Z.rgba8(want)), "a middle frame is the restatement's"


def test_app_colour_keyframes_are_the_default(ctx, B, tmp_path):
    W, H, K, F = 64, 48, 1, 2
    base = ["--zoom", K, F, "--width", W, "--height", H, "--colour", "equalised"]
    for d, more in (("a", []), ("b", ["--zoom-keyframes", "colours"])):
        (tmp_path / d).mkdir()
        r = run_app(tmp_path / d, base + more)
        assert r.returncode == 0, r.stdout + r.stderr
    names = sorted(p.name for p in (tmp_path / "a").glob("*.png"))
    assert names == [f"mandelbrot_{i:05d}.png" for i in range(K * F + 1)]
    for n in names:
        assert (tmp_path / "a" / n).read_bytes() == (tmp_path / "b" / n).read_bytes(), n
