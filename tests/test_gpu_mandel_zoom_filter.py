"""The area filter of zoom sequences on the MI355X: both filtered compose kernels on uploaded keyframes against the host calls and
tests/mandel_zoom_filter_ref.py bit for bit (sizes under, at and across the blocks, each output alone and both, guard rows, special
values, filter 0 against the unfiltered device calls), the count forms in all four colourings on planes the device rendered, the
sequence objects' filtered frames against the chain by hand, every device refusal, the app."""
import os
import subprocess

import numpy as np
import pytest

import mandel_zoom_counts_ref as ZC
import mandel_zoom_filter_ref as ZF
import mandel_zoom_ref as Z
from test_gpu_mandel_zoom import ZERO, precision_pairs, refused
from test_gpu_mandel_zoom_counts import count_plane, host_map
from test_mandel_zoom_counts_host import KCOLOR
from test_mandel_zoom_host import bits, keyframes, ratios

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "mandelbrot")
INVALID = 1
SHAPES = [(1, 1), (2, 2), (3, 5), (37, 23), (130, 70)]   # (W, H); 37 x 23: no block fits; 130 x 70: 3 blocks of columns, 18 of rows, partial last ones


class Stage:
    """A filtered device compose on two uploaded keyframes (vec4, or uint32 counts with p and a table).  Each output lies between two guard
    rows, which must come back untouched; an output that was not asked for must come back untouched as a whole."""

    def __init__(self, ctx, wide, deep, p=None, table=None):
        import torch
        self.torch, self.ctx, self.p, self.table = torch, ctx, p, table
        self.H, self.W = wide.shape[:2]
        up = (lambda a: torch.from_numpy(np.array(a, np.float32)).cuda()) if p is None else (lambda a: torch.from_numpy(np.array(a).view(np.int32)).cuda())
        self.d_wide, self.d_deep = up(wide), up(deep)

    def __call__(self, r, filter, with_deep=True, want_rgba=True, want_rgba8=True, unfiltered=False):
        torch, H, W = self.torch, self.H, self.W
        d_f = torch.full((H + 2, W, 4), -7.0, dtype=torch.float32, device="cuda")
        d_8 = torch.full((H + 2, W, 4), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        w, d = self.d_wide.data_ptr(), self.d_deep.data_ptr() if with_deep else 0
        f, b = d_f[1:].data_ptr() if want_rgba else 0, d_8[1:].data_ptr() if want_rgba8 else 0
        if self.p is None:
            if unfiltered:
                self.ctx.zoom_compose_device(W, H, w, d, r, f, b)
            else:
                self.ctx.zoom_compose_filtered_device(W, H, w, d, r, filter, f, b)
        elif unfiltered:
            self.ctx.zoom_compose_counts_device(self.p, w, d, self.table, r, f, b)
        else:
            self.ctx.zoom_compose_counts_filtered_device(self.p, w, d, self.table, r, filter, f, b)
        self.ctx.synchronize()
        f, b = d_f.cpu().numpy(), d_8.cpu().numpy()
        assert (f[0] == -7.0).all() and (f[-1] == -7.0).all() and (b[0] == 7).all() and (b[-1] == 7).all(), "a write outside the frame"
        if not want_rgba:
            assert (f == -7.0).all()
        if not want_rgba8:
            assert (b == 7).all()
        return (f[1:-1] if want_rgba else None), (b[1:-1] if want_rgba8 else None)


@pytest.mark.parametrize("special", [False, True], ids=["unit", "special-values"])
@pytest.mark.parametrize("W,H", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_stage_is_the_host_call_and_the_restatement(ctx, B, W, H, special):
    wide, deep = ZF.special_keyframes(W, H) if special else keyframes(W, H)
    stage = Stage(ctx, wide, deep)
    A = B.ZOOM_FILTER_AREA
    for r in ratios(B):
        for with_deep in (True, False):
            d = deep if with_deep else None
            want, _ = ZF.compose(wide, d, r, ZF.AREA)
            host, host8 = B.zoom_compose_filtered(wide, d, r, A, want_rgba=True, want_rgba8=True)
            f, b = stage(r, A, with_deep)
            bad = ~(ZF.same_bits(f, want) & ZF.same_bits(f, host))
            assert not bad.any(), (W, H, r, with_deep, int(bad.sum()), f[bad][:2], want[bad][:2])
            assert np.array_equal(b, Z.rgba8(want)) and np.array_equal(b, host8), (W, H, r, with_deep)
            f1, b1 = stage(r, A, with_deep, want_rgba8=False)
            assert b1 is None and ZF.same_bits(f1, f).all(), (W, H, r, with_deep, "vec4 only")
            f1, b1 = stage(r, A, with_deep, want_rgba=False)
            assert f1 is None and np.array_equal(b1, b), (W, H, r, with_deep, "RGBA8 only")
            # filter 0: the existing device call's bits
            f0, b0 = stage(r, B.ZOOM_FILTER_BILINEAR, with_deep)
            fu, bu = stage(r, 0, with_deep, unfiltered=True)
            assert ZF.same_bits(f0, fu).all() and np.array_equal(b0, bu), (W, H, r, with_deep, "filter 0")
            assert ZF.same_bits(f0, Z.compose(wide, d, r)[0]).all()
    if not special:
        assert np.array_equal(bits(stage(1.0, A, False)[0]), bits(wide))
        assert np.array_equal(bits(stage(0.5, A)[0]), bits(deep))
    else:                                                      # (1 * a) / 1: -0.0 and the infinities bit for bit, a NaN as a NaN
        assert ZF.same_bits(stage(1.0, A, False)[0], wide).all() and ZF.same_bits(stage(0.5, A)[0], deep).all()
        finite = ~np.isnan(deep)
        assert np.array_equal(bits(stage(0.5, A)[0])[finite], bits(deep)[finite])


def test_stage_refusals(ctx, B):
    import torch
    W, H = 8, 8
    k = torch.zeros((3, H, W, 4), dtype=torch.float32, device="cuda")
    out8 = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    w, d, o = k[0].data_ptr(), k[1].data_ptr(), k[2].data_ptr()
    who = "mc_mandelbrot_zoom_compose_filtered_device_async"
    call = lambda *a, **kw: (lambda: ctx.zoom_compose_filtered_device(*a, **kw))
    for f in (0, 1):
        refused(B, call(W, H, w + 4, d, 0.75, f, o), [who, "aligned"])
        refused(B, call(W, H, w, d + 8, 0.75, f, o), "aligned")
        refused(B, call(W, H, w, d, 0.75, f, o + 4), "aligned")
        refused(B, call(W, H, w, d, 0.75, f, 0, out8.data_ptr() + 2), "aligned")
        refused(B, call(W, H, w, d, 0.75, f, w), [who, "overlaps"])
        refused(B, call(W, H, w, d, 0.75, f, d), "overlaps")
        refused(B, call(W, H, w, d, 0.75, f, 0, d + 16), "overlaps")
        refused(B, call(W, H, w, d, 0.75, f, o, o), "overlaps")
        refused(B, call(W, H, 0, d, 0.75, f, o), "NULL")
        refused(B, call(W, H, w, d, 0.75, f), "at least one output")
        refused(B, call(0, H, w, d, 0.75, f, o), "above 0")
        refused(B, call(W, H, w, d, 0.4999, f, o), "outside [0.5, 1]")
        refused(B, call(W, H, w, d, float("nan"), f, o), "outside [0.5, 1]")
    refused(B, call(W, H, w, d, 0.75, 2, o), [who, "filter = 2 is neither"])
    ctx.zoom_compose_filtered_device(W, H, w, w, 1.0, 1, o)               # (an input may be both keyframes; nothing is written to it)
    ctx.synchronize()
    # the count form
    c = torch.zeros((2, H, W), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    cw, cd = c[0].data_ptr(), c[1].data_ptr()
    M = 128
    P = lambda **kw: B.mandelbrot_params(W, H, max_iter=M, **kw)
    ident = np.arange(M + 1, dtype=np.uint32)
    who = "mc_mandelbrot_zoom_compose_counts_filtered_device_async"
    ccall = lambda *a, **kw: (lambda: ctx.zoom_compose_counts_filtered_device(*a, **kw))
    for f in (0, 1):
        refused(B, ccall(P(), cw + 2, cd, None, 0.75, f, o), [who, "aligned"])
        refused(B, ccall(P(), cw, cd, None, 0.75, f, o + 4), "aligned")
        refused(B, ccall(P(), cw, cd, None, 0.75, f, 0, cw), [who, "overlaps"])
        refused(B, ccall(P(), 0, cd, None, 0.75, f, o), "NULL")
        refused(B, ccall(P(), cw, cd, None, 0.75, f), "at least one output")
        refused(B, ccall(P(), cw, cd, None, 0.4999, f, o), "outside [0.5, 1]")
        refused(B, ccall(P(flags=B.MANDEL_COLOUR_EQUALISED | B.MANDEL_COLOUR_SMOOTH), cw, cd, ident, 0.75, f, o), "more than one colouring")
        refused(B, ccall(P(flags=B.MANDEL_COLOUR_DISTANCE), cw, cd, None, 0.75, f, o), "MC_MANDEL_COLOUR_DISTANCE")
        refused(B, ccall(P(supersample=2), cw, cd, None, 0.75, f, o), "MC_MANDEL_SUPERSAMPLE")
        refused(B, ccall(P(), cw, cd, ident, 0.75, f, o), "take none")
        refused(B, ccall(P(flags=B.MANDEL_COLOUR_EQUALISED), cw, cd, None, 0.75, f, o), "need a map")
    refused(B, ccall(P(), cw, cd, None, 0.75, 5, o), [who, "filter = 5 is neither"])


# ---- count keyframes ------------------------------------------------------------------------------------------------------------------------
CW, CH, CM = 37, 23, 200


@pytest.mark.parametrize("mode", ZC.MODES)
def test_count_stage_is_the_compose_of_colours(ctx, B, mode):
    """Count planes the device rendered in F32, an octave apart: the filtered count kernel equals the vec4 filtered compose of the two
    coloured planes (the library's own and the restatement's), bit for bit, in every output form; filter 0 is the existing call."""
    kws = [dict(max_iter=CM, k_color=KCOLOR, scale=(s, s)) for s in (2.34, 1.17)]
    wide, deep = (count_plane(ctx, B, mode, kw, CW, CH) for kw in kws)
    maps = [host_map(B, mode, a, CM) for a in (wide, deep)]
    lut = B.colour_lut(CM, KCOLOR)
    p = B.mandelbrot_params(CW, CH, max_iter=CM, k_color=KCOLOR, flags=ZC.flag(B, mode))
    A = B.ZOOM_FILTER_AREA
    for step, r in ((1, B.zoom_ratio(1, 3)), (2, B.zoom_ratio(2, 3)), (0, 1.0), (3, 0.5)):
        table = None if maps[0] is None else ZC.blend(maps[0], maps[1], step, 3)
        stage = Stage(ctx, wide, deep, p, table)
        cw, cd = ZC.colour(mode, wide, CM, lut, table), ZC.colour(mode, deep, CM, lut, table)
        for with_deep in (True, False):
            want, _ = ZF.compose(cw, cd if with_deep else None, r, ZF.AREA)
            lib = B.zoom_compose_filtered(cw, cd if with_deep else None, r, A)[0]
            host = B.zoom_compose_counts_filtered(p, wide, deep if with_deep else None, table, r, A)[0]
            f, b = stage(r, A, with_deep)
            assert np.array_equal(bits(f), bits(want)), (mode, r, with_deep, "the restatement")
            assert np.array_equal(bits(f), bits(lib)) and np.array_equal(bits(f), bits(host)), (mode, r, with_deep)
            assert np.array_equal(b, Z.rgba8(want)), (mode, r, with_deep)
            assert np.array_equal(stage(r, A, with_deep, want_rgba=False)[1], b)
            assert np.array_equal(bits(stage(r, A, with_deep, want_rgba8=False)[0]), bits(f))
            f0, b0 = stage(r, 0, with_deep)
            fu, bu = stage(r, 0, with_deep, unfiltered=True)
            assert np.array_equal(bits(f0), bits(fu)) and np.array_equal(b0, bu), (mode, r, with_deep, "filter 0")
    assert not np.array_equal(wide, deep)


# ---- the sequence objects -------------------------------------------------------------------------------------------------------------------
def render(ctx, p):
    return ctx.mandelbrot(p, want_iters=False)[0]


def test_sequence_filtered_frames(ctx, B):
    W, H, Mv, F = 48, 32, 128, 3
    A = B.ZOOM_FILTER_AREA
    ps = [B.mandelbrot_params(W, H, max_iter=Mv, scale=(s, s)) for s in (2.34, 1.17, 0.585)]
    before = render(ctx, ps[0])
    k = [render(ctx, p) for p in ps]
    with ctx.zoom(W, H) as z:
        refused(B, lambda: z.frame_filtered(1.0, A), ["mc_mandelbrot_zoom_frame_filtered", "no keyframe has been pushed"])
        z.push(ps[0])
        assert np.array_equal(bits(z.frame_filtered(1.0, A)[0]), bits(k[0])), "one keyframe, r = 1"
        for j in (1, 2):
            z.push(ps[j])
            for step in range(1, F):
                r = B.zoom_ratio(step, F)
                want = ZF.compose(k[j - 1], k[j], r, ZF.AREA)[0]
                f, f8 = z.frame_filtered(r, A, want_rgba8=True)
                kms, cms = ctx.last_timing()
                assert kms > 0 and cms >= 0
                assert np.array_equal(bits(f), bits(want)), (j, step)
                assert np.array_equal(f8, Z.rgba8(want)), (j, step)
                assert np.array_equal(z.frame_filtered(r, A, want_rgba=False, want_rgba8=True)[1], f8)
                assert np.array_equal(bits(z.frame_filtered(r, B.ZOOM_FILTER_BILINEAR)[0]), bits(z.frame(r)[0]))
                assert not np.array_equal(bits(f), bits(z.frame(r)[0]))
                assert np.array_equal(bits(z.frame(r)[0]), bits(Z.compose(k[j - 1], k[j], r)[0])), "frame() afterwards: the bilinear bits"
            assert np.array_equal(bits(z.frame_filtered(0.5, A)[0]), bits(k[j])), "r = 0.5: the deep keyframe's render"
        refused(B, lambda: z.frame_filtered(0.75, 2), ["mc_mandelbrot_zoom_frame_filtered", "filter = 2 is neither"])
        refused(B, lambda: z.frame_filtered(1.5, A), "outside [0.5, 1]")
        refused(B, lambda: z.frame_filtered(0.75, A, want_rgba=False, want_rgba8=False), "at least one output")
    assert np.array_equal(bits(render(ctx, ps[0])), bits(before)), "a plain render on the same context afterwards is unchanged"


@pytest.mark.parametrize("mode", ZC.MODES)
def test_counts_sequence_filtered_frames(ctx, B, mode):
    W, H, M, F = 48, 32, 128, 3
    A = B.ZOOM_FILTER_AREA
    kws = [dict(max_iter=M, k_color=KCOLOR, scale=(s, s)) for s in (2.34, 1.17, 0.585)]
    ps = [B.mandelbrot_params(W, H, flags=ZC.flag(B, mode), **kw) for kw in kws]
    before = render(ctx, ps[0])
    pl = [count_plane(ctx, B, mode, kw, W, H) for kw in kws]
    maps = [host_map(B, mode, a, M) for a in pl]
    lut = B.colour_lut(M, KCOLOR)
    with ctx.zoom_counts(W, H) as z:
        refused(B, lambda: z.frame_filtered(0, F, A), ["mc_mandelbrot_zoom_counts_frame_filtered", "no keyframe has been pushed"])
        z.push(ps[0])
        assert np.array_equal(bits(z.frame_filtered(0, F, A)[0]), bits(render(ctx, ps[0])))
        for j in (1, 2):
            z.push(ps[j])
            for step in range(1, F):
                table = None if maps[0] is None else ZC.blend(maps[j - 1], maps[j], step, F)
                want = ZF.frame_counts(mode, pl[j - 1], pl[j], M, lut, table, B.zoom_ratio(step, F), ZF.AREA)[0]
                f, f8 = z.frame_filtered(step, F, A, want_rgba8=True)
                kms, cms = ctx.last_timing()
                assert kms > 0 and cms >= 0
                assert np.array_equal(bits(f), bits(want)), (mode, j, step)
                assert np.array_equal(f8, Z.rgba8(want)), (mode, j, step)
                assert np.array_equal(z.frame_filtered(step, F, A, want_rgba=False, want_rgba8=True)[1], f8)
                plain = z.frame(step, F)[0]
                assert np.array_equal(bits(z.frame_filtered(step, F, 0)[0]), bits(plain))
                assert np.array_equal(bits(plain), bits(ZC.frame(mode, pl[j - 1], pl[j], M, lut, table, B.zoom_ratio(step, F))[0]))
            assert np.array_equal(bits(z.frame_filtered(F, F, A)[0]), bits(render(ctx, ps[j]))), "step F: the deep keyframe's own render"
        refused(B, lambda: z.frame_filtered(1, F, 3), ["mc_mandelbrot_zoom_counts_frame_filtered", "filter = 3 is neither"])
        refused(B, lambda: z.frame_filtered(F + 1, F, A), "steps per octave")
    assert np.array_equal(bits(render(ctx, ps[0])), bits(before)), "a render on the same context afterwards is unchanged"


def test_counts_sequence_perturbation(ctx, B):
    """One perturbation precision, an orbit bound per keyframe: the filtered frame equals the chain by hand on the planes the blocking
    render returns under the same orbits."""
    W, H, Mv, F = 37, 23, 200, 2
    mode = "smooth-equalised"
    name, pair = [x for x in precision_pairs(B, Mv) if x[0] == "perturb"][0]
    held = []
    try:
        with ctx.zoom_counts(W, H) as z:
            pl = []
            for kw, make in pair:
                o = make()
                held.append(o)
                ctx.bind_mandelbrot_orbit(o)
                kw = dict(kw, k_color=KCOLOR)
                pl.append(count_plane(ctx, B, mode, kw, W, H))
                z.push(B.mandelbrot_params(W, H, flags=ZC.flag(B, mode), **kw))
            maps = [host_map(B, mode, a, Mv) for a in pl]
            table = ZC.blend(maps[0], maps[1], 1, F)
            want = ZF.frame_counts(mode, pl[0], pl[1], Mv, B.colour_lut(Mv, KCOLOR), table, B.zoom_ratio(1, F), ZF.AREA)[0]
            f, f8 = z.frame_filtered(1, F, B.ZOOM_FILTER_AREA, want_rgba8=True)
            assert np.array_equal(bits(f), bits(want)) and np.array_equal(f8, Z.rgba8(want))
    finally:
        ctx.bind_mandelbrot_orbit(None)
        for o in held:
            o.close()


# ---- the app --------------------------------------------------------------------------------------------------------------------------------
def run_app(cwd, args):
    return subprocess.run([APP, "--quiet"] + [str(a) for a in args], capture_output=True, text=True, cwd=cwd, timeout=180)


@pytest.mark.parametrize("keyframes_as", ["colours", "counts"])
def test_app_zoom_filter(ctx, B, tmp_path, keyframes_as):
    """--zoom 1 3 --zoom-filter area writes the library chain's filtered frames; without the option (and with bilinear) the files are the
    bilinear chain's, byte for byte."""
    from PIL import Image
    W, H, Mv, K, F = 48, 32, 128, 1, 3
    mode = "equalised"
    centre, s = (-0.745, 0.11), 0.05
    ps = [B.mandelbrot_params(W, H, max_iter=Mv, flags=ZC.flag(B, mode), precision=B.PRECISION_F64, centre=centre, scale=(s * 2 ** (K - j),) * 2)
          for j in range(K + 1)]
    chains = {}
    for name, filt in (("area", B.ZOOM_FILTER_AREA), ("bilinear", B.ZOOM_FILTER_BILINEAR)):
        frames = []
        with (ctx.zoom_counts(W, H) if keyframes_as == "counts" else ctx.zoom(W, H)) as z:
            for j in range(K + 1):
                z.push(ps[j])
                for step in ([0] if j == 0 else range(1, F + 1)):
                    if keyframes_as == "counts":
                        frames.append(z.frame_filtered(step, F, filt, want_rgba=False, want_rgba8=True)[1])
                    else:
                        frames.append(z.frame_filtered(B.zoom_ratio(step, F), filt, want_rgba=False, want_rgba8=True)[1])
        chains[name] = frames
    base = ["--zoom", K, F, "--width", W, "--height", H, "--max-iter", Mv, "--colour", mode, "--zoom-keyframes", keyframes_as, "--gpu-postprocess",
            "--precision", "f64", "--centre", centre[0], centre[1], "--scale", s, s]
    for d, more, chain in (("a", ["--zoom-filter", "area"], "area"), ("b", [], "bilinear"), ("c", ["--zoom-filter", "bilinear"], "bilinear")):
        (tmp_path / d).mkdir()
        r = run_app(tmp_path / d, base + more)
        assert r.returncode == 0, r.stdout + r.stderr
        names = sorted(p.name for p in (tmp_path / d).glob("*.png"))
        assert names == [f"mandelbrot_{i:05d}.png" for i in range(K * F + 1)], names
        for i, n in enumerate(names):
            assert np.array_equal(np.asarray(Image.open(tmp_path / d / n).convert("RGBA")), chains[chain][i]), (d, i)
    for n in sorted(p.name for p in (tmp_path / "b").glob("*.png")):
        assert (tmp_path / "b" / n).read_bytes() == (tmp_path / "c" / n).read_bytes(), n
    assert any(not np.array_equal(a, b) for a, b in zip(chains["area"], chains["bilinear"]))
    for app, args, needle in (("mandelbrot", ["--zoom-filter", "area"], "--zoom-filter: needs --zoom"),
                              ("mandelbrot", base + ["--zoom-filter", "box"], "not one of bilinear | area")):
        r = run_app(tmp_path, args)
        assert r.returncode == 1 and needle in r.stdout and "now running app" not in r.stdout, r.stdout
    r = subprocess.run([os.path.join(os.path.dirname(APP), "pathtracer"), "--zoom-filter", "area"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and "--zoom-filter: a Mandelbrot option" in r.stdout and "now running app" not in r.stdout
