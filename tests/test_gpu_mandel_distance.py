"""MC_MANDEL_COLOUR_DISTANCE on the MI355X: the stencil kernel alone on uploaded synthetic smooth planes against tests/mandel_distance_ref.py
bit for bit (every shape class of the vector paths, an offset plane, output bands, each output alone, three thresholds, differences past
2^53), the whole chain in every precision, every refusal, the warm-up, the app."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mandel_distance_ref as DR
import mandel_smooth_ref as S
from test_gpu_mandel_equalise import bound_view, six_views

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "mandelbrot")
INVALID, UNSUPPORTED = 1, 5
M = 200                                                                  # the stage tests' max_iter
# (W, H): the issue's shapes, and widths of the classes they leave out: W mod 4 = 0 (every row one 16-B vector per lane) and W mod 4 = 2
# wide enough for a full group (rows alternate between the 16-B and the 8-B path)
SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 5), (13, 7), (67, 35), (131, 3), (257, 2), (1031, 517), (8, 5), (64, 9), (6, 4), (10, 3)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def dparams(B, w, h, flags=0, **kw):
    return B.mandelbrot_params(w, h, flags=B.MANDEL_COLOUR_DISTANCE | flags, **kw)


def stage(ctx, B, q, max_iter, T=1.0, rows=None, want_d=True, want_rgba=True, offset=0):
    """mc_mandelbrot_distance_device_async on the uploaded plane q: (D, rgba) of the band `rows` (None where not wanted).  offset: the
    plane starts that many uint32 past the allocation's start.  The outputs lie between two guard rows, which must come back untouched."""
    import torch
    H, W = q.shape
    r0, r1 = rows if rows else (0, H)
    buf = torch.zeros(H * W + offset, dtype=torch.int32, device="cuda")
    buf[offset:] = torch.from_numpy(np.ascontiguousarray(q).view(np.int32).ravel()).cuda()
    n = r1 - r0
    d_D = torch.full((n + 2, W), -7.0, dtype=torch.float32, device="cuda")
    d_rgba = torch.full((n + 2, W, 4), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    p = dparams(B, W, H, max_iter=max_iter, row_begin=r0, row_end=r1)
    ctx.mandelbrot_distance_device(p, buf.data_ptr() + 4 * offset, T, d_D[1:].data_ptr() if want_d else 0,
                                   d_rgba[1:].data_ptr() if want_rgba else 0)
    ctx.synchronize()
    D, rgba = d_D.cpu().numpy(), d_rgba.cpu().numpy()
    for a in (D, rgba):
        assert (a[0] == -7.0).all() and (a[-1] == -7.0).all(), "a write outside the band"
    if not want_d:
        assert (D == -7.0).all()
    if not want_rgba:
        assert (rgba == -7.0).all()
    return (D[1:-1] if want_d else None), (rgba[1:-1] if want_rgba else None)


def check_stage(ctx, B, q, max_iter, what, lut=None, **kw):
    rows = kw.get("rows")
    r0, r1 = rows if rows else (0, q.shape[0])
    want_D = DR.plane(q, max_iter)[r0:r1]                            # the WHOLE plane's D, then the band
    D, rgba = stage(ctx, B, q, max_iter, **kw)
    if D is not None:
        bad = bits(D) != bits(want_D)
        assert not bad.any(), (what, "D", int(bad.sum()), D[bad][:4], want_D[bad][:4])
    if rgba is not None:
        lut = B.colour_lut(max_iter) if lut is None else lut
        want = DR.colour(q[r0:r1], want_D, max_iter, lut, kw.get("T", 1.0))
        bad = (bits(rgba) != bits(want)).any(axis=-1)
        assert not bad.any(), (what, "rgba", int(bad.sum()), rgba[bad][:2], want[bad][:2])


# ---- the stage alone --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_stage_is_the_restatement(ctx, B, W, H):
    lut = B.colour_lut(M)
    planes = DR.synthetic_planes(W, H, M)
    if W * H > 100000:
        planes = [pl for pl in planes if pl[0] in ("random", "blobs")]      # the large shape: two planes keep the case quick
    for name, q in planes:
        check_stage(ctx, B, q, M, (name, W, H), lut=lut)
    q = dict(planes)["blobs"]
    check_stage(ctx, B, q, M, ("offset by 4 bytes", W, H), lut=lut, offset=1)
    check_stage(ctx, B, q, M, ("offset by 8 bytes", W, H), lut=lut, offset=2)
    check_stage(ctx, B, q, M, ("D only", W, H), want_rgba=False)
    check_stage(ctx, B, q, M, ("rgba only", W, H), lut=lut, want_d=False)
    for T in (0.5, 3.0):
        check_stage(ctx, B, q, M, ("threshold", T, W, H), lut=lut, T=T)
    bands = {(0, 1), (H - 1, H), (H // 3, max(H // 3 + 1, 2 * H // 3))}
    if H >= 3:
        bands.add((1, H - 1))                                           # its halo rows are the image's first and last rows
    for band in sorted(bands):
        for off in (0, 1):
            check_stage(ctx, B, q, M, ("band", band, off, W, H), lut=lut, rows=band, offset=off)


@pytest.mark.parametrize("W,H", [(5, 3), (67, 35), (260, 9)], ids=["5x3", "67x35", "260x9"])
def test_stage_with_differences_past_2_to_53(ctx, B, W, H):
    q = DR.large_plane(W, H)
    assert DR.g2_of(q).max() > 2.0 ** 53
    check_stage(ctx, B, q, DR.BIG_M, ("large, D", W, H), want_rgba=False)
    check_stage(ctx, B, q, DR.BIG_M, ("large, D, offset", W, H), want_rgba=False, offset=1)
    m = 400000                                                            # central differences of 2^26.6 each: g2 > 2^53, a 6 MB table
    q = DR.large_plane(W, H, m)
    assert (DR.g2_of(q) > 2.0 ** 53).mean() > 0.2
    check_stage(ctx, B, q, m, ("large, both", W, H))


# ---- the chain ----------------------------------------------------------------------------------------------------------------------------
def chain_views(B):
    ref = dict(max_iter=128)
    views = six_views(B)
    deep = (views[5][0] + " as perturb", dict(views[5][1], precision=B.PRECISION_PERTURB), views[5][2])
    return [("f32", dict(ref, precision=B.PRECISION_F32), None, (40, 24)),
            ("ds", dict(ref, precision=B.PRECISION_DS), None, (40, 24)),
            ("f64", dict(ref, precision=B.PRECISION_F64), None, (40, 24)),
            views[3] + ((203, 131),), views[4] + ((203, 131),), deep + ((203, 131),), views[5] + ((203, 131),)]


@pytest.mark.parametrize("which", range(7), ids=["f32", "ds", "f64", "perturb", "perturb-bla", "deep-orbit", "perturb-bla-deep"])
def test_chain_in_every_precision(ctx, B, which):
    name, kw, make, (W, H) = chain_views(B)[which]
    Mv = kw["max_iter"]
    lut = B.colour_lut(Mv)
    with bound_view(B, ctx, kw, make):
        _, n, q = ctx.mandelbrot_smooth(B.mandelbrot_params(W, H, flags=B.MANDEL_COLOUR_SMOOTH, **kw), want_rgba=False)
        p = dparams(B, W, H, **kw)
        rgba, n2, q2, D = ctx.mandelbrot_distance(p)
        assert np.array_equal(n2, n) and np.array_equal(q2, q), name
        want_D = DR.plane(q, Mv)
        want = DR.colour(q, want_D, Mv, lut)
        assert np.array_equal(bits(D), bits(want_D)), (name, int((bits(D) != bits(want_D)).sum()))
        assert np.array_equal(bits(rgba), bits(want)), name
        assert len(np.unique(D)) > 10, name
        rgba1, n1 = ctx.mandelbrot(p)
        assert np.array_equal(bits(rgba1), bits(want)) and np.array_equal(n1, n), name
        u8 = ctx.mandelbrot_rgba8(p)
        assert np.array_equal(u8, ctx.convert_rgba8(want, 255.0)), name
        again = ctx.mandelbrot_distance(p)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(again, (rgba, n2, q2, D))), name
        assert np.array_equal(ctx.mandelbrot_rgba8(p), u8)
        only_D = ctx.mandelbrot_distance(p, want_rgba=False, want_iters=False, want_smooth=False)
        assert only_D[:3] == (None, None, None) and np.array_equal(bits(only_D[3]), bits(want_D))
        kms, cms = ctx.last_timing()
        assert kms > 0 and cms >= 0


def test_chain_on_views_without_a_boundary(ctx, B):
    Mv = 128
    lut = B.colour_lut(Mv)
    p = dparams(B, 40, 24, max_iter=Mv, centre=(0.0, 0.0), scale=(0.1, 0.1))          # all interior
    rgba, n, q, D = ctx.mandelbrot_distance(p)
    assert (n == Mv).all() and (q == 256 * Mv).all() and (D == 0).all()
    assert np.array_equal(bits(rgba), bits(np.broadcast_to(lut[Mv], rgba.shape)))
    assert np.array_equal(ctx.mandelbrot_rgba8(p), ctx.convert_rgba8(rgba, 255.0))
    p = dparams(B, 40, 24, max_iter=Mv, centre=(2.0, 2.0), scale=(0.1, 0.1))          # every pixel escapes at once
    rgba, n, q, D = ctx.mandelbrot_distance(p)
    assert (n == 0).all() and (q < 256 * Mv).all()
    want_D = DR.plane(q, Mv)
    assert np.array_equal(bits(D), bits(want_D)) and np.array_equal(bits(rgba), bits(DR.colour(q, want_D, Mv, lut)))


# ---- refusals, the warm-up ------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, B):
    import torch
    w, h, Mv = 64, 48, 200
    d_rgba = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    d_it = torch.zeros((4 * h, 4 * w), dtype=torch.int32, device="cuda")
    d_D = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    L = B.lib()
    L.mc_context_warmup_mandelbrot.argtypes = [C.c_void_p, C.POINTER(B.MandelbrotParams), C.c_int]
    FLAG = "MC_MANDEL_COLOUR_DISTANCE"

    def refused(call, status=INVALID, says=FLAG):
        with pytest.raises(B.McError) as e:
            call()
        assert e.value.status == status, e.value
        if says:
            assert says in str(e.value), e.value

    p = dparams(B, w, h, max_iter=Mv)
    # a row tile or band of the two calls that honour the flag, and of the four-plane call; interleave
    for tile in (dict(row_begin=0, row_end=8), dict(row_begin=8, row_end=h), dict(row_begin=0, row_end=h, row_block=8, row_stride=16)):
        t = dparams(B, w, h, max_iter=Mv, **tile)
        refused(lambda: ctx.mandelbrot(t))
        refused(lambda: ctx.mandelbrot_rgba8(t))
        refused(lambda: ctx.mandelbrot_distance(t))
    # the calls that never take the flag (each names the calls to use instead)
    ident = np.arange(Mv + 1, dtype=np.uint32)
    refused(lambda: ctx.mandelbrot_device(p, d_rgba.data_ptr(), d_it.data_ptr()), says="mc_mandelbrot_render_distance")
    refused(lambda: ctx.mandelbrot_device(p, d_rgba.data_ptr(), d_it.data_ptr()))
    refused(lambda: ctx.mandelbrot_banded(p, 16))
    refused(lambda: ctx.mandelbrot_banded(p, 16, rgba8=True))
    refused(lambda: ctx.mandelbrot_smooth(p))
    refused(lambda: ctx.mandelbrot_smooth_device(p, d_rgba.data_ptr(), d_it.data_ptr(), 0))
    refused(lambda: ctx.mandelbrot_recolour_device(p, d_it.data_ptr(), 4, ident, d_rgba.data_ptr()))
    refused(lambda: ctx.mandelbrot_resolve_device(dparams(B, w, h, max_iter=Mv, supersample=2), d_it.data_ptr(), 4, None, d_rgba.data_ptr()))
    refused(lambda: ctx.mandelbrot_assemble_device(p, d_it.data_ptr(), 4, 1, 8, h, d_rgba.data_ptr()))
    with B.Multi(1) as mm:
        refused(lambda: mm.mandelbrot(p), UNSUPPORTED)
        refused(lambda: mm.mandelbrot_rgba8(p), UNSUPPORTED)
    # the flag together with another colouring, a resolve or the contraction switch
    combos = [(dict(flags=B.MANDEL_COLOUR_SMOOTH), "MC_MANDEL_COLOUR_SMOOTH"),
              (dict(flags=B.MANDEL_COLOUR_EQUALISED), "MC_MANDEL_COLOUR_EQUALISED"),
              (dict(supersample=2), "MC_MANDEL_SUPERSAMPLE"),
              (dict(supersample=8), "MC_MANDEL_SUPERSAMPLE"),
              (dict(supersample=4, adaptive=True), "MC_MANDEL_SUPERSAMPLE_ADAPTIVE"),
              (dict(adaptive=True), "MC_MANDEL_SUPERSAMPLE_ADAPTIVE"),
              (dict(flags=B.MANDEL_FMA), "MC_MANDEL_FMA")]
    for extra, word in combos:
        flags = extra.pop("flags", 0)
        c = dparams(B, w, h, flags=flags, max_iter=Mv, **extra)
        for call in (lambda: ctx.mandelbrot(c), lambda: ctx.mandelbrot(c, want_iters=False), lambda: ctx.mandelbrot_rgba8(c),
                     lambda: ctx.mandelbrot_distance(c),
                     lambda: ctx.mandelbrot_distance_device(c, d_it.data_ptr(), 1.0, d_D.data_ptr(), d_rgba.data_ptr())):
            refused(call)
            refused(call, says=word)
        assert L.mc_context_warmup_mandelbrot(ctx._h, C.byref(c), 1) == INVALID
        assert FLAG in L.mc_last_error_detail().decode()
    # the new calls' own rules
    plain = B.mandelbrot_params(w, h, max_iter=Mv)
    refused(lambda: ctx.mandelbrot_distance(plain), says="must carry MC_MANDEL_COLOUR_DISTANCE")
    refused(lambda: ctx.mandelbrot_distance_device(plain, d_it.data_ptr(), 1.0, d_D.data_ptr(), 0), says="must carry MC_MANDEL_COLOUR_DISTANCE")
    refused(lambda: ctx.mandelbrot_distance(p, want_rgba=False, want_iters=False, want_smooth=False, want_distance=False), says=None)
    refused(lambda: ctx.mandelbrot_distance_device(p, d_it.data_ptr(), 1.0, 0, 0), says=None)
    refused(lambda: ctx.mandelbrot_distance_device(p, 0, 1.0, d_D.data_ptr(), 0), says=None)
    refused(lambda: ctx.mandelbrot_distance_device(p, d_it.data_ptr() + 2, 1.0, d_D.data_ptr(), 0), says=None)
    refused(lambda: ctx.mandelbrot_distance_device(p, d_it.data_ptr(), 1.0, 0, d_rgba.data_ptr() + 4), says=None)
    for T in (0.0, -1.0, float("inf"), float("nan")):
        refused(lambda: ctx.mandelbrot_distance_device(p, d_it.data_ptr(), T, d_D.data_ptr(), 0), says="threshold_px")
    inter = dparams(B, w, h, max_iter=Mv, row_begin=0, row_end=h, row_block=8, row_stride=16)
    refused(lambda: ctx.mandelbrot_distance_device(inter, d_it.data_ptr(), 1.0, d_D.data_ptr(), 0), says="interleaved")
    refused(lambda: ctx.mandelbrot(dparams(B, w, h, flags=B.MANDEL_ITERS_U16, max_iter=Mv)))
    big = dparams(B, 8, 8, max_iter=S.MAX_ITER_LIMIT + 1, centre=(2.0, 2.0), scale=(0.1, 0.1))
    for call in (lambda: ctx.mandelbrot(big), lambda: ctx.mandelbrot_rgba8(big), lambda: ctx.mandelbrot_distance(big)):
        refused(call, says="2^24 - 1")
    # mc_mandelbrot_supersample_params copies the bit like any other
    assert B.supersample_params(dparams(B, w, h, max_iter=Mv, supersample=2)).flags & B.MANDEL_COLOUR_DISTANCE
    # after all that the context still renders plain, smooth and distance images
    rgba, n = ctx.mandelbrot(plain)
    assert np.array_equal(bits(rgba), bits(B.colour_lut(Mv)[n]))
    srgba, n2, q = ctx.mandelbrot_smooth(B.mandelbrot_params(w, h, max_iter=Mv, flags=B.MANDEL_COLOUR_SMOOTH))
    assert np.array_equal(n2, n) and np.array_equal(bits(srgba), bits(S.colour(q, Mv, B.colour_lut(Mv))))
    drgba, n3, q3, D = ctx.mandelbrot_distance(p)
    assert np.array_equal(n3, n) and np.array_equal(q3, q) and np.array_equal(bits(D), bits(DR.plane(q, Mv)))
    assert np.array_equal(bits(drgba), bits(DR.colour(q, DR.plane(q, Mv), Mv, B.colour_lut(Mv))))


def test_render_after_a_warm_up_with_the_flag(B):
    L = B.lib()
    L.mc_context_warmup_mandelbrot.argtypes = [C.c_void_p, C.POINTER(B.MandelbrotParams), C.c_int]
    W, H, Mv = 67, 35, 128
    with B.Context(0) as c2:
        p = dparams(B, W, H, max_iter=Mv)
        for how in (0, 1, 2, 3):
            assert L.mc_context_warmup_mandelbrot(c2._h, C.byref(p), how) == 0
        a = c2.mandelbrot_distance(p)
        u8 = c2.mandelbrot_rgba8(p)
        p64 = dparams(B, 40, 24, max_iter=Mv, precision=B.PRECISION_F64)
        assert L.mc_context_warmup_mandelbrot(c2._h, C.byref(p64), 1) == 0
        a64 = c2.mandelbrot_distance(p64)
    with B.Context(0) as c3:                                            # the same renders on a context never warmed up
        b = c3.mandelbrot_distance(p)
        b64 = c3.mandelbrot_distance(p64)
        assert np.array_equal(c3.mandelbrot_rgba8(p), u8)
    for x, y in zip(a + a64, b + b64):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert np.array_equal(bits(a[3]), bits(DR.plane(a[2], Mv)))


# ---- the app --------------------------------------------------------------------------------------------------------------------------------
def test_app_colour_distance(ctx, B, tmp_path):
    from PIL import Image
    w, h = 64, 48
    p = dparams(B, w, h, max_iter=300)
    want = ctx.mandelbrot_rgba8(p)
    D = ctx.mandelbrot_distance(p, want_rgba=False, want_iters=False, want_smooth=False)[3]
    assert not np.array_equal(want, ctx.mandelbrot_rgba8(B.mandelbrot_params(w, h, max_iter=300, flags=B.MANDEL_COLOUR_SMOOTH)))
    share = f"distance below 1 pixel: {int((D < 1).sum())} of {w * h} pixels"
    for extra in ([], ["--gpu-postprocess"]):
        out = tmp_path / "distance.png"
        r = subprocess.run([APP, "--out", str(out), "--quiet", "--colour", "distance", "--width", str(w), "--height", str(h), "--max-iter",
                            "300"] + extra, capture_output=True, text=True, cwd=tmp_path, timeout=180)
        assert r.returncode == 0, r.stdout + r.stderr
        assert np.array_equal(np.asarray(Image.open(out).convert("RGBA")), want), extra
        assert share in r.stdout, r.stdout
    r = subprocess.run([APP, "--out", str(tmp_path / "no.png"), "--quiet", "--colour", "distance", "--supersample", "2", "--width", str(w),
                        "--height", str(h)], capture_output=True, text=True, cwd=tmp_path, timeout=180)
    assert r.returncode != 0 and "--colour distance" in r.stdout
