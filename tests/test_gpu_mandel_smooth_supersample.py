"""MC_MANDEL_SUPERSAMPLE_SMOOTH on the MI355X, every comparison bit for bit: the resolve kernel alone against the host call on random
smooth planes (every factor, both forms, widths that make unaligned sample rows, heads and tails, counts above 256 M, guard rows, the
grid's row-stride loop), the whole-image calls in every precision against the host resolve of the library's OWN smooth plane of the sample
grid, the ranked chain against its composition by hand, bands and tiles, the all-interior identity, every refusal, the zoom sequence, the
warm-up, the app end to end."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mandel_smooth_equalise_ref as Q
import mandel_smooth_ref as S
import mandel_smooth_supersample_ref as X
from test_gpu_mandel_equalise import bound_view, six_views

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "mandelbrot")
INVALID, UNSUPPORTED = 1, 5
WIDTHS = [1, 2, 3, 5, 63, 64, 65, 129, 257]
ROWS = [1, 3, 5]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want, what=""):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g, w), (what, int((g != w).any(axis=-1).sum()), "pixels differ")


def flagged(B, w, h, s, ranked=False, **kw):
    colour = B.MANDEL_COLOUR_SMOOTH_EQUALISED if ranked else B.MANDEL_COLOUR_SMOOTH
    return B.mandelbrot_params(w, h, flags=colour | kw.pop("flags", 0), supersample=s, smooth_samples=True, **kw)


def upload(values, offset=0):
    """A torch device plane of the uint32 counts, `offset` elements into its allocation (offset = 1: a pointer aligned to 4 only)."""
    import torch
    a = np.ascontiguousarray(values, np.uint32).reshape(-1)
    buf = torch.zeros(a.size + offset, dtype=torch.int32, device="cuda")
    buf[offset:] = torch.from_numpy(a.view(np.int32)).cuda()
    return buf, buf[offset:]


def device_resolve(ctx, p, plane, qmap, rows, offset=0):
    """The kernel's colours of the tile, with a guard row on either side of the output checked unchanged."""
    import torch
    keep, d = upload(plane, offset)
    W = p.width
    out = torch.full((rows + 2, W, 4), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.mandelbrot_resolve_smooth_device(p, d.data_ptr(), qmap, out[1:].data_ptr())
    ctx.synchronize()
    got = out.cpu().numpy()
    assert (got[0] == -1.0).all() and (got[-1] == -1.0).all(), "guard rows"
    del keep
    return got[1:-1]


# ---- the resolve kernel alone -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ranked", [False, True], ids=["smooth", "ranked"])
@pytest.mark.parametrize("s", X.FACTORS)
def test_kernel_is_the_host_call(ctx, B, s, ranked):
    M = 1000
    top = 256 * M
    rng = np.random.default_rng(10 * s + ranked)
    maps = X.knot_maps(rng, M)[1:3] if ranked else [("none", None)]        # random knots, and runs of coinciding knots
    for W in WIDTHS:
        for rows in ROWS:
            p = flagged(B, W, rows, s, ranked, max_iter=M)
            plane = X.seeded_plane(rng, rows, W, s, M)
            wild = plane.astype(np.int64).reshape(-1)                     # some counts above 256 M, and 0xffffffff: interior
            pick = rng.random(wild.size)
            wild[pick < 0.1] = top + 1 + rng.integers(0, 5000, int((pick < 0.1).sum()))
            wild[(pick >= 0.1) & (pick < 0.15)] = 0xffffffff
            wild = wild.astype(np.uint32).reshape(plane.shape)
            for name, qmap in maps:
                for offset in (0, 1):
                    want = B.resolve_smooth(M, s, np.minimum(wild, top), qmap)
                    same(device_resolve(ctx, p, wild, qmap, rows, offset), want, (W, rows, name, offset))


@pytest.mark.parametrize("ranked", [False, True], ids=["smooth", "ranked"])
def test_kernel_on_interleaved_tiles_and_many_rows(ctx, B, ranked):
    M = 300
    rng = np.random.default_rng(77 + ranked)
    qmap = X.knot_maps(rng, M)[1][1] if ranked else None
    p = flagged(B, 65, 37, 2, ranked, max_iter=M, row_begin=8, row_block=8, row_stride=24)   # rows 8 .. 15 and 32 .. 36
    rows = B.tile_rows(p)
    assert rows == 13
    plane = X.seeded_plane(rng, rows, 65, 2, M)
    same(device_resolve(ctx, p, plane, qmap, rows), B.resolve_smooth(M, 2, plane, qmap), "interleaved")
    rows = 65537                                                          # more rows than the grid's second dimension holds
    p = flagged(B, 1, rows, 2, ranked, max_iter=M)
    plane = X.seeded_plane(rng, rows, 1, 2, M)
    same(device_resolve(ctx, p, plane, qmap, rows), B.resolve_smooth(M, 2, plane, qmap), "65537 rows")


# ---- the chain against the host resolve of the library's own smooth plane ------------------------------------------------------------
def grid_plane(ctx, B, p):
    """The library's own smooth plane of p's sample grid (the existing suites pin it to the restatements)."""
    g = B.supersample_params(p)
    assert g.flags & B.MANDEL_COLOUR_SMOOTH and not g.flags & (B.MANDEL_SUPERSAMPLE_SMOOTH | B.MANDEL_COLOUR_SMOOTH_EQUALISED | (15 << 8))
    return ctx.mandelbrot_smooth(g, want_rgba=False, want_iters=False)[2]


def check_chain(ctx, B, p, s, M, what):
    q = grid_plane(ctx, B, p)
    ranked = bool(p.flags & B.MANDEL_COLOUR_SMOOTH_EQUALISED)
    qmap = B.smooth_equalise_map(M, Q.histogram(q, M)) if ranked else None   # by hand: the ref histogram of ALL samples, the library's map
    want = B.resolve_smooth(M, s, q, qmap, k_color=tuple(p.k_color))
    rgba, _ = ctx.mandelbrot(p, want_iters=False)
    same(rgba, want, what)
    kms, cms = ctx.last_timing()
    assert kms > 0
    assert np.array_equal(ctx.mandelbrot_rgba8(p), ctx.convert_rgba8(want, 255.0)), what
    return q, want


@pytest.mark.parametrize("ranked", [False, True], ids=["smooth", "ranked"])
@pytest.mark.parametrize("precision", ["f32", "ds", "f64"])
def test_chain_plain_precisions(ctx, B, precision, ranked):
    W, H, M = 48, 32, 200
    prec = dict(f32=B.PRECISION_F32, ds=B.PRECISION_DS, f64=B.PRECISION_F64)[precision]
    for s in (2, 4):
        p = flagged(B, W, H, s, ranked, max_iter=M, precision=prec)
        q, want = check_chain(ctx, B, p, s, M, (precision, s, ranked))
        assert len(np.unique(q)) > 300 and (q == 256 * M).any()           # a real picture: escaped and interior samples
        one = ctx.mandelbrot(B.mandelbrot_params(W, H, max_iter=M, precision=prec, flags=p.flags & (B.MANDEL_COLOUR_SMOOTH | B.MANDEL_COLOUR_SMOOTH_EQUALISED)),
                             want_iters=False)[0]
        assert not np.array_equal(bits(one), bits(want))                  # and not the 1-sample image


@pytest.mark.parametrize("which", ["perturb", "perturb-bla", "perturb-bla-deep", "perturb-deep-orbit"])
def test_chain_perturbation_precisions(ctx, B, which):
    W, H, s = 24, 16, 2
    name, kw, make = six_views(B)[dict(perturb=3, **{"perturb-bla": 4, "perturb-bla-deep": 5, "perturb-deep-orbit": 5})[which]]
    if which == "perturb-deep-orbit":
        kw = dict(kw, precision=B.PRECISION_PERTURB)                       # a deep orbit bound: PERTURB renders by the deep kernel
    M = kw["max_iter"]
    with bound_view(B, ctx, kw, make):
        for ranked in (False, True):
            check_chain(ctx, B, flagged(B, W, H, s, ranked, **kw), s, M, (which, ranked))


def test_tiles_and_bands_are_the_whole_images_rows(ctx, B):
    W, H, M = 48, 32, 200
    for s in (2, 4):
        whole, _ = ctx.mandelbrot(flagged(B, W, H, s, max_iter=M), want_iters=False)
        whole8 = ctx.mandelbrot_rgba8(flagged(B, W, H, s, max_iter=M))
        tile, _ = ctx.mandelbrot(flagged(B, W, H, s, max_iter=M, row_begin=5, row_end=17), want_iters=False)
        same(tile, whole[5:17], ("rows", s))
        p = flagged(B, W, H, s, max_iter=M, row_begin=2, row_block=2, row_stride=6)
        rows = [2 + 6 * k + j for k in range(6) for j in range(2) if 2 + 6 * k + j < H]
        inter, _ = ctx.mandelbrot(p, want_iters=False)
        assert B.tile_rows(p) == len(rows)
        same(inter, whole[rows], ("interleaved", s))
        band = ctx.mandelbrot_rgba8(flagged(B, W, H, s, max_iter=M, row_begin=8, row_end=19))
        assert np.array_equal(band, whole8[8:19]), s


def test_all_interior_view_is_the_plain_smooth_image(ctx, B):
    W, H, M = 40, 24, 100
    view = dict(centre=(-0.1, 0.0), scale=(0.01, 0.01), max_iter=M)
    plain, _, q = ctx.mandelbrot_smooth(B.mandelbrot_params(W, H, flags=B.MANDEL_COLOUR_SMOOTH, **view), want_iters=False)
    assert (q == 256 * M).all()
    for s in X.FACTORS:
        for ranked in (False, True):
            same(ctx.mandelbrot(flagged(B, W, H, s, ranked, **view), want_iters=False)[0], plain, (s, ranked))


# ---- refusals, the zoom sequence, the warm-up, the app -------------------------------------------------------------------------------
def test_refusals(ctx, B):
    import torch
    w, h, M = 48, 32, 200
    BIT, SM, SE = B.MANDEL_SUPERSAMPLE_SMOOTH, B.MANDEL_COLOUR_SMOOTH, B.MANDEL_COLOUR_SMOOTH_EQUALISED
    WORD = "MC_MANDEL_SUPERSAMPLE_SMOOTH"
    d_rgba = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    d_it = torch.zeros((4 * h, 4 * w), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L = B.lib()
    L.mc_context_warmup_mandelbrot.argtypes = [C.c_void_p, C.POINTER(B.MandelbrotParams), C.c_int]

    def refused(call, status=INVALID, says=None):
        with pytest.raises(B.McError) as e:
            call()
        assert e.value.status == status, e.value
        for word in ([says] if isinstance(says, str) else says or []):
            assert word in str(e.value), e.value

    P = lambda flags, **kw: B.mandelbrot_params(w, h, max_iter=M, flags=flags, **kw)
    ident = 256 * np.arange(M + 1, dtype=np.uint32)
    # the bit alone, with s <= 1, with neither or both colourings, with what it does not combine with: the calls that honour it, by name
    bad = [(P(BIT | SM), "MC_MANDEL_SUPERSAMPLE(s)"), (P(BIT | SM, supersample=1), "MC_MANDEL_SUPERSAMPLE(s)"), (P(BIT), "MC_MANDEL_SUPERSAMPLE(s)"),
           (P(BIT, supersample=2), "exactly one"), (P(BIT | SM | SE, supersample=2), "exactly one"),
           (P(BIT | SM, supersample=3), "MC_MANDEL_SUPERSAMPLE(s)"),
           (P(BIT | SM, supersample=2, adaptive=True), "MC_MANDEL_SUPERSAMPLE_ADAPTIVE"),
           (P(BIT | SM | B.MANDEL_COLOUR_EQUALISED, supersample=2), "MC_MANDEL_COLOUR_EQUALISED"),
           (P(BIT | SM | B.MANDEL_COLOUR_DISTANCE, supersample=2), "MC_MANDEL_COLOUR_DISTANCE"),
           (P(BIT | SE | B.MANDEL_COLOUR_DISTANCE, supersample=2), "MC_MANDEL_COLOUR_DISTANCE"),
           (P(BIT | SM | B.MANDEL_ITERS_U16, supersample=2), "MC_MANDEL_ITERS_U16"), (P(BIT | SM | B.MANDEL_FMA, supersample=2), "MC_MANDEL_FMA")]
    for p, word in bad:
        refused(lambda: ctx.mandelbrot(p, want_iters=False), says=[WORD, word])
        refused(lambda: ctx.mandelbrot_rgba8(p), says=[WORD, word])
        refused(lambda: ctx.mandelbrot_resolve_smooth_device(p, d_it.data_ptr(), None, d_rgba.data_ptr()), says=[WORD, word])
        assert L.mc_context_warmup_mandelbrot(ctx._h, C.byref(p), 1) == INVALID
    big = flagged(B, 8, 8, 2, max_iter=S.MAX_ITER_LIMIT + 1, centre=(2.0, 2.0), scale=(0.1, 0.1))
    refused(lambda: ctx.mandelbrot(big, want_iters=False), says=[WORD, "2^24 - 1"])
    # out_iters; the ranked form's tiles and bands; interleaved tiles of render_rgba8; the stage's own rules
    ok, okr = flagged(B, w, h, 2, max_iter=M), flagged(B, w, h, 2, True, max_iter=M)
    refused(lambda: ctx.mandelbrot(ok), says="out_iters")
    refused(lambda: ctx.mandelbrot(ok, want_rgba=False), says="out_iters")
    refused(lambda: ctx.mandelbrot(flagged(B, w, h, 2, True, max_iter=M, row_begin=4), want_iters=False), says="MC_MANDEL_COLOUR_SMOOTH_EQUALISED")
    refused(lambda: ctx.mandelbrot_rgba8(flagged(B, w, h, 2, True, max_iter=M, row_end=16)), says="MC_MANDEL_COLOUR_SMOOTH_EQUALISED")
    refused(lambda: ctx.mandelbrot_rgba8(flagged(B, w, h, 2, max_iter=M, row_block=2, row_stride=6)))
    refused(lambda: ctx.mandelbrot_resolve_smooth_device(ok, d_it.data_ptr(), ident, d_rgba.data_ptr()), says="qmap")
    refused(lambda: ctx.mandelbrot_resolve_smooth_device(okr, d_it.data_ptr(), None, d_rgba.data_ptr()), says="qmap")
    refused(lambda: ctx.mandelbrot_resolve_smooth_device(okr, d_it.data_ptr(), ident[::-1].copy(), d_rgba.data_ptr()), says="qmap[")
    refused(lambda: ctx.mandelbrot_resolve_smooth_device(P(SM, supersample=2), d_it.data_ptr(), None, d_rgba.data_ptr()), says="must carry " + WORD)
    refused(lambda: ctx.mandelbrot_resolve_smooth_device(ok, d_it.data_ptr() + 2, None, d_rgba.data_ptr()))
    refused(lambda: ctx.mandelbrot_resolve_smooth_device(ok, d_it.data_ptr(), None, d_rgba.data_ptr() + 8))
    refused(lambda: ctx.mandelbrot_resolve_smooth_device(ok, 0, None, d_rgba.data_ptr()))
    # the two old pairs stay refused, with their words, and now name the bit
    refused(lambda: ctx.mandelbrot(P(SM, supersample=2)), says=["MC_MANDEL_COLOUR_SMOOTH does not combine", "MC_MANDEL_SUPERSAMPLE", WORD])
    refused(lambda: ctx.mandelbrot(P(SE, supersample=2)), says=["MC_MANDEL_COLOUR_SMOOTH_EQUALISED does not combine", "MC_MANDEL_SUPERSAMPLE", WORD])
    # every other call refuses the bit by name
    for p in (ok, okr):
        others = [lambda: ctx.mandelbrot_device(p, d_rgba.data_ptr(), d_it.data_ptr()), lambda: ctx.mandelbrot_banded(p, 16),
                  lambda: ctx.mandelbrot_smooth(p), lambda: ctx.mandelbrot_smooth_device(p, d_rgba.data_ptr(), 0, d_it.data_ptr()),
                  lambda: ctx.mandelbrot_distance(p), lambda: ctx.mandelbrot_distance_device(p, d_it.data_ptr(), 1.0, 0, d_rgba.data_ptr()),
                  lambda: ctx.mandelbrot_smooth_equalised(p), lambda: ctx.mandelbrot_recolour_device(p, d_it.data_ptr(), 4, ident >> 8, d_rgba.data_ptr()),
                  lambda: ctx.mandelbrot_resolve_device(p, d_it.data_ptr(), 4, None, d_rgba.data_ptr()),
                  lambda: ctx.mandelbrot_assemble_device(p, d_it.data_ptr(), 4, 1, 8, h, d_rgba.data_ptr()),
                  lambda: ctx.mandelbrot_smooth_remap_device(p, d_it.data_ptr(), ident, 0, d_rgba.data_ptr()),
                  lambda: ctx.zoom_compose_counts_device(p, d_it.data_ptr(), 0, None, 0.75, d_rgba.data_ptr()),
                  lambda: B.zoom_compose_counts(p, np.zeros((h, w), np.uint32), None, None, 0.75)]
        for call in others:
            refused(call, says=WORD)
        with ctx.zoom_counts(w, h) as z:
            refused(lambda: z.push(p), says=WORD)
        with B.Multi(1) as mm:
            refused(lambda: mm.mandelbrot(p), UNSUPPORTED, WORD)
            refused(lambda: mm.mandelbrot_rgba8(p), UNSUPPORTED, WORD)
    # after all that the context still renders plain and smooth images
    lut = B.colour_lut(M)
    rgba, n = ctx.mandelbrot(B.mandelbrot_params(w, h, max_iter=M))
    assert np.array_equal(bits(rgba), bits(lut[n]))
    rgba, n2, q = ctx.mandelbrot_smooth(P(SM))
    assert np.array_equal(n, n2) and np.array_equal(bits(rgba), bits(S.colour(q, M, lut)))


@pytest.mark.parametrize("ranked", [False, True], ids=["smooth", "ranked"])
def test_zoom_keyframe(ctx, B, ranked):
    W, H, M = 48, 32, 128
    p = flagged(B, W, H, 2, ranked, max_iter=M)
    want, _ = ctx.mandelbrot(p, want_iters=False)
    with ctx.zoom(W, H) as z:
        z.push(p)
        f, f8 = z.frame(1.0, want_rgba8=True)
        same(f, want, "the frame at r = 1")
        assert np.array_equal(f8, ctx.mandelbrot_rgba8(p))


def test_render_after_a_warm_up_with_the_bit(ctx, B):
    L = B.lib()
    L.mc_context_warmup_mandelbrot.argtypes = [C.c_void_p, C.POINTER(B.MandelbrotParams), C.c_int]
    for ranked in (False, True):
        p = flagged(B, 40, 24, 4, ranked, max_iter=128, precision=B.PRECISION_F64)
        want, _ = ctx.mandelbrot(p, want_iters=False)
        with B.Context(0) as c2:
            for how in (0, 1, 3):
                assert L.mc_context_warmup_mandelbrot(c2._h, C.byref(p), how) == 0
            same(c2.mandelbrot(p, want_iters=False)[0], want, ("after the warm-up", ranked))
            band = flagged(B, 40, 24, 4, False, max_iter=128, precision=B.PRECISION_F64, row_begin=3, row_end=11)
            assert L.mc_context_warmup_mandelbrot(c2._h, C.byref(band), 1) == 0
            assert np.array_equal(c2.mandelbrot_rgba8(band), ctx.mandelbrot_rgba8(band))


def test_app(ctx, B, tmp_path):
    from PIL import Image
    w, h = 96, 64
    for colour, ranked in (("smooth", False), ("smooth-equalised", True)):
        want = ctx.mandelbrot_rgba8(flagged(B, w, h, 2, ranked, max_iter=300))
        for extra in ([], ["--gpu-postprocess"]):
            out = tmp_path / (colour + ".png")
            r = subprocess.run([APP, "--out", str(out), "--quiet", "--colour", colour, "--supersample", "2", "--supersample-smooth", "--width", str(w),
                                "--height", str(h), "--max-iter", "300"] + extra, capture_output=True, text=True, cwd=tmp_path, timeout=180)
            assert r.returncode == 0, r.stdout + r.stderr
            assert np.array_equal(np.asarray(Image.open(out).convert("RGBA")), want), (colour, extra)
    out = tmp_path / "zoom.png"
    r = subprocess.run([APP, "--out", str(out), "--quiet", "--colour", "smooth", "--supersample", "2", "--supersample-smooth", "--width", str(w),
                        "--height", str(h), "--zoom", "1", "2"], capture_output=True, text=True, cwd=tmp_path, timeout=180)
    assert r.returncode == 0 and len(list(tmp_path.glob("zoom_*.png"))) == 3, r.stdout + r.stderr
