"""MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE on the MI355X, every comparison bit for bit: the refine stage through the blocking call's report
and image (empty lists, full lists, lists and planes that end inside a wave and inside a block), the images in every precision against
the rule's restatement on the library's OWN plain smooth plane and the host resolve of the library's OWN grid plane, the ranked form
against its composition by hand, the anchor fact, narrow images, repeatability, the all-interior identity, every refusal, the warm-up, the
zoom sequence, the app end to end, and the existing paths before and after the chain ran on the same context."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mandel_adaptive_smooth_ref as A
import mandel_smooth_equalise_ref as Q
import mandel_smooth_ref as S
from test_gpu_mandel_equalise import bound_view, six_views

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "mandelbrot")
INVALID, UNSUPPORTED = 1, 5
TAUS = [0, 64, 256, 2**32 - 1]
WORD = "MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want, what=""):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g, w), (what, int((g != w).any(axis=-1).sum()), "pixels differ")


def colouring(B, ranked):
    return B.MANDEL_COLOUR_SMOOTH_EQUALISED if ranked else B.MANDEL_COLOUR_SMOOTH


def flagged(B, w, h, s, ranked=False, **kw):
    return B.mandelbrot_params(w, h, flags=colouring(B, ranked) | kw.pop("flags", 0), supersample=s, adaptive_smooth=True, **kw)


def parts(ctx, B, p, s, ranked):
    """What the image is made of, from the library's existing calls: the plain smooth plane, the plain image (the colouring alone), and the
    host resolve of the library's own grid plane (for the ranked form through the ANCHOR plane's map, composed by hand)."""
    M = p.max_iter
    g = B.supersample_params(p)
    assert g.flags & B.MANDEL_COLOUR_SMOOTH and not g.flags & (B.MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE | B.MANDEL_COLOUR_SMOOTH_EQUALISED | (15 << 8))
    grid_q = ctx.mandelbrot_smooth(g, want_rgba=False, want_iters=False)[2]
    one = B.MandelbrotParams.from_buffer_copy(bytes(p))
    one.flags = B.MANDEL_COLOUR_SMOOTH
    q = ctx.mandelbrot_smooth(one, want_rgba=False, want_iters=False)[2]
    assert np.array_equal(A.anchor(grid_q, s), q), "the anchor fact"
    one.flags = colouring(B, ranked)
    plain = ctx.mandelbrot(one, want_iters=False)[0]
    qmap = B.smooth_equalise_map(M, Q.histogram(q, M)) if ranked else None
    full = B.resolve_smooth(M, s, grid_q, qmap, k_color=tuple(p.k_color))
    return q, plain, full


def check_image(ctx, B, p, s, ranked, taus, what):
    """Every tau of one case; returns [(tau, share, image)]."""
    W, H, M = p.width, p.height, p.max_iter
    q, plain, full = parts(ctx, B, p, s, ranked)
    out = []
    for tau in taus:
        mask = A.refine(q, M, tau)
        want = np.where(mask[..., None], full, plain)
        img = ctx.mandelbrot_adaptive_smooth(p, tau)
        assert ctx.last_refined() == (int(mask.sum()), W * H), (what, tau)
        assert ctx.last_timing()[0] > 0
        same(img[mask], full[mask], (what, tau, "refined"))
        same(img[~mask], plain[~mask], (what, tau, "unrefined"))
        img8 = ctx.mandelbrot_adaptive_smooth(p, tau, rgba8=True)
        assert ctx.last_refined() == (int(mask.sum()), W * H)
        assert np.array_equal(img8, ctx.convert_rgba8(want, 255.0)), (what, tau)
        out.append((tau, mask.mean(), img))
    return out, full


def full_call(ctx, B, p):
    """The full MC_MANDEL_SUPERSAMPLE_SMOOTH image of the same request."""
    f = B.MandelbrotParams.from_buffer_copy(bytes(p))
    f.flags = (f.flags & ~B.MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE) | B.MANDEL_SUPERSAMPLE_SMOOTH
    return ctx.mandelbrot(f, want_iters=False)[0]


# ---- the refine stage, through the report and the image ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(48, 32), (50, 13), (64, 5), (7, 9), (256, 1), (257, 1)], ids=str)
def test_refine_stage(ctx, B, shape):
    """48 x 32: whole blocks; 50 x 13 = 650 pixels: the plane ends inside a wave and inside a block; 64 x 5: at a wave's end inside a
    block; 7 x 9: inside the first wave.  tau = 2^32 - 1 and 256 M: the empty list; tau = 0 on this exterior view: every pixel."""
    W, H = shape
    M = 200
    kw = dict(max_iter=M, centre=(0.45, 0.4), scale=(0.1, 0.1))           # nearly all exterior: q varies from pixel to pixel
    p = flagged(B, W, H, 2, **kw)
    res, _ = check_image(ctx, B, p, 2, False, [0, 1, 64, 256, 1024, 256 * M - 1, 256 * M, 2**32 - 1], shape)
    share = dict((t, sh) for t, sh, _ in res)
    assert share[2**32 - 1] == 0 and share[256 * M] == 0
    if H > 1:                                                              # (a condition on the view: the restatement gives it for these shapes)
        assert share[0] == 1.0, "the view was chosen so that every pixel differs from a neighbour"
    else:
        assert 0.9 < share[0] < 1.0
    counts = sorted(set(int(round(sh * W * H)) for sh in share.values()))
    print(shape, "list lengths:", counts)


def test_list_lengths_end_inside_a_wave(ctx, B):
    """List lengths that are no multiple of the entries per wave (16, 4, 1 at s = 2, 4, 8) nor of a block: the default view's lists."""
    W, H, M = 48, 32, 200
    seen = set()
    for s in (2, 4):
        res, _ = check_image(ctx, B, flagged(B, W, H, s, max_iter=M), s, False, [64, 256, 1000], s)
        seen |= {int(round(sh * W * H)) for _, sh, _ in res}
    assert any(n % 16 for n in seen) and any(n % 4 for n in seen) and any(n % 256 for n in seen), seen


# ---- images in every precision -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ranked", [False, True], ids=["smooth", "ranked"])
@pytest.mark.parametrize("precision", ["f32", "ds", "f64"])
def test_images_plain_precisions(ctx, B, precision, ranked):
    W, H, M = 48, 32, 200
    prec = dict(f32=B.PRECISION_F32, ds=B.PRECISION_DS, f64=B.PRECISION_F64)[precision]
    real = False
    for s in (2, 4, 8) if precision == "f64" else (2, 4):
        p = flagged(B, W, H, s, ranked, max_iter=M, precision=prec)
        res, full = check_image(ctx, B, p, s, ranked, TAUS, (precision, s, ranked))
        at = dict((t, img) for t, _, img in res)
        same(ctx.mandelbrot(p, want_iters=False)[0], at[256], "the flag route is the explicit call at tau = 256")
        assert np.array_equal(ctx.mandelbrot_rgba8(p), ctx.mandelbrot_adaptive_smooth(p, 256, rgba8=True))
        assert ctx.last_refined()[1] == W * H
        fc = full_call(ctx, B, p)
        if not ranked:
            same(fc, full, "the full call is the host resolve of the grid plane")
        real |= any(0 < sh < 1 and not np.array_equal(bits(img), bits(fc)) for _, sh, img in res)
    assert real, "a share strictly inside (0, 1) and an image unequal to the full call's"


@pytest.mark.parametrize("which", ["perturb", "perturb-bla", "perturb-bla-deep", "perturb-deep-orbit"])
def test_images_perturbation_precisions(ctx, B, which):
    W, H, s = 48, 32, 2
    name, kw, make = six_views(B)[dict(perturb=3, **{"perturb-bla": 4, "perturb-bla-deep": 5, "perturb-deep-orbit": 5})[which]]
    if which == "perturb-deep-orbit":
        kw = dict(kw, precision=B.PRECISION_PERTURB)                       # a deep orbit bound: PERTURB renders by the deep kernel
    real = False
    with bound_view(B, ctx, kw, make):
        for ranked in (False, True):
            p = flagged(B, W, H, s, ranked, **kw)
            res, full = check_image(ctx, B, p, s, ranked, TAUS, (which, ranked))
            same(ctx.mandelbrot(p, want_iters=False)[0], dict((t, img) for t, _, img in res)[256], "the flag route")
            assert np.array_equal(ctx.mandelbrot_rgba8(p), ctx.mandelbrot_adaptive_smooth(p, 256, rgba8=True))
            fc = full_call(ctx, B, p)
            real |= any(0 < sh < 1 and not np.array_equal(bits(img), bits(fc)) for _, sh, img in res)
    assert real, "a share strictly inside (0, 1) and an image unequal to the full call's"


def test_ranked_unrefined_pixels_are_the_plain_ranked_image(ctx, B):
    """The composition by hand, spelled out once: anchor histogram -> mc_mandelbrot_smooth_equalise_map -> host resolve with that qmap;
    and that map is NOT the full ranked call's."""
    W, H, M, s = 48, 32, 200, 4
    p = flagged(B, W, H, s, True, max_iter=M)
    q = ctx.mandelbrot_smooth(B.mandelbrot_params(W, H, max_iter=M, flags=B.MANDEL_COLOUR_SMOOTH), want_rgba=False, want_iters=False)[2]
    grid_q = ctx.mandelbrot_smooth(B.supersample_params(p), want_rgba=False, want_iters=False)[2]
    hist = Q.histogram(q, M)
    assert np.array_equal(hist, Q.histogram(A.anchor(grid_q, s), M))
    qmap = B.smooth_equalise_map(M, hist)
    mask = A.refine(q, M, 256)
    img = ctx.mandelbrot(p, want_iters=False)[0]
    same(img[mask], B.resolve_smooth(M, s, grid_q, qmap)[mask], "refined")
    same(img[~mask], ctx.mandelbrot(B.mandelbrot_params(W, H, max_iter=M, flags=B.MANDEL_COLOUR_SMOOTH_EQUALISED), want_iters=False)[0][~mask],
         "unrefined")
    assert not np.array_equal(qmap, B.smooth_equalise_map(M, Q.histogram(grid_q, M)))
    assert 0 < mask.sum() < W * H


@pytest.mark.parametrize("which", range(6), ids=["f32", "ds", "f64", "perturb", "perturb-bla", "perturb-bla-deep"])
def test_anchor_fact_on_the_device(ctx, B, which):
    name, kw, make = six_views(B)[which]
    W, H = 40, 24
    with bound_view(B, ctx, kw, make):
        q = ctx.mandelbrot_smooth(B.mandelbrot_params(W, H, flags=B.MANDEL_COLOUR_SMOOTH, **kw), want_rgba=False, want_iters=False)[2]
        for s in (2, 4):
            g = B.supersample_params(flagged(B, W, H, s, **kw))
            assert np.array_equal(A.anchor(ctx.mandelbrot_smooth(g, want_rgba=False, want_iters=False)[2], s), q), (name, s)


@pytest.mark.parametrize("W", [1, 63, 65, 257])
def test_narrow_and_odd_widths(ctx, B, W):
    """Three rows: the last partial wave of the list at s = 2 (16 entries per wave), s = 4 (4) and s = 8 (1)."""
    H, M = 3, 200
    for s in A.FACTORS:
        for ranked in (False, True):
            check_image(ctx, B, flagged(B, W, H, s, ranked, max_iter=M, centre=(0.45, 0.4), scale=(0.1, 0.1)), s, ranked, [0, 256], (W, s, ranked))


def test_two_runs_give_the_same_bytes(ctx, B):
    for ranked in (False, True):
        p = flagged(B, 96, 64, 4, ranked, max_iter=300)
        a, b = ctx.mandelbrot_adaptive_smooth(p, 64), ctx.mandelbrot_adaptive_smooth(p, 64)
        assert np.array_equal(bits(a), bits(b))
        with B.Context(0) as c2:                                           # and on a fresh context, whose list arrives in its own order
            assert np.array_equal(bits(c2.mandelbrot_adaptive_smooth(p, 64)), bits(a))
            assert c2.last_refined() == ctx.last_refined()


def test_all_interior_view_is_the_plain_image(ctx, B):
    W, H, M = 40, 24, 100
    view = dict(centre=(-0.1, 0.0), scale=(0.01, 0.01), max_iter=M)
    plain, _, q = ctx.mandelbrot_smooth(B.mandelbrot_params(W, H, flags=B.MANDEL_COLOUR_SMOOTH, **view), want_iters=False)
    assert (q == 256 * M).all()
    for s in A.FACTORS:
        for ranked in (False, True):
            same(ctx.mandelbrot(flagged(B, W, H, s, ranked, **view), want_iters=False)[0], plain, (s, ranked))
            assert ctx.last_refined() == (0, W * H)
            same(ctx.mandelbrot_adaptive_smooth(flagged(B, W, H, s, ranked, **view), 0), plain, (s, ranked, 0))


# ---- refusals, the warm-up, the zoom sequence, the app -------------------------------------------------------------------------------
def test_refusals(ctx, B):
    import torch
    w, h, M = 48, 32, 200
    BIT, SM, SE = B.MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE, B.MANDEL_COLOUR_SMOOTH, B.MANDEL_COLOUR_SMOOTH_EQUALISED
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
    bad = [(P(BIT | SM), "MC_MANDEL_SUPERSAMPLE(s)"), (P(BIT | SM, supersample=1), "MC_MANDEL_SUPERSAMPLE(s)"), (P(BIT), "MC_MANDEL_SUPERSAMPLE(s)"),
           (P(BIT, supersample=2), "exactly one"), (P(BIT | SM | SE, supersample=2), "exactly one"),
           (P(BIT | SM, supersample=3), "MC_MANDEL_SUPERSAMPLE(s)"),
           (P(BIT | SM, supersample=2, adaptive=True), "MC_MANDEL_SUPERSAMPLE_ADAPTIVE"),
           (P(BIT | SM, supersample=2, smooth_samples=True), "MC_MANDEL_SUPERSAMPLE_SMOOTH (that bit"),
           (P(BIT | SE, supersample=2, smooth_samples=True, adaptive=True), "does not combine"),
           (P(BIT | SM | B.MANDEL_COLOUR_EQUALISED, supersample=2), "MC_MANDEL_COLOUR_EQUALISED"),
           (P(BIT | SM | B.MANDEL_COLOUR_DISTANCE, supersample=2), "MC_MANDEL_COLOUR_DISTANCE"),
           (P(BIT | SE | B.MANDEL_COLOUR_DISTANCE, supersample=2), "MC_MANDEL_COLOUR_DISTANCE"),
           (P(BIT | SM | B.MANDEL_ITERS_U16, supersample=2), "MC_MANDEL_ITERS_U16"), (P(BIT | SM | B.MANDEL_FMA, supersample=2), "MC_MANDEL_FMA"),
           (P(BIT | SM, supersample=2, row_begin=4), "whole image"), (P(BIT | SM, supersample=2, row_end=16), "whole image"),
           (P(BIT | SE, supersample=2, row_block=2, row_stride=6), "whole image")]
    for p, word in bad:
        refused(lambda: ctx.mandelbrot(p, want_iters=False), says=[WORD, word])
        refused(lambda: ctx.mandelbrot_rgba8(p), says=[WORD, word])
        refused(lambda: ctx.mandelbrot_adaptive_smooth(p, 256), says=[WORD, word])
        assert L.mc_context_warmup_mandelbrot(ctx._h, C.byref(p), 1) == INVALID
        assert WORD in L.mc_last_error_detail().decode()
    big = flagged(B, 8, 8, 2, max_iter=S.MAX_ITER_LIMIT + 1, centre=(2.0, 2.0), scale=(0.1, 0.1))
    refused(lambda: ctx.mandelbrot(big, want_iters=False), says=[WORD, "2^24 - 1"])
    ok, okr = flagged(B, w, h, 2, max_iter=M), flagged(B, w, h, 2, True, max_iter=M)
    refused(lambda: ctx.mandelbrot(ok), says=["out_iters", WORD])
    refused(lambda: ctx.mandelbrot(ok, want_rgba=False), says="out_iters")
    refused(lambda: ctx.mandelbrot_adaptive_smooth(P(SM, supersample=2, smooth_samples=True), 256), says="must carry " + WORD)
    assert L.mc_mandelbrot_render_adaptive_smooth(ctx._h, C.byref(ok), 256, None, None) == INVALID
    assert "at least one" in L.mc_last_error_detail().decode()
    # bits 5 and 13 together, without the bit, stay refused with the same words
    refused(lambda: ctx.mandelbrot(P(SM, supersample=2, smooth_samples=True, adaptive=True), want_iters=False),
            says=["MC_MANDEL_SUPERSAMPLE_SMOOTH does not combine with MC_MANDEL_SUPERSAMPLE_ADAPTIVE (adaptive refinement compares integer counts)"])
    # every other call refuses the bit by name
    for p in (ok, okr):
        others = [lambda: ctx.mandelbrot_device(p, d_rgba.data_ptr(), d_it.data_ptr()), lambda: ctx.mandelbrot_banded(p, 16),
                  lambda: ctx.mandelbrot_smooth(p), lambda: ctx.mandelbrot_smooth_device(p, d_rgba.data_ptr(), 0, d_it.data_ptr()),
                  lambda: ctx.mandelbrot_distance(p), lambda: ctx.mandelbrot_distance_device(p, d_it.data_ptr(), 1.0, 0, d_rgba.data_ptr()),
                  lambda: ctx.mandelbrot_smooth_equalised(p), lambda: ctx.mandelbrot_recolour_device(p, d_it.data_ptr(), 4, ident >> 8, d_rgba.data_ptr()),
                  lambda: ctx.mandelbrot_resolve_device(p, d_it.data_ptr(), 4, None, d_rgba.data_ptr()),
                  lambda: ctx.mandelbrot_resolve_smooth_device(p, d_it.data_ptr(), None, d_rgba.data_ptr()),
                  lambda: ctx.mandelbrot_resolve_smooth_device(p, d_it.data_ptr(), ident, d_rgba.data_ptr()),
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


def test_render_after_a_warm_up_with_the_bit(ctx, B):
    L = B.lib()
    L.mc_context_warmup_mandelbrot.argtypes = [C.c_void_p, C.POINTER(B.MandelbrotParams), C.c_int]
    for ranked in (False, True):
        for prec in (B.PRECISION_F32, B.PRECISION_F64):
            p = flagged(B, 40, 24, 4, ranked, max_iter=128, precision=prec)
            want = ctx.mandelbrot(p, want_iters=False)[0]
            with B.Context(0) as c2:
                for how in (0, 1, 3):
                    assert L.mc_context_warmup_mandelbrot(c2._h, C.byref(p), how) == 0, L.mc_last_error_detail()
                same(c2.mandelbrot(p, want_iters=False)[0], want, ("after the warm-up", ranked))
                assert np.array_equal(c2.mandelbrot_rgba8(p), ctx.mandelbrot_rgba8(p))


@pytest.mark.parametrize("ranked", [False, True], ids=["smooth", "ranked"])
def test_zoom_keyframe(ctx, B, ranked):
    W, H, M = 48, 32, 128
    p = flagged(B, W, H, 2, ranked, max_iter=M)
    want = ctx.mandelbrot(p, want_iters=False)[0]
    with ctx.zoom(W, H) as z:
        z.push(p)
        f, f8 = z.frame(1.0, want_rgba8=True)
        same(f, want, "the frame at r = 1")
        assert np.array_equal(f8, ctx.mandelbrot_rgba8(p))


def test_app(ctx, B, tmp_path):
    from PIL import Image
    w, h = 96, 64
    for colour, ranked in (("smooth", False), ("smooth-equalised", True)):
        p = flagged(B, w, h, 2, ranked, max_iter=300)
        for opt, tau in (("--adaptive-smooth", 256), ("--adaptive-smooth=64", 64)):
            want = ctx.mandelbrot_adaptive_smooth(p, tau, rgba8=True)
            refined, pixels = ctx.last_refined()
            for extra in ([], ["--gpu-postprocess"]):
                out = tmp_path / (colour + ".png")
                r = subprocess.run([APP, "--out", str(out), "--quiet", "--colour", colour, "--supersample", "2", opt, "--width", str(w),
                                    "--height", str(h), "--max-iter", "300"] + extra, capture_output=True, text=True, cwd=tmp_path, timeout=180)
                assert r.returncode == 0, r.stdout + r.stderr
                assert f"refined {refined} of {pixels} pixels (threshold {tau})" in r.stdout, r.stdout
                assert np.array_equal(np.asarray(Image.open(out).convert("RGBA")), want), (colour, opt, extra)
    out = tmp_path / "zoom.png"
    r = subprocess.run([APP, "--out", str(out), "--quiet", "--colour", "smooth", "--supersample", "2", "--adaptive-smooth", "--width", str(w),
                        "--height", str(h), "--zoom", "1", "2"], capture_output=True, text=True, cwd=tmp_path, timeout=180)
    assert r.returncode == 0 and len(list(tmp_path.glob("zoom_*.png"))) == 3, r.stdout + r.stderr


# ---- the existing paths, on a context the chain has run on (it swaps table slots) ------------------------------------------------------
def test_existing_paths_are_unchanged_by_the_chain(B):
    W, H, M = 48, 32, 200
    SM = B.MANDEL_COLOUR_SMOOTH
    requests = {
        "plain": lambda c: c.mandelbrot(B.mandelbrot_params(W, H, max_iter=M)),
        "plain f64": lambda c: c.mandelbrot(B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_F64)),
        "smooth": lambda c: c.mandelbrot_smooth(B.mandelbrot_params(W, H, max_iter=M, flags=SM)),
        "bit 13": lambda c: c.mandelbrot(B.mandelbrot_params(W, H, max_iter=M, flags=SM, supersample=2, smooth_samples=True), want_iters=False),
        "bit 5": lambda c: c.mandelbrot(B.mandelbrot_params(W, H, max_iter=M, supersample=2, adaptive=True), want_iters=False),
        "grid plain": lambda c: c.mandelbrot(B.mandelbrot_params(2 * W, 2 * H, max_iter=M)),
    }

    def run(c):
        return {k: [None if a is None else np.ascontiguousarray(a).view(np.uint32).copy() for a in f(c)] for k, f in requests.items()}

    def equal(a, b):
        return all((x is None and y is None) or np.array_equal(x, y) for k in a for x, y in zip(a[k], b[k]))

    with B.Context(0) as c:
        before = run(c)
        bit5 = c.last_refined()
        for ranked in (False, True):
            for prec in (B.PRECISION_F32, B.PRECISION_F64):
                c.mandelbrot_adaptive_smooth(flagged(B, W, H, 2, ranked, max_iter=M, precision=prec), 256)
            assert equal(run(c), before), ranked
            assert c.last_refined() == bit5                                # (the last adaptive render of run() is bit 5's)
        for name, f in requests.items():                                   # and interleaved with it, one by one
            c.mandelbrot_adaptive_smooth(flagged(B, W, H, 2, False, max_iter=M), 0)
            got = [None if a is None else np.ascontiguousarray(a).view(np.uint32) for a in f(c)]
            assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(got, before[name])), name
