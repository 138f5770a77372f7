"""The area filter of zoom sequences without a GPU: the filtered host calls (the kernels' own source, compiled for the host) against
tests/mandel_zoom_filter_ref.py bit for bit, filter 0 against the unfiltered calls, the contract's identities, the weights in exact
rational arithmetic, every host refusal, the count forms in all four colourings, the app's option parsing; and what the filter is for,
measured against a direct render of each frame's own view with 8 x 8 samples per pixel."""
import ctypes as C
import functools
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import mandel_zoom_counts_ref as ZC
import mandel_zoom_filter_ref as ZF
import mandel_zoom_ref as Z
from test_mandel_zoom_counts_host import KCOLOR, frame_map, planes
from test_mandel_zoom_host import SHAPES, bits, keyframes, ratios

INVALID = 1
NAMES = ("mc_mandelbrot_zoom_compose_filtered", "mc_mandelbrot_zoom_compose_filtered_device_async",
         "mc_mandelbrot_zoom_compose_counts_filtered", "mc_mandelbrot_zoom_compose_counts_filtered_device_async",
         "mc_mandelbrot_zoom_frame_filtered", "mc_mandelbrot_zoom_counts_frame_filtered")


def test_symbols(B):
    for name in NAMES:
        assert name in B.declared_symbols() and hasattr(B.lib(), name), name
    assert (B.ZOOM_FILTER_BILINEAR, B.ZOOM_FILTER_AREA) == (0, 1) == (ZF.BILINEAR, ZF.AREA)
    assert B.lib().mc_abi_version() == 3


@pytest.mark.parametrize("W,H", SHAPES)
def test_compose_matches_restatement(B, W, H):
    for wide, deep in (keyframes(W, H), ZF.special_keyframes(W, H)):
        in_unit = float(np.nanmax(np.abs(wide))) <= 1.0
        for r in ratios(B):
            for d in (deep, None):
                want, mask = ZF.compose(wide, d, r, ZF.AREA)
                got, got8 = B.zoom_compose_filtered(wide, d, r, B.ZOOM_FILTER_AREA, want_rgba=True, want_rgba8=True)
                bad = ~ZF.same_bits(got, want)
                assert not bad.any(), (W, H, r, d is not None, int(bad.sum()), got[bad][:2], want[bad][:2])
                assert np.array_equal(got8, Z.rgba8(want)), (W, H, r, d is not None)
                only8 = B.zoom_compose_filtered(wide, d, r, B.ZOOM_FILTER_AREA, want_rgba=False, want_rgba8=True)[1]
                assert np.array_equal(only8, got8)
                if in_unit:
                    assert float(want.max()) <= 1.0                  # (the byte conversion cannot wrap)
                # outside the deep-sourced rectangle the AREA frame is the BILINEAR frame
                plain = B.zoom_compose(wide, d, r)[0]
                assert ZF.same_bits(got, plain)[~mask].all(), (W, H, r)
                assert np.array_equal(mask, Z.deep_mask(W, H, r, d is not None))


@pytest.mark.parametrize("W,H", SHAPES)
def test_filter_zero_is_the_unfiltered_call(B, W, H):
    for wide, deep in (keyframes(W, H), ZF.special_keyframes(W, H)):
        for r in ratios(B):
            for d in (deep, None):
                a, a8 = B.zoom_compose(wide, d, r, want_rgba=True, want_rgba8=True)
                b, b8 = B.zoom_compose_filtered(wide, d, r, B.ZOOM_FILTER_BILINEAR, want_rgba=True, want_rgba8=True)
                assert np.array_equal(bits(a), bits(b)) and np.array_equal(a8, b8), (W, H, r, d is not None)


@pytest.mark.parametrize("W,H", SHAPES)
def test_identities(B, W, H):
    A = B.ZOOM_FILTER_AREA
    for wide, deep in (keyframes(W, H), ZF.special_keyframes(W, H)):
        assert np.array_equal(bits(B.zoom_compose_filtered(wide, None, 1.0, A)[0]), bits(wide)), "r = 1 without deep is wide's bits"
        assert np.array_equal(bits(B.zoom_compose_filtered(wide, deep, 0.5, A)[0]), bits(deep)), "r = 0.5 is deep's bits on every pixel"
        assert np.array_equal(bits(ZF.compose(wide, deep, 0.5, ZF.AREA)[0]), bits(deep)), "and so says the restatement"
    assert Z.deep_mask(W, H, 0.5).all()


def test_constant_plane(B):
    """A constant plane, on the pixels the filter computes (the deep-sourced ones; the others are the bilinear contract's): exact where the constant is 0 or a power of two; otherwise within the roundings of nine products, eight additions
    per sum and one division, (1 + 2^-24)^19 - 1 < 2^-21 relative (the header's bound); measured and printed in ulp."""
    W, H = 67, 35
    worst = 0.0
    for c in (0.0, -0.0, 0.25, 1.0, 2.0, 0.1, 0.7, 1.0 / 3.0, 0.999999, 123.456):
        wide = np.full((H, W, 4), np.float32(c), np.float32)
        wide[..., 3] = 1.0
        for r in ratios(B) + [0.53, 0.7071, 0.99]:
            got = B.zoom_compose_filtered(wide, wide, r, B.ZOOM_FILTER_AREA)[0]
            assert ZF.same_bits(got, ZF.compose(wide, wide, r, ZF.AREA)[0]).all()
            mask = Z.deep_mask(W, H, r)
            m = abs(c)
            if m == 0.0 or math.frexp(m)[0] == 0.5:
                assert np.array_equal(bits(got)[mask], bits(wide)[mask]), (c, r)
            else:
                rel = float(np.abs(got[mask][:, :3].astype(np.float64) - np.float64(np.float32(c))).max()) / m
                worst = max(worst, rel / 2.0 ** -24)
                assert rel <= 2.0 ** -21, (c, r, rel)
    print(f"constant plane: worst relative error {worst:.2f} x 2^-24")


def test_weights_in_exact_arithmetic(B):
    """The double positions taken as exact rationals: the three cells k0 .. k0 + 2 hold the whole box (their exact overlaps sum to b - a,
    which is r2 up to the two roundings of a and b), no other cell overlaps it, a box that ends exactly on a half-integer leaves that cell
    at weight 0, and each fp32 weight is the exact overlap rounded (double subtraction, then fp32: 2^-24 + 2^-53 relative)."""
    def overlap(a, b, k):
        return max(Fraction(0), min(b, Fraction(2 * k + 1, 2)) - max(a, Fraction(2 * k - 1, 2)))

    cases = [(n, r) for (n, _) in SHAPES + [(4096, 1)] for r in ratios(B) + [0.53, 0.7071]]
    ends_on_half = 0
    for n, r in cases:
        r2 = np.float64(r) + np.float64(r)
        X2 = Z.positions(n, r2)
        X2 = X2[(X2 >= 0.0) & (X2 <= n - 1)]
        if X2.size > 300:
            X2 = np.concatenate([X2[:100], X2[X2.size // 2 - 50: X2.size // 2 + 50], X2[-100:]])
        idx, w, k0, a, b = ZF.box(X2, r2, n)
        # (the weights examined here are the library's: on an n x 1 keyframe its frame is the restatement built from them)
        line = keyframes(n, 1)[1] if n <= 67 else np.linspace(0.0, 1.0, 4 * n, dtype=np.float32).reshape(1, n, 4)
        assert ZF.same_bits(B.zoom_compose_filtered(line, line, r, B.ZOOM_FILTER_AREA)[0], ZF.compose(line, line, r, ZF.AREA)[0]).all(), (n, r)
        for i in range(X2.size):
            fa, fb, k = Fraction(float(a[i])), Fraction(float(b[i])), int(k0[i])
            exact = [overlap(fa, fb, k + j) for j in range(3)]
            assert sum(exact) == fb - fa, (n, r, i)
            assert abs((fb - fa) - Fraction(float(r2))) <= Fraction(math.ulp(max(abs(float(a[i])), abs(float(b[i])), 1.0))), (n, r, i)
            assert overlap(fa, fb, k - 1) == 0 and overlap(fa, fb, k + 3) == 0, (n, r, i)
            assert exact[0] > 0, "k0 is the cell that holds the box's lower end"
            assert k == math.floor(fa + Fraction(1, 2)), "k0 is floor(a + 0.5) of the exact a"
            for j in range(3):
                if exact[j] == 0:
                    assert w[i, j] == 0.0
                else:
                    assert abs(Fraction(float(w[i, j])) - exact[j]) <= exact[j] * Fraction(1, 2 ** 23), (n, r, i, j)
                if fb == Fraction(2 * (k + j) - 1, 2):
                    ends_on_half += 1
                    assert w[i, j] == 0.0, "the box ends on this cell's lower edge"
            assert (idx[i] == np.clip(k + np.arange(3), 0, n - 1)).all()
    assert ends_on_half >= 10                                     # (r = 0.5 and r = 1: every box ends on a half-integer)


@pytest.mark.parametrize("mode", ZC.MODES)
@pytest.mark.parametrize("W,H", [(1, 1), (7, 1), (2, 2), (67, 35)])
def test_counts_match_compose_of_colours(B, W, H, mode):
    for M in (1, 128, 300):
        wide, deep = planes(W, H, M, mode.startswith("smooth"))
        lut = B.colour_lut(M, KCOLOR)
        p = B.mandelbrot_params(W, H, max_iter=M, k_color=KCOLOR, flags=ZC.flag(B, mode))
        table = frame_map(mode, wide, deep, M)
        cw, cd = ZC.colour(mode, wide, M, lut, table), ZC.colour(mode, deep, M, lut, table)
        for r in ratios(B):
            for d, c in ((deep, cd), (None, None)):
                for f in (B.ZOOM_FILTER_AREA, B.ZOOM_FILTER_BILINEAR):
                    got, got8 = B.zoom_compose_counts_filtered(p, wide, d, table, r, f, want_rgba=True, want_rgba8=True)
                    lib, lib8 = B.zoom_compose_filtered(cw, c, r, f, want_rgba=True, want_rgba8=True)
                    assert np.array_equal(bits(got), bits(lib)) and np.array_equal(got8, lib8), (W, H, M, mode, r, f, "the library's own chain")
                    want, _ = ZF.frame_counts(mode, wide, d, M, lut, table, r, f)
                    assert np.array_equal(bits(got), bits(want)), (W, H, M, mode, r, f, "the restatement")
                    assert np.array_equal(got8, Z.rgba8(want))
                a, a8 = B.zoom_compose_counts(p, wide, d, table, r, want_rgba=True, want_rgba8=True)
                assert np.array_equal(bits(a), bits(got)) and np.array_equal(a8, got8), "filter 0 is the unfiltered call"
        assert np.array_equal(bits(B.zoom_compose_counts_filtered(p, wide, deep, table, 0.5, B.ZOOM_FILTER_AREA)[0])[..., :3], bits(cd)[..., :3])


def test_refusals(B):
    L = B.lib()
    wide, deep = keyframes(8, 8)
    out = np.empty((8, 8, 4), np.float32)
    out8 = np.empty((8, 8, 4), np.uint8)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def refused(W, H, w, d, r, f, o, o8, text):
        assert L.mc_mandelbrot_zoom_compose_filtered(W, H, p(w), p(d), r, f, p(o), p(o8)) == INVALID, text
        detail = L.mc_last_error_detail()
        assert text.encode() in detail and detail.startswith(b"mc_mandelbrot_zoom_compose_filtered: "), (text, detail)
        if f == 0:                                                 # the namesake's status and text after the name
            assert L.mc_mandelbrot_zoom_compose(W, H, p(w), p(d), r, p(o), p(o8)) == INVALID
            assert L.mc_last_error_detail().split(b": ", 1)[1] == detail.split(b": ", 1)[1]

    for f in (0, 1):
        refused(8, 8, None, deep, 0.75, f, out, None, "the wide keyframe is NULL")
        refused(0, 8, wide, deep, 0.75, f, out, None, "width and height must be above 0")
        refused(8, 0, wide, deep, 0.75, f, out, None, "width and height must be above 0")
        refused(8, 8, wide, deep, 0.75, f, None, None, "at least one output must be given")
        for r in (float(np.nextafter(0.5, 0.0)), float(np.nextafter(1.0, 2.0)), 0.0, -0.75, 2.0, math.inf, math.nan):
            refused(8, 8, wide, deep, r, f, out, out8, "is outside [0.5, 1]")
    for f in (2, 3, 0xffffffff):
        refused(8, 8, wide, deep, 0.75, f, out, out8, f"filter = {f} is neither")
    with pytest.raises(B.McError, match="filter = 7"):
        B.zoom_compose_filtered(wide, deep, 0.75, 7)
    with pytest.raises(B.McError, match="outside"):
        B.zoom_compose_filtered(wide, deep, 1.5, B.ZOOM_FILTER_AREA)

    # the count form: its namesake's refusals, then the filter's
    W, H, M = 8, 8, 128
    cw, cd = planes(W, H, M, False)
    qw, qd = planes(W, H, M, True)
    ident = np.arange(M + 1, dtype=np.uint32)
    knots = (256 * np.arange(M + 1)).astype(np.uint32)
    P = lambda **kw: B.mandelbrot_params(W, H, max_iter=kw.pop("max_iter", M), **kw)
    EQ, SM, SQ, DI = B.MANDEL_COLOUR_EQUALISED, B.MANDEL_COLOUR_SMOOTH, B.MANDEL_COLOUR_SMOOTH_EQUALISED, B.MANDEL_COLOUR_DISTANCE

    def crefused(q, w, d, m, r, f, o, o8, text):
        assert L.mc_mandelbrot_zoom_compose_counts_filtered(C.byref(q), p(w), p(d), p(m), r, f, p(o), p(o8)) == INVALID, text
        detail = L.mc_last_error_detail()
        assert text.encode() in detail and detail.startswith(b"mc_mandelbrot_zoom_compose_counts_filtered: "), (text, detail)
        if f == 0:
            assert L.mc_mandelbrot_zoom_compose_counts(C.byref(q), p(w), p(d), p(m), r, p(o), p(o8)) == INVALID
            assert L.mc_last_error_detail().split(b": ", 1)[1] == detail.split(b": ", 1)[1]

    assert L.mc_mandelbrot_zoom_compose_counts_filtered(None, p(cw), None, None, 1.0, 1, p(out), None) == INVALID
    for f in (0, 1):
        crefused(P(), None, cd, None, 0.75, f, out, None, "the wide keyframe is NULL")
        crefused(P(), cw, cd, None, 0.75, f, None, None, "at least one output must be given")
        crefused(P(), cw, cd, None, math.nan, f, out, out8, "is outside [0.5, 1]")
        crefused(P(), cw, cd, None, 1.25, f, out, out8, "is outside [0.5, 1]")
        crefused(B.mandelbrot_params(0, H, max_iter=M), cw, cd, None, 0.75, f, out, None, "width and height must be above 0")
        crefused(P(max_iter=0), cw, cd, None, 0.75, f, out, None, "max_iter")
        crefused(P(row_begin=1), cw, cd, None, 0.75, f, out, None, "whole image")
        crefused(P(flags=B.MANDEL_ITERS_U16), cw, cd, None, 0.75, f, out, None, "MC_MANDEL_ITERS_U16")
        crefused(P(flags=EQ | SM), cw, cd, ident, 0.75, f, out, None, "more than one colouring")
        crefused(P(flags=DI), qw, qd, None, 0.75, f, out, None, "MC_MANDEL_COLOUR_DISTANCE")
        crefused(P(supersample=2), cw, cd, None, 0.75, f, out, None, "MC_MANDEL_SUPERSAMPLE")
        crefused(P(adaptive=True), cw, cd, None, 0.75, f, out, None, "MC_MANDEL_SUPERSAMPLE_ADAPTIVE")
        crefused(P(flags=B.MANDEL_FMA), cw, cd, None, 0.75, f, out, None, "MC_MANDEL_FMA")
        crefused(P(), cw, cd, ident, 0.75, f, out, None, "take none")
        crefused(P(flags=EQ), cw, cd, None, 0.75, f, out, None, "need a map")
        bad = ident.copy(); bad[3] = M + 1
        crefused(P(flags=EQ), cw, cd, bad, 0.75, f, out, None, "a map entry exceeds max_iter")
        bad = knots.copy(); bad[5] = bad[6] + 1
        crefused(P(flags=SQ), qw, qd, bad, 0.75, f, out, None, "must not decrease")
        crefused(P(flags=SM, max_iter=1 << 24), qw, qd, None, 0.75, f, out, None, "2^24 - 1")
        over = qw.copy(); over[2, 3] = 256 * M + 1
        crefused(P(flags=SM), over, qd, None, 0.75, f, out, None, "wide[19] = 32769 is above 256 * max_iter")
    crefused(P(), cw, cd, None, 0.75, 2, out, None, "filter = 2 is neither")
    crefused(P(flags=SQ), qw, qd, knots, 0.75, 9, out, None, "filter = 9 is neither")
    assert L.mc_mandelbrot_zoom_compose_counts_filtered(C.byref(P(flags=SQ)), p(qw), p(qd), p(knots), 0.5, 1, p(out), None) == 0
    # the device forms and the sequence objects refuse a missing context or sequence before anything else
    assert L.mc_mandelbrot_zoom_compose_filtered_device_async(None, 8, 8, None, None, 0.75, 1, None, None, None) == INVALID
    assert L.mc_mandelbrot_zoom_compose_counts_filtered_device_async(None, C.byref(P()), None, None, None, 0.75, 1, None, None, None) == INVALID
    assert L.mc_mandelbrot_zoom_frame_filtered(None, 0.75, 1, p(out), None) == INVALID
    assert L.mc_mandelbrot_zoom_counts_frame_filtered(None, 1, 2, 1, p(out), None) == INVALID


def test_app_option_parsing(B, tmp_path):
    """--zoom-filter bilinear | area: a closed list, needs --zoom, a Mandelbrot option; refused by name before a device is touched."""
    bindir = os.path.join(os.path.dirname(os.path.dirname(B.LIB_PATH)), "bin")
    run = lambda app, args: subprocess.run([os.path.join(bindir, app)] + args, capture_output=True, text=True, cwd=tmp_path)
    zoom = ["--zoom", "1", "2", "--width", "16", "--height", "16"]
    for app, args, needle in (("mandelbrot", zoom + ["--zoom-filter", "box"], "not one of bilinear | area"),
                              ("mandelbrot", zoom + ["--zoom-filter"], "missing value"),
                              ("mandelbrot", ["--zoom-filter", "area"], "--zoom-filter: needs --zoom"),
                              ("mandelbrot", ["--zoom-filter", "bilinear"], "--zoom-filter: needs --zoom"),
                              ("pathtracer", ["--zoom-filter", "area"], "--zoom-filter: a Mandelbrot option")):
        r = run(app, args)
        assert r.returncode == 1 and needle in r.stdout, (app, args, r.stdout)
        assert "now running app" not in r.stdout
    n = C.c_int(0)
    if B.lib().mc_device_count(C.byref(n)) == 0 and n.value > 0:
        return                                                                 # (a GPU is present: the accepted forms run in the gpu tests)
    for words in (["area"], ["bilinear"], ["area", "--zoom-keyframes", "counts"], ["area", "--zoom-keyframes", "counts", "--colour", "smooth-equalised"]):
        r = run("mandelbrot", zoom + ["--quiet", "--zoom-filter"] + words)
        assert r.returncode == 1 and "could not find a device" in r.stdout and "not one of" not in r.stdout, r.stdout
    assert not list(tmp_path.glob("*.png"))


# ---- what the filter is for: the deep-sourced centre against a direct render of the frame's own view ------------------------------------
QW, QH, QM, QSTEPS = 96, 64, 200, 4
VIEWS = (("reference view", (-0.445, 0.0), (2.34, 1.56)),
         ("seahorse valley 2e-2", (-0.7436438870371587, 0.13182590420531198), (0.02, 0.0133333)),
         ("same centre 1e-4", (-0.7436438870371587, 0.13182590420531198), (1e-4, 6.6667e-5)))


def counts_f64(centre, scale, offsets):
    """The iteration counts of the QW x QH view in float64 with the oracle's loop and escape rule (|z|^2 > 2 after the update, at most QM
    updates), sampled at pixel + (ox, oy) for every offset: (len(offsets), QH, QW) int64.  c = centre + (g / n - 0.5) * scale."""
    off = np.asarray(offsets, np.float64)
    gx = (np.arange(QW, dtype=np.float64)[None, None, :] + off[:, 0][:, None, None]) / QW
    gy = (np.arange(QH, dtype=np.float64)[None, :, None] + off[:, 1][:, None, None]) / QH
    cx = np.broadcast_to(centre[0] + (gx - 0.5) * scale[0], (len(off), QH, QW)).ravel()
    cy = np.broadcast_to(centre[1] + (gy - 0.5) * scale[1], (len(off), QH, QW)).ravel()
    n = np.zeros(cx.size, np.int64)
    live = np.arange(cx.size)
    zx = np.zeros(cx.size)
    zy = np.zeros(cx.size)
    for _ in range(QM):
        nzx = (zx * zx - zy * zy) + cx
        zy = ((2.0 * zx) * zy) + cy
        zx = nzx
        keep = ~(zx * zx + zy * zy > 2.0)
        live, zx, zy, cx, cy = live[keep], zx[keep], zy[keep], cx[keep], cy[keep]
        n[live] += 1
        if not live.size:
            break
    return n.reshape(len(off), QH, QW)


def grid(s):
    """The s x s sample offsets centred on the pixel's sample point: (i + 0.5) / s - 0.5 on each axis."""
    o = (np.arange(s) + 0.5) / s - 0.5
    return [(x, y) for y in o for x in o]


@functools.lru_cache(maxsize=None)
def quality(B, view):
    """Per step 0 .. QSTEPS: (rmse bilinear, rmse area, frames bit-equal) on the deep-sourced pixels, in units of 255, for keyframes of
    1 sample per pixel and of 4 x 4 samples; truth is the frame's own view with 8 x 8 samples per pixel, averaged as colours."""
    _, centre, scale = VIEWS[view]
    lut = B.colour_lut(QM)
    colour = lambda n: lut[np.minimum(n, QM)].astype(np.float64).mean(axis=0).astype(np.float32)
    keys = {}
    for s in (1, 4):
        keys[s] = tuple(np.ascontiguousarray(colour(counts_f64(centre, (scale[0] * f, scale[1] * f), grid(s)))) for f in (1.0, 0.5))
    rows = []
    for step in range(QSTEPS + 1):
        r = B.zoom_ratio(step, QSTEPS)
        mask = Z.deep_mask(QW, QH, r)
        truth = colour(counts_f64(centre, (scale[0] * r, scale[1] * r), grid(8)))
        row = []
        for s in (1, 4):
            bil = B.zoom_compose_filtered(keys[s][0], keys[s][1], r, B.ZOOM_FILTER_BILINEAR)[0]
            area = B.zoom_compose_filtered(keys[s][0], keys[s][1], r, B.ZOOM_FILTER_AREA)[0]
            rmse = lambda f: float(np.sqrt(np.mean((255.0 * (f[mask][:, :3].astype(np.float64) - truth[mask][:, :3].astype(np.float64))) ** 2)))
            row.append((rmse(bil), rmse(area), bool(np.array_equal(bits(bil), bits(area)))))
        rows.append(tuple(row))
    return tuple(rows)


@pytest.mark.parametrize("view", range(len(VIEWS)))
def test_area_is_closer_to_the_supersampled_truth(B, view):
    """With keyframes of one sample per pixel the filtered centre is closer to the truth than the bilinear one at every in-between step
    (1, 2, 3 of 4), and at step 4 (r = 0.5, the keyframe itself) the two frames are the same bits.  The bare inequality is the assertion;
    every figure is printed (DESIGN.md §3.23 records them), the 4 x 4 supersampled keyframes' too, which are not asserted."""
    rows = quality(B, view)
    for step, ((b1, a1, same1), (b4, a4, same4)) in enumerate(rows):
        print(f"{VIEWS[view][0]}, step {step}/{QSTEPS}: 1 spp bilinear {b1:.2f} -> area {a1:.2f} (ratio {a1 / b1:.3f}); "
              f"4 x 4 keyframes bilinear {b4:.2f} -> area {a4:.2f} (ratio {a4 / b4:.3f})")
    for step in (1, 2, 3):
        b1, a1, _ = rows[step][0]
        assert a1 < b1, (VIEWS[view][0], step, b1, a1)
    assert rows[QSTEPS][0][2] and rows[QSTEPS][1][2], "r = 0.5: the two filters give the same bits"
    assert rows[QSTEPS][0][0] == rows[QSTEPS][0][1]
