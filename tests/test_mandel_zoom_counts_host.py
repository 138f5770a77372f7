"""Zoom sequences from count keyframes without a GPU: mc_mandelbrot_zoom_blend_map against Python integers with the contract's stated
consequences, mc_mandelbrot_zoom_compose_counts (the kernel's own source, compiled for the host) against tests/mandel_zoom_counts_ref.py
bit for bit in all four colourings, the no-seam property and the defect of separately ranked keyframes it removes, every host refusal,
the app's option parsing."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import mandel_zoom_counts_ref as ZC
import mandel_zoom_ref as Z
from test_mandel_zoom_host import bits, ratios

INVALID = 1
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (64, 4), (67, 35)]   # (W, H)
MAX_ITERS = (1, 128, 300)
KCOLOR = (0.15, 0.65, 0.55, 0.0)


@functools.lru_cache(maxsize=None)
def planes(W, H, M, smooth):
    """Two random count keyframes (read-only): counts over the whole range with interior pixels; plain counts also run past M (the
    contract clamps them), smooth counts stop at 256 M (the host refuses more)."""
    rng = np.random.default_rng(100000 * W + 100 * H + M + (7 if smooth else 0))
    out = []
    for _ in range(2):
        top = 256 * M if smooth else M
        a = rng.integers(0, top + 1, size=(H, W), dtype=np.int64)
        pick = rng.random((H, W))
        a[pick < 0.15] = top
        if not smooth:
            a[pick > 0.95] = top + rng.integers(1, 1000)
            a[pick > 0.99] = 0xffffffff
        a = a.astype(np.uint32)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


def frame_map(mode, wide, deep, M, step=1, steps=3):
    """The map of a frame between two keyframes: the blend of their own maps (None without one)."""
    mw, md = ZC.own_map(mode, wide, M), ZC.own_map(mode, deep, M)
    return None if mw is None else ZC.blend(mw, md, step, steps)


def test_symbols(B):
    for name in ("mc_mandelbrot_zoom_blend_map", "mc_mandelbrot_zoom_compose_counts", "mc_mandelbrot_zoom_compose_counts_device_async",
                 "mc_mandelbrot_zoom_counts_create", "mc_mandelbrot_zoom_counts_push", "mc_mandelbrot_zoom_counts_frame",
                 "mc_mandelbrot_zoom_counts_maps", "mc_mandelbrot_zoom_counts_destroy"):
        assert name in B.declared_symbols() and hasattr(B.lib(), name), name
    assert B.lib().mc_abi_version() == 3


def test_blend_map(B):
    rng = np.random.default_rng(5)
    TOP = ZC.BLEND_MAX
    cases = []
    for n in (1, 2, 129, 1000):
        a = np.sort(rng.integers(0, TOP + 1, size=n, dtype=np.int64)).astype(np.uint32)
        b = np.sort(rng.integers(0, TOP + 1, size=n, dtype=np.int64)).astype(np.uint32)
        a[-1] = b[-1] = TOP                                  # the largest entry, and one equal in both
        cases.append((a, b))
    M = 300
    h = rng.integers(0, 50, size=M + 1)
    import mandel_equalise_ref as E
    import mandel_smooth_equalise_ref as SE
    cases.append((E.rank_map(h, M), E.rank_map(h[::-1].copy(), M)))
    cases.append((SE.knot_map(h, M), SE.knot_map(h[::-1].copy(), M)))
    for a, b in cases:
        for S in (1, 2, 3, 240, 2 ** 32 - 1):
            for s in sorted({0, 1, S // 2, S - 1, S}):
                got = B.zoom_blend_map(a, b, s, S)
                assert np.array_equal(got, ZC.blend(a, b, s, S)), (a.size, s, S)
                assert (got >= np.minimum(a, b)).all() and (got <= np.maximum(a, b)).all(), "between the two inputs"
                assert (np.diff(got.astype(np.int64)) >= 0).all(), "non-decreasing inputs give a non-decreasing output"
                assert got[-1] == a[-1] == b[-1], "an entry equal in both is kept"
                if s == 0:
                    assert np.array_equal(got, a)
                if s == S:
                    assert np.array_equal(got, b)
                if 0 < s < S:                               # below the top wherever either input is
                    below = (a < a[-1]) | (b < b[-1])
                    assert (got[below] < got[-1]).all()
    L = B.lib()
    a = np.array([0, 5], np.uint32)
    big = np.array([0, TOP + 1], np.uint32)
    out = np.zeros(2, np.uint32)
    p = lambda v: v.ctypes.data_as(C.c_void_p)
    assert L.mc_mandelbrot_zoom_blend_map(2, p(a), p(big), 1, 2, p(out)) == INVALID and b"256 * (2^24 - 1)" in L.mc_last_error_detail()
    assert L.mc_mandelbrot_zoom_blend_map(2, p(big), p(a), 1, 2, p(out)) == INVALID
    assert L.mc_mandelbrot_zoom_blend_map(2, p(a), p(a), 3, 2, p(out)) == INVALID and b"3 of 2" in L.mc_last_error_detail()
    assert L.mc_mandelbrot_zoom_blend_map(2, p(a), p(a), 0, 0, p(out)) == INVALID and b"mc_mandelbrot_zoom_blend_map" in L.mc_last_error_detail()
    assert L.mc_mandelbrot_zoom_blend_map(2, None, p(a), 0, 1, p(out)) == INVALID
    assert L.mc_mandelbrot_zoom_blend_map(2, p(a), p(a), 0, 1, None) == INVALID
    assert L.mc_mandelbrot_zoom_blend_map(0, None, None, 0, 1, None) == 0


@pytest.mark.parametrize("mode", ZC.MODES)
@pytest.mark.parametrize("W,H", SHAPES)
def test_compose_matches_restatement(B, W, H, mode):
    for M in MAX_ITERS:
        wide, deep = planes(W, H, M, mode.startswith("smooth"))
        lut = B.colour_lut(M, KCOLOR)
        p = B.mandelbrot_params(W, H, max_iter=M, k_color=KCOLOR, flags=ZC.flag(B, mode))
        table = frame_map(mode, wide, deep, M)
        for r in ratios(B):
            for d in (deep, None):
                want, _ = ZC.frame(mode, wide, d, M, lut, table, r)
                got, got8 = B.zoom_compose_counts(p, wide, d, table, r, want_rgba=True, want_rgba8=True)
                bad = (bits(got) != bits(want)).any(axis=-1)
                assert not bad.any(), (W, H, M, mode, r, d is not None, int(bad.sum()), got[bad][:2], want[bad][:2])
                assert np.array_equal(got8, Z.rgba8(want)), (W, H, M, mode, r, d is not None)
                only8 = B.zoom_compose_counts(p, wide, d, table, r, want_rgba=False, want_rgba8=True)[1]
                assert np.array_equal(only8, got8)
        # the ends: r = 1 without deep is the wide keyframe's own colours, r = 0.5 the deep one's, on every pixel
        assert np.array_equal(bits(B.zoom_compose_counts(p, wide, None, table, 1.0)[0])[..., :3], bits(ZC.colour(mode, wide, M, lut, table))[..., :3])
        assert np.array_equal(bits(B.zoom_compose_counts(p, wide, deep, table, 0.5)[0])[..., :3], bits(ZC.colour(mode, deep, M, lut, table))[..., :3])


@pytest.mark.parametrize("mode", ZC.MODES)
def test_no_seam(B, mode):
    """One piecewise-constant count field sampled at two scales an octave apart.  Wherever a frame's pixel reads four equal counts n, its
    colour is exactly the tap colour of n under the frame's ONE map, whichever keyframe it read, at every step; composing the two
    keyframes each ranked by its own map (the vec4 sequence's scheme) gives one count two colours in one frame."""
    W, H, M, S = 67, 35, 128, 4
    smooth = mode.startswith("smooth")
    wide, deep = ZC.field_plane(W, H, 1.0, M, smooth), ZC.field_plane(W, H, 0.5, M, smooth)
    lut = B.colour_lut(M, KCOLOR)
    p = B.mandelbrot_params(W, H, max_iter=M, k_color=KCOLOR, flags=ZC.flag(B, mode))
    mw, md = ZC.own_map(mode, wide, M), ZC.own_map(mode, deep, M)
    top = 256 * M if smooth else M
    key = lambda v: np.minimum(v.astype(np.int64) >> (8 if smooth else 0), M)      # a count's entry in the map
    if mw is not None:
        shared = np.intersect1d(key(wide[wide < top]), key(deep[deep < top]))
        assert shared.size >= 5 and (mw[shared[1:]] != md[shared[1:]]).all(), "the two keyframes' own maps differ on the shared counts"
    for step in range(S + 1):
        r = B.zoom_ratio(step, S)
        table = None if mw is None else B.zoom_blend_map(mw, md, step, S)
        got = B.zoom_compose_counts(p, wide, deep, table, r)[0]
        same, n = ZC.equal_taps(wide, deep, r)
        share = float(same.mean())
        print(f"{mode} step {step}/{S}: {100 * share:.1f} % of the pixels read four equal counts")
        assert share >= 0.5
        want = ZC.colour(mode, n, M, lut, table)
        assert np.array_equal(bits(got)[same][:, :3], bits(want)[same][:, :3]), (mode, step)
        if table is not None and 0 < step < S:
            occupied = np.union1d(key(wide[wide < top]), key(deep[deep < top]))
            assert (table[occupied] < table[M]).all(), "no escaped tap takes the interior's entry"
        if mw is not None and 0 < step < S:
            # the defect: each keyframe coloured by its own map, then composed.  A count read from both keyframes has two colours.
            apart = Z.compose(ZC.colour(mode, wide, M, lut, mw), ZC.colour(mode, deep, M, lut, md), r)[0]
            mask = Z.deep_mask(W, H, r)
            broken = 0
            for v in np.intersect1d(n[same & mask], n[same & ~mask]):
                if v >= top:
                    continue
                cols = {tuple(c) for c in bits(apart)[same & (n == v)][:, :3].tolist()}
                ours = {tuple(c) for c in bits(got)[same & (n == v)][:, :3].tolist()}
                assert len(ours) == 1
                broken += len(cols) > 1
            assert broken >= 1, (mode, step, "separately ranked keyframes were expected to break the property")


def test_refusals(B):
    L = B.lib()
    W, H, M = 8, 8, 128
    wide, deep = planes(W, H, M, False)
    qw, qd = planes(W, H, M, True)
    out = np.empty((H, W, 4), np.float32)
    out8 = np.empty((H, W, 4), np.uint8)
    ident = np.arange(M + 1, dtype=np.uint32)
    knots = (256 * np.arange(M + 1)).astype(np.uint32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    P = lambda **kw: B.mandelbrot_params(W, H, max_iter=kw.pop("max_iter", M), **kw)
    EQ, SM, SQ, DI = B.MANDEL_COLOUR_EQUALISED, B.MANDEL_COLOUR_SMOOTH, B.MANDEL_COLOUR_SMOOTH_EQUALISED, B.MANDEL_COLOUR_DISTANCE

    def refused(p, w, d, m, r, o, o8, text):
        assert L.mc_mandelbrot_zoom_compose_counts(C.byref(p), ptr(w), ptr(d), ptr(m), r, ptr(o), ptr(o8)) == INVALID, text
        detail = L.mc_last_error_detail()
        assert text.encode() in detail and b"mc_mandelbrot_zoom_compose_counts" in detail, (text, detail)

    assert L.mc_mandelbrot_zoom_compose_counts(None, ptr(wide), None, None, 1.0, ptr(out), None) == INVALID
    refused(P(), None, deep, None, 0.75, out, None, "the wide keyframe is NULL")
    refused(P(), wide, deep, None, 0.75, None, None, "at least one output must be given")
    for r in (float(np.nextafter(0.5, 0.0)), float(np.nextafter(1.0, 2.0)), 0.0, -0.75, 2.0, math.inf, math.nan):
        refused(P(), wide, deep, None, r, out, out8, "is outside [0.5, 1]")
    refused(B.mandelbrot_params(0, H, max_iter=M), wide, deep, None, 0.75, out, None, "width and height must be above 0")
    refused(P(max_iter=0), wide, deep, None, 0.75, out, None, "max_iter")
    refused(P(row_begin=1), wide, deep, None, 0.75, out, None, "whole image")
    refused(P(row_end=4), wide, deep, None, 0.75, out, None, "whole image")
    refused(P(row_block=8, row_stride=16), wide, deep, None, 0.75, out, None, "whole image")
    refused(P(flags=B.MANDEL_ITERS_U16), wide, deep, None, 0.75, out, None, "MC_MANDEL_ITERS_U16")
    for f in (EQ | SM, EQ | SQ, SM | SQ, EQ | SM | SQ):
        refused(P(flags=f), wide, deep, ident, 0.75, out, None, "more than one colouring")
    refused(P(flags=DI), qw, qd, None, 0.75, out, None, "MC_MANDEL_COLOUR_DISTANCE")
    refused(P(flags=SM | DI), qw, qd, None, 0.75, out, None, "MC_MANDEL_COLOUR_DISTANCE")
    refused(P(supersample=2), wide, deep, None, 0.75, out, None, "MC_MANDEL_SUPERSAMPLE")
    refused(P(supersample=4, adaptive=True), wide, deep, None, 0.75, out, None, "MC_MANDEL_SUPERSAMPLE")
    refused(P(adaptive=True), wide, deep, None, 0.75, out, None, "MC_MANDEL_SUPERSAMPLE_ADAPTIVE")
    refused(P(flags=B.MANDEL_FMA), wide, deep, None, 0.75, out, None, "MC_MANDEL_FMA")
    # a map where none belongs, none where one does, a map that is not one
    refused(P(), wide, deep, ident, 0.75, out, None, "take none")
    refused(P(flags=SM), qw, qd, knots, 0.75, out, None, "take none")
    refused(P(flags=EQ), wide, deep, None, 0.75, out, None, "need a map")
    refused(P(flags=SQ), qw, qd, None, 0.75, out, None, "need a map")
    bad = ident.copy(); bad[3] = M + 1
    refused(P(flags=EQ), wide, deep, bad, 0.75, out, None, "a map entry exceeds max_iter")
    bad = knots.copy(); bad[5] = bad[6] + 1
    refused(P(flags=SQ), qw, qd, bad, 0.75, out, None, "must not decrease")
    bad = knots.copy(); bad[M] -= 1
    refused(P(flags=SQ), qw, qd, bad, 0.75, out, None, "qmap[max_iter] must be 256 * max_iter")
    # the smooth colourings: max_iter within 24.8 fixed point, no q above 256 M on the host
    for f, m in ((SM, None), (SQ, knots)):
        refused(P(flags=f, max_iter=1 << 24), qw, qd, m, 0.75, out, None, "2^24 - 1")
        over = qw.copy(); over[2, 3] = 256 * M + 1
        refused(P(flags=f), over, qd, m, 0.75, out, None, "wide[19] = 32769 is above 256 * max_iter")
        refused(P(flags=f), qw, over, m, 0.75, out, None, "deep[19] = 32769 is above 256 * max_iter")
    # ... and what is accepted beside them
    assert L.mc_mandelbrot_zoom_compose_counts(C.byref(P(flags=EQ)), ptr(wide), None, ptr(ident), 1.0, None, ptr(out8)) == 0
    assert L.mc_mandelbrot_zoom_compose_counts(C.byref(P(flags=SQ)), ptr(qw), ptr(qd), ptr(knots), 0.5, ptr(out), None) == 0
    with pytest.raises(B.McError, match="outside"):
        B.zoom_compose_counts(P(), wide, deep, None, 1.5)
    with pytest.raises(ValueError):
        B.zoom_compose_counts(P(flags=EQ), wide, deep, ident[:-1], 0.75)
    with pytest.raises(ValueError):
        B.zoom_compose_counts(P(), wide[:-1], None, None, 0.75)
    # the device form and the sequence object refuse a missing context or sequence before anything else
    assert L.mc_mandelbrot_zoom_compose_counts_device_async(None, C.byref(P()), None, None, None, 0.75, None, None, None) == INVALID
    h = C.c_void_p()
    assert L.mc_mandelbrot_zoom_counts_create(None, W, H, C.byref(h)) == INVALID and not h
    assert L.mc_mandelbrot_zoom_counts_create(None, W, H, None) == INVALID
    assert L.mc_mandelbrot_zoom_counts_push(None, C.byref(P())) == INVALID
    assert L.mc_mandelbrot_zoom_counts_frame(None, 0, 1, ptr(out), None) == INVALID
    assert L.mc_mandelbrot_zoom_counts_maps(None, None, None) == INVALID
    assert L.mc_mandelbrot_zoom_counts_destroy(None) == 0


def test_app_option_parsing(B, tmp_path):
    """--zoom-keyframes colours | counts: a closed list; counts needs --zoom and refuses what a count keyframe cannot carry, by name, before
    a device is touched."""
    bindir = os.path.join(os.path.dirname(os.path.dirname(B.LIB_PATH)), "bin")
    run = lambda app, args: subprocess.run([os.path.join(bindir, app)] + args, capture_output=True, text=True, cwd=tmp_path)
    zoom = ["--zoom", "1", "2", "--width", "16", "--height", "16"]
    for app, args, needle in (("mandelbrot", zoom + ["--zoom-keyframes", "count"], "not one of colours | counts"),
                              ("mandelbrot", zoom + ["--zoom-keyframes"], "missing value"),
                              ("mandelbrot", ["--zoom-keyframes", "counts"], "--zoom-keyframes counts: needs --zoom"),
                              ("mandelbrot", zoom + ["--zoom-keyframes", "counts", "--colour", "distance"], "--zoom-keyframes counts: not with --colour distance"),
                              ("mandelbrot", zoom + ["--zoom-keyframes", "counts", "--supersample", "2"], "--zoom-keyframes counts: not with --supersample"),
                              ("mandelbrot", zoom + ["--zoom-keyframes", "counts", "--supersample", "4", "--adaptive"], "--zoom-keyframes counts: not with --adaptive"),
                              ("pathtracer", ["--zoom-keyframes", "counts"], "--zoom-keyframes: a Mandelbrot option")):
        r = run(app, args)
        assert r.returncode == 1 and needle in r.stdout, (app, args, r.stdout)
        assert "now running app" not in r.stdout
    n = C.c_int(0)
    if B.lib().mc_device_count(C.byref(n)) == 0 and n.value > 0:
        return                                                                 # (a GPU is present: the accepted forms run in the gpu tests)
    for words in (["colours"], ["counts"], ["counts", "--colour", "smooth-equalised"], ["colours", "--colour", "distance"]):
        r = run("mandelbrot", zoom + ["--quiet", "--zoom-keyframes"] + words)
        assert r.returncode == 1 and "could not find a device" in r.stdout and "not one of" not in r.stdout, r.stdout
    assert not list(tmp_path.glob("*.png"))
