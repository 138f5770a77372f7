"""Zoom sequences without a GPU: mc_mandelbrot_zoom_ratio against mpmath, mc_mandelbrot_zoom_compose (the kernel's own source, compiled for
the host) against tests/mandel_zoom_ref.py bit for bit, the contract's identities and closed form, every host refusal."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import mandel_zoom_ref as Z

INVALID = 1
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (8, 8), (67, 35)]   # (W, H)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ratios(B):
    return [1.0, 0.5, B.zoom_ratio(1, 3), B.zoom_ratio(2, 3), 0.75, float(np.nextafter(0.5, 1.0)), float(np.nextafter(1.0, 0.0))]


@functools.lru_cache(maxsize=None)
def keyframes(W, H):
    """Two random keyframes in [0, 1] with exact 0.0 and 1.0 entries, alpha 1; shared and read-only."""
    rng = np.random.default_rng(1000 * W + H)
    out = []
    for _ in range(2):
        a = rng.random((H, W, 4), dtype=np.float32)
        pick = rng.random((H, W, 4))
        a[pick < 0.1] = 0.0
        a[pick > 0.9] = 1.0
        a[..., 3] = 1.0
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


def test_symbols(B):
    for name in ("mc_mandelbrot_zoom_ratio", "mc_mandelbrot_zoom_compose", "mc_mandelbrot_zoom_compose_device_async",
                 "mc_mandelbrot_zoom_create", "mc_mandelbrot_zoom_push", "mc_mandelbrot_zoom_frame", "mc_mandelbrot_zoom_destroy"):
        assert name in B.declared_symbols() and hasattr(B.lib(), name), name
    assert B.lib().mc_abi_version() == 3


def test_ratio(B):
    import mpmath
    mpmath.mp.prec = 200
    for F in (1, 2, 3, 30, 240):
        r = [B.zoom_ratio(t, F) for t in range(F + 1)]
        assert r[0] == 1.0 and r[F] == 0.5, F
        assert all(a > b for a, b in zip(r, r[1:])), F
        for t, v in enumerate(r):
            exact = mpmath.power(2, -mpmath.mpf(t) / F)
            err = abs(mpmath.mpf(v) - exact)
            assert err <= mpmath.mpf(math.ulp(v)), (F, t, v)
    fn = B.lib().mc_mandelbrot_zoom_ratio
    out = C.c_double(0.0)
    assert fn(4, 3, C.byref(out)) == INVALID and b"4 of 3" in B.lib().mc_last_error_detail()
    assert fn(0, 0, C.byref(out)) == INVALID and b"steps per octave" in B.lib().mc_last_error_detail()
    assert fn(1, 3, None) == INVALID


@pytest.mark.parametrize("W,H", SHAPES)
def test_compose_matches_restatement(B, W, H):
    wide, deep = keyframes(W, H)
    for r in ratios(B):
        for d in (deep, None):
            want, mask = Z.compose(wide, d, r)
            got, got8 = B.zoom_compose(wide, d, r, want_rgba=True, want_rgba8=True)
            bad = (bits(got) != bits(want)).any(axis=-1)
            assert not bad.any(), (W, H, r, d is not None, int(bad.sum()), got[bad][:2], want[bad][:2])
            assert np.array_equal(got8, Z.rgba8(want)), (W, H, r, d is not None)
            only8 = B.zoom_compose(wide, d, r, want_rgba=False, want_rgba8=True)[1]
            assert np.array_equal(only8, got8)
            assert float(want.max()) <= 1.0                      # (the byte conversion cannot wrap)


@pytest.mark.parametrize("W,H", SHAPES)
def test_identities(B, W, H):
    wide, deep = keyframes(W, H)
    got = B.zoom_compose(wide, None, 1.0)[0]
    assert np.array_equal(bits(got), bits(wide)), "r = 1 without deep is wide's bits"
    got = B.zoom_compose(wide, deep, 0.5)[0]
    assert np.array_equal(bits(got), bits(deep)), "r = 0.5 is deep's bits on every pixel"
    assert Z.deep_mask(W, H, 0.5).all()
    # any finite input, signed zeros included (the distance shading writes -0.0f): still bit for bit
    rng = np.random.default_rng(7)
    odd = [(rng.random((H, W, 4), dtype=np.float32) - np.float32(0.5)) * np.float32(4.0) for _ in range(2)]
    for a in odd:
        a[rng.random((H, W, 4)) < 0.2] = np.float32(-0.0)
        a[..., 3] = 1.0
    assert np.array_equal(bits(B.zoom_compose(odd[0], None, 1.0)[0]), bits(odd[0]))
    assert np.array_equal(bits(B.zoom_compose(odd[0], odd[1], 0.5)[0]), bits(odd[1]))
    for r in (1.0, 0.5, 0.75):
        assert np.array_equal(bits(B.zoom_compose(odd[0], odd[1], r)[0]), bits(Z.compose(odd[0], odd[1], r)[0])), r


@pytest.mark.parametrize("W,H", SHAPES)
def test_deep_mask(B, W, H):
    """The pixels that read the deep keyframe: wide = 0 everywhere, deep = 1 everywhere, so the frame's red channel IS the mask."""
    wide = np.zeros((H, W, 4), np.float32)
    deep = np.ones((H, W, 4), np.float32)
    wide[..., 3] = 1.0
    for r in ratios(B):
        got = B.zoom_compose(wide, deep, r)[0]
        mask = Z.deep_mask(W, H, r)
        assert np.array_equal(got[..., 0] == 1.0, mask), (W, H, r)
        assert np.array_equal(got[..., 0] == 0.0, ~mask), (W, H, r)


def test_ramp_closed_form(B):
    """Keyframes that are linear ramps of the plane at scales 1 and 0.5 (values in [0.25, 0.75]): the frame at r is the ramp at scale r.
    Bound 2^-22 = 4 ulp at 0.5: the restatement measures 1 ulp; the margin is for the closed form's own summation order, computed in
    double here and rounded once, never for the library, which must equal the restatement exactly (test_compose_matches_restatement)."""
    W, H = 67, 35
    wide, deep = Z.ramp(W, H, 1.0), Z.ramp(W, H, 0.5)
    assert 0.25 <= float(wide[..., :2].min()) and float(wide[..., :2].max()) <= 0.75
    for r in ratios(B) + [0.53, 0.7071, 0.99]:
        got = B.zoom_compose(wide, deep, r)[0]
        want, _ = Z.compose(wide, deep, r)
        assert np.array_equal(bits(got), bits(want)), r
        err = float(np.abs(got[..., :2].astype(np.float64) - Z.ramp(W, H, r)[..., :2].astype(np.float64)).max())
        print(f"ramp r = {r!r}: max error {err / 2.0 ** -24:.2f} ulp(0.5)")
        assert err <= 2.0 ** -22, (r, err)
        assert np.array_equal(got[..., 2:], wide[..., 2:])


def test_refusals(B):
    L = B.lib()
    wide, deep = keyframes(8, 8)
    out = np.empty((8, 8, 4), np.float32)
    out8 = np.empty((8, 8, 4), np.uint8)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def refused(W, H, w, d, r, o, o8, text):
        assert L.mc_mandelbrot_zoom_compose(W, H, p(w), p(d), r, p(o), p(o8)) == INVALID, text
        assert text.encode() in L.mc_last_error_detail(), (text, L.mc_last_error_detail())

    refused(8, 8, None, deep, 0.75, out, None, "the wide keyframe is NULL")
    refused(0, 8, wide, deep, 0.75, out, None, "width and height must be above 0")
    refused(8, 0, wide, deep, 0.75, out, None, "width and height must be above 0")
    refused(8, 8, wide, deep, 0.75, None, None, "at least one output must be given")
    for r in (float(np.nextafter(0.5, 0.0)), float(np.nextafter(1.0, 2.0)), 0.0, -0.75, 2.0, math.inf, math.nan):
        refused(8, 8, wide, deep, r, out, out8, "is outside [0.5, 1]")
    with pytest.raises(B.McError, match="outside"):
        B.zoom_compose(wide, deep, 1.5)
    with pytest.raises(B.McError, match="steps per octave"):
        B.zoom_ratio(5, 4)
