"""MC_MANDEL_SUPERSAMPLE_SMOOTH without a GPU: mc_mandelbrot_resolve_smooth against the restatement bit for bit
(tests/mandel_smooth_supersample_ref.py), the contract's first two stated consequences, mc_mandelbrot_supersample_params with and without
the bit, every refusal of the host call, the app's option errors, the motivating fact on an exact restatement of the reference view, the
exports."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mandel_smooth_ref as S
import mandel_smooth_supersample_ref as X
import mandel_supersample_ref as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
SHAPES = [(1, 1), (3, 2), (5, 3), (33, 7), (130, 5)]                      # width x rows
MAX_ITERS = [1, 7, 300, 70000]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want, what=""):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g, w), (what, int((g != w).any(axis=-1).sum()), "pixels differ")


def test_enum_value_and_symbols(B):
    assert B.MANDEL_SUPERSAMPLE_SMOOTH == X.SUPERSAMPLE_SMOOTH == 1 << 13
    text = open(B.HEADER_PATH).read()
    assert "MC_MANDEL_SUPERSAMPLE_SMOOTH = 1u << 13" in text and "#define MC_ABI_VERSION 3" in text
    names = B.declared_symbols()
    for s in ("mc_mandelbrot_resolve_smooth_device_async", "mc_mandelbrot_resolve_smooth"):
        assert s in names and hasattr(B.lib(), s)
    p = B.mandelbrot_params(8, 8, flags=B.MANDEL_COLOUR_SMOOTH, supersample=2, smooth_samples=True)
    assert p.flags == B.MANDEL_COLOUR_SMOOTH | B.MANDEL_SUPERSAMPLE(2) | B.MANDEL_SUPERSAMPLE_SMOOTH
    assert not B.mandelbrot_params(8, 8, supersample=2).flags & B.MANDEL_SUPERSAMPLE_SMOOTH


@pytest.mark.parametrize("M", MAX_ITERS)
@pytest.mark.parametrize("s", X.FACTORS)
def test_host_call_is_the_restatement(B, s, M):
    rng = np.random.default_rng(1000 * s + M)
    lut = B.colour_lut(M)
    maps = [("none", None)] + X.knot_maps(rng, M)
    for W, rows in SHAPES:
        q = X.seeded_plane(rng, rows, W, s, M)
        for name, qmap in maps:
            got = B.resolve_smooth(M, s, q, qmap)
            assert got.dtype == np.float32 and got.shape == (rows, W, 4)
            same(got, X.resolve(q, s, M, lut, qmap), (W, rows, name))
            assert (got[..., 3] == np.float32(1.0)).all()


@pytest.mark.parametrize("s", X.FACTORS)
def test_flat_pixels_get_the_smooth_colour(B, s):
    """Consequence 1: every q of M = 300 as a pixel whose s * s samples share it: exactly mc_mandelbrot_smooth_colour of q."""
    M = 300
    q = np.arange(256 * M + 1, dtype=np.uint32)
    plane = np.repeat(np.repeat(q[None, :], s, axis=0), s, axis=1)
    same(B.resolve_smooth(M, s, plane)[0], B.smooth_colour(M, q), "unranked")
    rng = np.random.default_rng(7 + s)
    for name, qmap in X.knot_maps(rng, M):
        same(B.resolve_smooth(M, s, plane, qmap)[0], B.smooth_colour(M, B.smooth_remap(M, qmap, q)), name)


@pytest.mark.parametrize("s", X.FACTORS)
def test_zero_fractions_give_the_integer_resolve(B, s):
    """Consequence 2: q = 256 n gives what the integer resolve gives for the counts n (the restatement of MC_MANDEL_SUPERSAMPLE)."""
    for M in (1, 7, 300):
        rng = np.random.default_rng(50 * s + M)
        lut = B.colour_lut(M)
        for W, rows in SHAPES:
            n = rng.integers(0, M + 1, size=(rows * s, W * s))
            same(B.resolve_smooth(M, s, (256 * n).astype(np.uint32)), SS.resolve(n, s, M, lut), (M, W, rows))


def test_supersample_params(B):
    SM, SE, BIT = B.MANDEL_COLOUR_SMOOTH, B.MANDEL_COLOUR_SMOOTH_EQUALISED, B.MANDEL_SUPERSAMPLE_SMOOTH
    fields = ("width", "height", "row_begin", "row_end", "row_block", "row_stride")
    for s in (0, 1, 2, 4, 8):
        for flags in (0, SM, SE, B.MANDEL_COLOUR_DISTANCE, B.MANDEL_COLOUR_EQUALISED, SM | BIT, SE | BIT, BIT):
            for adaptive in (False, True):
                p = B.mandelbrot_params(37, 24, max_iter=99, flags=flags, supersample=s, adaptive=adaptive, row_begin=4, row_end=20,
                                        row_block=2, row_stride=6)
                g = B.supersample_params(p)
                want = B.MandelbrotParams.from_buffer_copy(bytes(p))
                for f in fields:
                    setattr(want, f, getattr(p, f) * max(s, 1))
                want.flags = X.grid_flags(p.flags)
                assert bytes(g) == bytes(want), (s, flags, adaptive)
                if flags & BIT:                                           # the grid is the smooth render's argument
                    assert not g.flags & BIT and bool(g.flags & SM) == bool(flags & (SM | SE)) and not g.flags & SE
                else:                                                     # as before: the smooth bits are copied
                    assert g.flags & (SM | SE) == flags & (SM | SE)
                    assert g.flags == p.flags & ~(15 << 8) & ~B.MANDEL_COLOUR_EQUALISED & ~B.MANDEL_SUPERSAMPLE_ADAPTIVE


def test_host_refusals(B):
    L = B.lib()
    M, s, W, rows = 3, 2, 2, 1
    k = (C.c_float * 4)(0.1, 0.7, 0.6, 0.0)
    q = (C.c_uint32 * 8)(0, 255, 256, 767, 768, 1, 2, 3)
    qmap = (C.c_uint32 * 4)(0, 100, 500, 768)
    out = (C.c_float * 8)()
    call = L.mc_mandelbrot_resolve_smooth
    assert call(M, k, s, W, rows, q, qmap, out) == 0 and call(M, k, s, W, rows, q, None, out) == 0
    assert call(0, k, s, W, rows, q, None, out) == INVALID
    assert call(S.MAX_ITER_LIMIT + 1, k, s, W, rows, q, None, out) == INVALID
    for bad in (0, 1, 3, 5, 6, 7, 16):
        assert call(M, k, bad, W, rows, q, None, out) == INVALID
    assert call(M, None, s, W, rows, q, None, out) == INVALID
    assert call(M, k, s, 0, rows, q, None, out) == INVALID
    assert call(M, k, s, W, 0, q, None, out) == INVALID
    assert call(M, k, s, W, rows, None, None, out) == INVALID
    assert call(M, k, s, W, rows, q, None, None) == INVALID
    high = (C.c_uint32 * 8)(0, 255, 256, 767, 769, 1, 2, 3)               # a q above 256 M, as mc_mandelbrot_smooth_colour refuses it
    assert call(M, k, s, W, rows, high, None, out) == INVALID and b"above 256 * max_iter" in L.mc_last_error_detail()
    for knots in ((0, 100, 500, 767), (0, 600, 500, 768), (0, 100, 900, 768)):   # as mc_mandelbrot_smooth_remap refuses them
        assert call(M, k, s, W, rows, q, (C.c_uint32 * 4)(*knots), out) == INVALID
        assert b"mc_mandelbrot_resolve_smooth" in L.mc_last_error_detail()
    with pytest.raises(ValueError):
        B.resolve_smooth(M, 2, np.zeros((3, 4), np.uint32))
    with pytest.raises(ValueError):
        B.resolve_smooth(M, 2, np.zeros((2, 4), np.uint32), np.zeros(3, np.uint32))


def test_device_call_refuses_bad_arguments_without_a_device(B):
    L = B.lib()
    p = B.mandelbrot_params(8, 8, max_iter=10, flags=B.MANDEL_COLOUR_SMOOTH, supersample=2, smooth_samples=True)
    buf = (C.c_uint32 * 64)()
    assert L.mc_mandelbrot_resolve_smooth_device_async(None, C.byref(p), buf, None, buf, None) == INVALID
    assert L.mc_mandelbrot_render(None, C.byref(p), buf, None) == INVALID
    assert L.mc_mandelbrot_render_rgba8(None, C.byref(p), buf) == INVALID


def app(name, *args, cwd):
    return subprocess.run([os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", name)] + list(args), capture_output=True, text=True,
                          cwd=cwd, timeout=60)


def test_app_option_errors(tmp_path):
    size = ["--width", "64", "--height", "48"]
    for args in (["--supersample-smooth"], ["--supersample-smooth", "--colour", "smooth"], ["--supersample-smooth", "--supersample", "1", "--colour", "smooth"],
                 ["--supersample-smooth", "--supersample", "2"], ["--supersample-smooth", "--supersample", "2", "--colour", "equalised"],
                 ["--supersample-smooth", "--supersample", "4", "--colour", "distance"],
                 ["--supersample-smooth", "--supersample", "2", "--colour", "smooth", "--adaptive"]):
        r = app("mandelbrot", *args, *size, cwd=tmp_path)
        assert r.returncode == 1 and "--supersample-smooth" in r.stdout, (args, r.stdout)
        assert "could not find a device" not in r.stdout
    r = app("mandelbrot", "--colour", "smooth", "--supersample", "2", *size, cwd=tmp_path)         # still refused without the switch
    assert r.returncode == 1 and "--colour smooth" in r.stdout and "does not combine with --supersample" in r.stdout
    assert "--supersample-smooth" in r.stdout
    r = app("mandelbrot", "--colour", "smooth-equalised", "--supersample", "2", *size, cwd=tmp_path)
    assert r.returncode == 1 and "--colour smooth-equalised" in r.stdout and "--supersample-smooth" in r.stdout
    r = app("mandelbrot", "--colour", "smooth", "--supersample", "2", "--supersample-smooth", "--zoom", "1", "1", "--zoom-keyframes", "counts",
            *size, cwd=tmp_path)
    assert r.returncode == 1 and "--zoom-keyframes counts" in r.stdout
    r = app("pathtracer", "--supersample-smooth", cwd=tmp_path)
    assert r.returncode == 1 and "--supersample-smooth: a Mandelbrot option" in r.stdout
    for colour in ("smooth", "smooth-equalised"):                          # accepted: renders, or finds no device
        r = app("mandelbrot", "--colour", colour, "--supersample", "2", "--supersample-smooth", "--quiet", *size, cwd=tmp_path)
        assert "--supersample-smooth:" not in r.stdout and "unknown option" not in r.stdout and "does not combine" not in r.stdout
        assert (r.returncode == 0 and (tmp_path / "mandelbrot.png").exists()) or (r.returncode == 1 and "could not find a device" in r.stdout)


def rmse(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float(np.sqrt((d * d).mean()))


def test_motivating_fact(B, O):
    """On the F32 reference view at 64 x 64, M = 128, the s = 4 smooth-resolved image is closer (RMSE of the vec4) to the s = 8 one than
    the 1-sample smooth image is.  The direction only; DESIGN.md section 3.25 quotes the two values printed here."""
    W = H = 64
    M = 128
    lut = B.colour_lut(M)

    def plane(s):
        n, zx, zy, cx, cy = S.f32_capture(s * W, s * H, M)
        return S.smooth_count(O, n, M, zx, zy, cx, cy)

    one = S.colour(plane(1), M, lut)
    four = B.resolve_smooth(M, 4, plane(4))
    q8 = plane(8)
    eight = B.resolve_smooth(M, 8, q8)
    same(eight, X.resolve(q8, 8, M, lut), "s = 8 against the restatement")
    near, far = rmse(four, eight), rmse(one, eight)
    print(f"RMSE to the s = 8 image: s = 4 {near:.6f}, 1 sample {far:.6f}")
    assert near < far
