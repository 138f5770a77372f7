"""MC_MANDEL_SUPERSAMPLE without a GPU: the macro and the exports, mc_mandelbrot_supersample_params against the restatement
(tests/mandel_supersample_ref.py) and its refusals, the two restatements of the colour rule against each other, the flat-pixel identity
over the library's own M = 50 000 table, the motivating fact (on K4's view most pixels hold more than one count), the argument checks of
mc_mandelbrot_resolve_device_async that need no device, the app's option handling."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mandel_f64_ref as F
import mandel_supersample_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
BAD_FACTORS = (3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(autouse=True)
def feature(B):
    """Every test here is about MC_MANDEL_SUPERSAMPLE: a library without it fails them all, the restatement-only ones included."""
    assert "MC_MANDEL_SUPERSAMPLE" in open(B.HEADER_PATH).read() and hasattr(B.lib(), "mc_mandelbrot_supersample_params")


def test_macro_value_and_position(B):
    text = open(B.HEADER_PATH).read()
    assert "#define MC_MANDEL_SUPERSAMPLE(s) (((uint32_t)(s) & 15u) << 8)" in text
    assert re.search(r"#define MC_ABI_VERSION 3\b", text)
    for s in range(16):
        assert B.MANDEL_SUPERSAMPLE(s) == s << 8 == S.flag(s)
    assert B.MANDEL_SUPERSAMPLE(8) & (B.MANDEL_COLOUR_EQUALISED | B.MANDEL_ITERS_U16 | 1 | 4 | 8) == 0
    # the keyword of mandelbrot_params: unused, the struct is byte for byte today's
    a, b = B.mandelbrot_params(33, 21, max_iter=77), B.mandelbrot_params(33, 21, max_iter=77, supersample=0)
    assert bytes(a) == bytes(b) and a.flags == 0
    assert B.mandelbrot_params(33, 21, supersample=4, flags=B.MANDEL_COLOUR_EQUALISED).flags == (4 << 8) | 16


def test_symbols_declared_and_exported(B):
    names = B.declared_symbols()
    for s in ("mc_mandelbrot_supersample_params", "mc_mandelbrot_resolve_device_async"):
        assert s in names and hasattr(B.lib(), s)


# ---- mc_mandelbrot_supersample_params -------------------------------------------------------------------------------------------
INT_FIELDS = ("width", "height", "max_iter", "precision", "row_begin", "row_end", "row_block", "row_stride", "flags", "reserved")
FLOAT_FIELDS = ("centre_x_hi", "centre_x_lo", "centre_y_hi", "centre_y_lo", "scale_x_hi", "scale_x_lo", "scale_y_hi", "scale_y_lo")


def as_dict(p):
    return {k: int(getattr(p, k)) for k in INT_FIELDS}


def check_grid(B, p):
    want = S.grid_params(as_dict(p))
    assert want is not None
    q = B.supersample_params(p)
    assert as_dict(q) == want
    for k in FLOAT_FIELDS:
        assert np.float32(getattr(q, k)).view(np.uint32) == np.float32(getattr(p, k)).view(np.uint32)
    assert list(q.k_color) == list(p.k_color)
    return q


@pytest.mark.parametrize("s", [0, 1, 2, 4, 8])
def test_supersample_params(B, s):
    kw = dict(max_iter=500, precision=B.PRECISION_F64, centre=F.DEEP_CENTRE, scale=(1e-8, 1e-8 * 2 / 3), k_color=(0.2, 0.3, 0.4, 0.5))
    f = max(s, 1)
    for extra in (0, B.MANDEL_COLOUR_EQUALISED, B.MANDEL_ITERS_U16 | B.MANDEL_COLOUR_EQUALISED | 1):
        flags = extra | B.MANDEL_SUPERSAMPLE(s)
        q = check_grid(B, B.mandelbrot_params(203, 131, flags=flags, **kw))                                       # a whole image
        assert (q.width, q.height, q.row_begin, q.row_end) == (203 * f, 131 * f, 0, 131 * f)
        assert q.flags == extra & ~B.MANDEL_COLOUR_EQUALISED
        q = check_grid(B, B.mandelbrot_params(203, 131, row_begin=17, row_end=90, flags=flags, **kw))             # a row tile
        assert (q.row_begin, q.row_end, q.row_block, q.row_stride) == (17 * f, 90 * f, 0, 0)
        p = B.mandelbrot_params(203, 131, row_begin=8, row_end=131, row_block=8, row_stride=24, flags=flags, **kw)  # an interleaved tile
        q = check_grid(B, p)
        assert (q.row_begin, q.row_end, q.row_block, q.row_stride) == (8 * f, 131 * f, 8 * f, 24 * f)
        # the tile of q: for each compact pixel row of p, its s sample rows in order
        assert B.tile_rows(q) == f * B.tile_rows(p)
        rows_p = [r for r in range(8, 131) if (r - 8) % 24 < 8]
        rows_q = [r for r in range(8 * f, 131 * f) if (r - 8 * f) % (24 * f) < 8 * f]
        assert rows_q == [f * r + i for r in rows_p for i in range(f)]
    p = B.mandelbrot_params(64, 48, supersample=s)
    assert B.lib().mc_mandelbrot_supersample_params(C.byref(p), C.byref(p)) == 0   # in place
    assert (p.width, p.height, p.row_end, p.flags) == (64 * f, 48 * f, 48 * f, 0)


def test_supersample_params_refusals(B):
    L = B.lib()
    q = B.MandelbrotParams()
    for s in BAD_FACTORS:
        p = B.mandelbrot_params(64, 48, supersample=s)
        assert S.grid_params(as_dict(p)) is None
        assert L.mc_mandelbrot_supersample_params(C.byref(p), C.byref(q)) == INVALID
        assert f"MC_MANDEL_SUPERSAMPLE({s})" in L.mc_last_error_detail().decode()
    big = 2 ** 32 - 1
    for field, value, s in (("width", big // 2 + 1, 2), ("height", big // 4 + 1, 4), ("row_end", big // 8 + 1, 8),
                            ("row_begin", 2 ** 31, 2), ("row_stride", 2 ** 30, 4), ("row_block", 2 ** 29, 8)):
        p = B.mandelbrot_params(64, 48, supersample=s)
        setattr(p, field, value)
        assert S.grid_params(as_dict(p)) is None
        assert L.mc_mandelbrot_supersample_params(C.byref(p), C.byref(q)) == INVALID, field
        setattr(p, field, value - 1)                                                  # the largest value that still fits
        assert L.mc_mandelbrot_supersample_params(C.byref(p), C.byref(q)) == 0, field
        assert getattr(q, field) == (value - 1) * s == S.grid_params(as_dict(p))[field]
    p = B.mandelbrot_params(64, 48, supersample=2)
    assert L.mc_mandelbrot_supersample_params(None, C.byref(q)) == INVALID
    assert L.mc_mandelbrot_supersample_params(C.byref(p), None) == INVALID


# ---- the colour rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", S.FACTORS)
def test_the_two_restatements_agree(B, s):
    M = 300
    lut = B.colour_lut(M)
    rng = np.random.default_rng(s)
    plane = rng.integers(0, M + 40, size=(5 * s, 7 * s), dtype=np.uint32)       # some counts above max_iter: entry max_iter
    plane[:s, :s] = 123                                                        # a flat pixel
    map_ = np.sort(rng.integers(0, M + 1, size=M + 1)).astype(np.uint32)
    for m in (None, map_):
        a, b = S.resolve(plane, s, M, lut, m), S.resolve_scalar(plane, s, M, lut, m)
        assert a.shape == (5, 7, 4) and np.array_equal(bits(a), bits(b))
        assert (bits(a[..., 3]) == 0x3f800000).all()                           # alpha: exactly 1.0f
        assert np.array_equal(bits(a[0, 0]), bits(lut[123] if m is None else lut[m[123]]))
        assert np.array_equal(S.rgba8(a)[..., 3], np.full((5, 7), 255, np.uint8))
    # a pixel of counts above max_iter: entry max_iter
    clamp = S.resolve(np.full((s, s), M + 5, np.uint32), s, M, lut)
    assert np.array_equal(bits(clamp[0, 0]), bits(lut[M]))


@pytest.mark.parametrize("s", S.FACTORS)
def test_flat_pixels_get_exactly_the_plain_colour(B, s):
    """Every entry of the library's own M = 50 000 table: s * s equal samples resolve to that entry, bit for bit."""
    M = 50000
    lut = B.colour_lut(M)
    plane = np.repeat(np.repeat(np.arange(M + 1, dtype=np.uint32).reshape(1, M + 1), s, axis=0), s, axis=1)   # (s, s * (M + 1))
    got = S.resolve(plane, s, M, lut)
    assert got.shape == (1, M + 1, 4)
    assert np.array_equal(bits(got[0]), bits(lut))
    assert np.array_equal(S.rgba8(got[0]), S.rgba8(lut))


def test_left_to_right_sums_would_not_keep_flat_pixels(B):
    """Why the order is part of the contract: 64 equal values added one after the other miss the value on a large share of the table."""
    M = 50000
    lut = B.colour_lut(M)
    acc = np.zeros_like(lut)
    for _ in range(64):
        acc = acc + lut
    off = (bits(acc * np.float32(1.0 / 64)) != bits(lut)).any(axis=-1).mean()
    print(f"left-to-right, s = 8: {100 * off:.1f} % of the table's entries change")
    assert off > 0


# ---- the motivating fact --------------------------------------------------------------------------------------------------------
def test_motivating_fact():
    """The central 96 x 64 pixels of K4's frame (scale 1e-8 by 2/3 of it at 7680 x 5120, M = 50 000) by tests/mandel_f64_ref.py: most
    pixels hold more than one count, and sample (s * y, s * x) is the plain image's count."""
    M, W, H = 50000, 96, 64
    sx = 1e-8 * 96 / 7680
    scale = (sx, sx * 2.0 / 3.0)
    plain = F.mandelbrot_iters_f64(W, H, M, F.DEEP_CENTRE, scale)
    for s in (2, 4):
        samples = F.mandelbrot_iters_f64(s * W, s * H, M, F.DEEP_CENTRE, scale)
        share, spread = S.mixed_share(samples, s)
        print(f"s = {s}: {100 * share:.1f} % of the pixels hold more than one count, mean (max - min) inside a pixel {spread:.0f}")
        assert share >= 0.80
        assert np.array_equal(samples[::s, ::s], plain)


# ---- the device call's argument checks ------------------------------------------------------------------------------------------
def test_resolve_refuses_bad_arguments_without_a_device(B):
    L = B.lib()
    res = L.mc_mandelbrot_resolve_device_async
    p = B.mandelbrot_params(8, 8, max_iter=10, supersample=2)
    buf = (C.c_uint32 * 1024)()
    one = C.cast(buf, C.c_void_p)
    m = (C.c_uint32 * 11)()
    fake = C.c_void_p(1)   # never dereferenced: the argument checks come first
    assert res(None, C.byref(p), one, 4, m, one, None) == INVALID       # no context
    assert res(fake, None, one, 4, m, one, None) == INVALID
    assert res(fake, C.byref(p), None, 4, m, one, None) == INVALID
    assert res(fake, C.byref(p), one, 4, m, None, None) == INVALID
    for width in (0, 1, 3, 8):
        assert res(fake, C.byref(p), one, width, m, one, None) == INVALID
    p.max_iter = 0
    assert res(fake, C.byref(p), one, 4, m, one, None) == INVALID


# ---- the app --------------------------------------------------------------------------------------------------------------------
def app(name, *args, cwd):
    return subprocess.run([os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", name)] + list(args), capture_output=True, text=True,
                          cwd=cwd, timeout=60)


def test_app_supersample_option(B, tmp_path):
    for bad in ("3", "0", "16", "two", "-2"):
        r = app("mandelbrot", "--supersample", bad, cwd=tmp_path)
        assert r.returncode == 1 and f"--supersample {bad}: not one of 1 | 2 | 4 | 8" in r.stdout
        assert "using device" not in r.stdout and not list(tmp_path.iterdir())
    r = app("mandelbrot", "--supersample", cwd=tmp_path)
    assert r.returncode == 1 and "missing value for --supersample" in r.stdout and not list(tmp_path.iterdir())
    for s in ("1", "2", "4", "8"):   # parsed and run up to the device: without a GPU init() fails with the device message
        r = app("mandelbrot", "--supersample", s, "--width", "64", "--height", "48", "--quiet", cwd=tmp_path)
        assert "not one of" not in r.stdout and "unknown option" not in r.stdout
        assert (r.returncode == 0 and (tmp_path / "mandelbrot.png").exists()) or (r.returncode == 1 and "could not find a device" in r.stdout)
    r = app("pathtracer", "--supersample", "2", cwd=tmp_path)
    assert r.returncode == 1 and "--supersample: a Mandelbrot option" in r.stdout and not (tmp_path / "pathtracer.png").exists()
