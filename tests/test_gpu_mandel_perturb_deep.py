"""MC_PRECISION_PERTURB below 2^-960 on the MI355X: the deep kernel's iteration planes bit-exact against the numpy restatement of the
rescaled loop (tests/mandel_perturb_deep_ref.py) fed the library's own orbit table; every single-device entry point against the blocking
render; the multi-GPU refusal; the test switch that forces the deep kernel on today's views (its plain phase is StatePerturb bit for bit);
sampled rows at full size; the app end to end.  Orbits are bound to a context of the module's own."""
import ctypes as C
import fractions
import os
import subprocess

import numpy as np
import pytest

import mandel_perturb_deep_ref as D
import mandel_perturb_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "mandelbrot")


@pytest.fixture(scope="module")
def dctx(B):
    c = B.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def pp(B, W, H, M, **kw):
    return B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_PERTURB, centre=(0.0, 0.0), scale=(0.0, 0.0), **kw)


def deep_orbit(B, point, depth, M, mantissa=None):
    c, m, E = D.view(point, depth)
    o = B.Orbit(c[0], c[1], *(mantissa or m), M, E)
    assert o.deep
    return o


VIEWS = [
    ("just below 2^-960", D.M33, "5e-290", 2000, 96, 64, None),
    ("M33 1e-300", D.M33, "1e-300", 2000, 96, 64, None),
    ("M33 1e-1000", D.M33, "1e-1000", 6000, 96, 64, None),
    ("M41 1e-1000", D.M41, "1e-1000", 10000, 96, 64, None),
    ("near the floor 1e-2400", D.M33, "1e-2400", 12000, 64, 48, None),
    ("non-square, negative mantissa", D.M41, "1e-900", 8000, 72, 40, (-0.7, 0.45)),
]


@pytest.mark.parametrize("name,point,depth,M,W,H,mant", VIEWS, ids=[v[0] for v in VIEWS])
def test_plane_is_the_restatement(dctx, B, O, name, point, depth, M, W, H, mant):
    with deep_orbit(B, point, depth, M, mant) as o:
        dctx.bind_mandelbrot_orbit(o)
        rgba, it = dctx.mandelbrot(pp(B, W, H, M))
        ref = D.orbit_plane(o, W, H, M)
        import torch
        t16 = torch.zeros((H, W), dtype=torch.int16, device="cuda")
        dctx.mandelbrot_device(pp(B, W, H, M, flags=B.MANDEL_ITERS_U16), 0, t16.data_ptr())
        torch.cuda.synchronize()
    assert np.array_equal(it, ref), (name, int((it != ref).sum()))
    assert np.array_equal(t16.cpu().numpy().view(np.uint16).astype(np.uint32), ref)
    assert len(np.unique(ref)) >= 10, (name, len(np.unique(ref)))
    lut, _ = O.mandel_lut(M)
    assert np.array_equal(bits(rgba), bits(lut[ref]))


def tile_row_list(H, row_begin, row_end, row_block, row_stride):
    if not row_stride:
        return list(range(row_begin, row_end))
    return [r for r in range(row_begin, row_end) if (r - row_begin) % row_stride < row_block]


def test_every_entry_point(dctx, B):
    import torch
    L = B.lib()
    L.mc_mandelbrot_render_rgba8.argtypes = [C.c_void_p, C.POINTER(B.MandelbrotParams), C.c_void_p]
    L.mc_context_warmup_mandelbrot.argtypes = [C.c_void_p, C.POINTER(B.MandelbrotParams), C.c_int]
    W, H, M = 203, 131, 6000
    c, m, E = D.view(D.M33, "1e-1000")
    with B.Orbit(c[0], c[1], *m, M, E) as o:
        dctx.bind_mandelbrot_orbit(o)
        p = pp(B, W, H, M)
        rgba, whole = dctx.mandelbrot(p)
        assert len(np.unique(whole)) >= 10
        for rb, re_ in ((0, 1), (5, 37), (37, H), (H - 1, H)):
            _, t = dctx.mandelbrot(pp(B, W, H, M, row_begin=rb, row_end=re_))
            assert np.array_equal(t, whole[rb:re_]), (rb, re_)
        for rb, blk, stride in ((0, 8, 16), (3, 5, 20)):
            _, t = dctx.mandelbrot(pp(B, W, H, M, row_begin=rb, row_end=H, row_block=blk, row_stride=stride))
            assert np.array_equal(t, whole[tile_row_list(H, rb, H, blk, stride)]), (rb, blk, stride)
        d_rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        d_it = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        s = torch.cuda.Stream()
        dctx.mandelbrot_device(p, d_rgba.data_ptr(), d_it.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        assert np.array_equal(d_it.cpu().numpy().astype(np.uint32), whole) and np.array_equal(bits(d_rgba.cpu().numpy()), bits(rgba))
        whole8 = dctx.convert_rgba8(rgba, 255.0)
        out = np.zeros((H, W, 4), np.uint8)
        assert L.mc_mandelbrot_render_rgba8(dctx._h, C.byref(p), out.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(out, whole8)
        for band_rows in (1000, 37):
            for rgba8 in (False, True):
                img, _ = dctx.mandelbrot_banded(pp(B, W, H, M), band_rows, rgba8=rgba8)
                want = whole8 if rgba8 else rgba
                assert np.array_equal(img.view(np.uint8), want.view(np.uint8)), (band_rows, rgba8)
        with B.Multi(1) as mm:                                   # multi-GPU: unsupported, as for PERTURB
            with pytest.raises(B.McError) as e:
                mm.mandelbrot(p)
            assert e.value.status == 5
        with B.Context(0) as c2:                                 # warm-up on a fresh context, then the render
            c2.bind_mandelbrot_orbit(o)
            for rgba8 in (0, 1, 2):
                assert L.mc_context_warmup_mandelbrot(c2._h, C.byref(p), rgba8) == 0
                rg, it2 = c2.mandelbrot(p)
                assert np.array_equal(it2, whole) and np.array_equal(bits(rg), bits(rgba))


K4 = R.DEEP_CENTRE
SHALLOW = [   # the views of tests/test_gpu_mandel_perturb.py
    (96, 64, 256, ("-0.445", "0"), (2.34, 2.34)),
    (64, 48, 20000, K4, (1e-8, 1e-8 * 2 / 3)),
    (64, 48, 20000, K4, (1e-20, 1e-20)),
    (64, 48, 5000, ("-0.1", "0.2"), (1e-14, 1e-14)),
    (40, 24, 3000, ("-0.75", "0.1"), (1e-100, 1e-100)),
    (24, 16, 2000, ("-1.25", "0.001"), (2.0 ** -950, 2.0 ** -950)),
    (77, 45, 1003, ("-0.75", "0.1"), (0.05, 0.03)),
    (13, 5, 7, ("-0.445", "0"), (2.34, 2.34)),
    (64, 48, 4000, "boundary", (1e-20, 1e-20)),   # an escaping reference orbit (L < M), computed in the test
]


@pytest.mark.parametrize("W,H,M,centre,scale", SHALLOW)
def test_forced_deep_kernel_is_perturb_on_shallow_views(dctx, B, W, H, M, centre, scale):
    if centre == "boundary":
        centre = R.mp_boundary_point(("-0.5", "0"), ("-0.5", "1"), 4000, 70, 134)
    with B.Orbit(centre[0], centre[1], scale[0], scale[1], M) as o:
        dctx.bind_mandelbrot_orbit(o)
        rgba, it = dctx.mandelbrot(pp(B, W, H, M))
        rgba_d, it_d = dctx.mandelbrot(pp(B, W, H, M, flags=B.MANDEL_PERTURB_FORCE_DEEP))
    assert np.array_equal(it_d, it), int((it_d != it).sum())
    assert np.array_equal(bits(rgba_d), bits(rgba))


def test_forced_deep_kernel_k4_full_size_rows(dctx, B):
    W, H, M = 7680, 5120, 20000
    with B.Orbit(*K4, 1e-20, 1e-20 * 2 / 3, M) as o:
        dctx.bind_mandelbrot_orbit(o)
        _, it = dctx.mandelbrot(pp(B, W, H, M), want_rgba=False)
        _, itd = dctx.mandelbrot(pp(B, W, H, M, flags=B.MANDEL_PERTURB_FORCE_DEEP), want_rgba=False)
        rows, cols = [0, 1777, 2560, H - 1], np.arange(0, W, 7)
        ref = R.plane(o.table(), o.length, W, H, M, o.scale, rows=rows, cols=cols)
    assert np.array_equal(itd, it), int((itd != it).sum())
    assert np.array_equal(itd[rows][:, cols], ref)


def test_full_size_sampled_rows(dctx, B):
    W, H, M = 7680, 5120, 6000
    with deep_orbit(B, D.M33, "1e-1000", M) as o:
        dctx.bind_mandelbrot_orbit(o)
        _, it = dctx.mandelbrot(pp(B, W, H, M), want_rgba=False)
        rows, cols = [0, 1777, 2560, H - 1], np.arange(0, W, 7)
        ref = D.orbit_plane(o, W, H, M, rows=rows, cols=cols)
    assert np.array_equal(it[rows][:, cols], ref), int((it[rows][:, cols] != ref).sum())
    assert len(np.unique(ref)) >= 10


def long_double_mantissa(text):
    """The app's (mantissa, exp2) of a scale text: strtold (x86-64: 64-bit significand, to nearest), frexpl, then a cast to double."""
    v = fractions.Fraction(text)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if v >= fractions.Fraction(2) ** e:
        e += 1
    q = v / fractions.Fraction(2) ** e * 2 ** 64               # [2^63, 2^64)
    f = q.numerator // q.denominator
    rem = q - f
    if rem > fractions.Fraction(1, 2) or (rem == fractions.Fraction(1, 2) and f % 2):
        f += 1
    return float(fractions.Fraction(f, 2 ** 64)), e


def test_app_end_to_end(B, O, tmp_path):
    W, H, M = 128, 96, 6000
    c, _, _ = D.view(D.M33, "1e-1000")
    m, E = B.scale_from_text("1e-1000")
    assert long_double_mantissa("1e-1000") == (m, E)      # the app's conversion gives the same pair for this text
    out = tmp_path / "deep.png"
    r = subprocess.run([APP, "--precision", "perturb", "--width", str(W), "--height", str(H), "--max-iter", str(M), "--centre", c[0],
                        c[1], "--scale", "1e-1000", "1e-1000", "--out", str(out), "--quiet"], capture_output=True, text=True, cwd=tmp_path,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with B.Orbit(c[0], c[1], m, m, M, E) as o:
        ref = D.orbit_plane(o, W, H, M)
    assert len(np.unique(ref)) >= 10
    lut, _ = O.mandel_lut(M)
    with B.Context(0) as ctx:
        want = ctx.convert_rgba8(np.ascontiguousarray(lut[ref]), 255.0)
    from PIL import Image
    img = np.asarray(Image.open(out).convert("RGBA"))
    assert np.array_equal(img, want)


@pytest.mark.parametrize("scale", [("1e-2500", "1e-2500"), ("1e-1000x", "1e-1000"), ("1e-1000", "")])
def test_app_refuses_bad_scales(tmp_path, scale):
    r = subprocess.run([APP, "--precision", "perturb", "--centre", "-0.75", "0.1", "--scale", *scale, "--width", "16", "--height", "16",
                        "--max-iter", "100", "--out", str(tmp_path / "x.png"), "--quiet"], capture_output=True, text=True, cwd=tmp_path,
                       timeout=60)
    assert r.returncode != 0 and not list(tmp_path.iterdir()), r.stdout
