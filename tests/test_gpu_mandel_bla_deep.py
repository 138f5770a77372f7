"""MC_PRECISION_PERTURB_BLA_DEEP on the MI355X: iteration planes and trip-count planes bit-exact against the numpy restatement of the
contract in include/mc_compute.h (tests/mandel_bla_deep_ref.py), fed the library's own orbit and floatexp tables, on deep and shallow
views; every entry point against the blocking render; the binding rules; precision 4 and PERTURB unchanged on an orbit that carries
both tables; the multi-GPU refusal; sampled rows at full size; the app end to end.  Orbits are bound to a context of the module's own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mandel_bla_deep_ref as BD
import mandel_bla_ref as BR
import mandel_perturb_deep_ref as D
import mandel_perturb_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "mandelbrot")
K4 = R.DEEP_CENTRE


@pytest.fixture(scope="module")
def xctx(B):
    c = B.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def pp(B, W, H, M, **kw):
    return B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_PERTURB_BLA_DEEP, centre=(0.0, 0.0), scale=(0.0, 0.0), **kw)


def deep_orbit(B, point, depth, M, mantissa=None):
    c, m, E = D.view(point, depth)
    o = B.Orbit(c[0], c[1], *(mantissa or m), M, E)
    assert o.deep
    o.bla_deep()
    return o


def shallow_orbit(B, centre, scale, M):
    o = B.Orbit(centre[0], centre[1], scale[0], scale[1], M)
    o.bla_deep()
    return o


DEEP = [   # the views of tests/test_gpu_mandel_perturb_deep.py
    ("just below 2^-960", D.M33, "5e-290", 2000, 96, 64, None),
    ("M33 1e-300", D.M33, "1e-300", 2000, 96, 64, None),
    ("M33 1e-1000", D.M33, "1e-1000", 6000, 96, 64, None),
    ("M41 1e-1000", D.M41, "1e-1000", 10000, 96, 64, None),
    ("near the floor 1e-2400", D.M33, "1e-2400", 12000, 64, 48, None),
    ("non-square, negative mantissa", D.M41, "1e-900", 8000, 72, 40, (-0.7, 0.45)),
]
SHALLOW = [
    ("K4 1e-20", 64, 48, 20000, K4, (1e-20, 1e-20)),
    ("centre -1 (zeros in the orbit)", 40, 24, 1000, ("-1", "0"), (1e-10, 1e-10)),
]


@pytest.mark.parametrize("name,point,depth,M,W,H,mant", DEEP, ids=[v[0] for v in DEEP])
def test_deep_planes_are_the_restatement(xctx, B, O, name, point, depth, M, W, H, mant):
    with deep_orbit(B, point, depth, M, mant) as o:
        xctx.bind_mandelbrot_orbit(o)
        rgba, it = xctx.mandelbrot(pp(B, W, H, M))
        _, tr = xctx.mandelbrot(pp(B, W, H, M, flags=B.MANDEL_BLA_COUNT_TRIPS), want_rgba=False)
        ref = BD.orbit_plane(o, W, H, M)
        rtr = BD.orbit_plane(o, W, H, M, trips=True)
    assert np.array_equal(it, ref), (name, int((it != ref).sum()))
    assert np.array_equal(tr, rtr), (name, int((tr != rtr).sum()))
    assert len(np.unique(ref)) >= 10, (name, len(np.unique(ref)))
    lut, _ = O.mandel_lut(M)
    assert np.array_equal(bits(rgba), bits(lut[ref]))


@pytest.mark.parametrize("name,W,H,M,centre,scale", SHALLOW, ids=[v[0] for v in SHALLOW])
def test_shallow_planes_are_the_restatement(xctx, B, O, name, W, H, M, centre, scale):
    with shallow_orbit(B, centre, scale, M) as o:
        xctx.bind_mandelbrot_orbit(o)
        rgba, it = xctx.mandelbrot(pp(B, W, H, M))
        _, tr = xctx.mandelbrot(pp(B, W, H, M, flags=B.MANDEL_BLA_COUNT_TRIPS), want_rgba=False)
        ref = BD.orbit_plane(o, W, H, M)
        rtr = BD.orbit_plane(o, W, H, M, trips=True)
    assert np.array_equal(it, ref), (name, int((it != ref).sum()))
    assert np.array_equal(tr, rtr), (name, int((tr != rtr).sum()))
    lut, _ = O.mandel_lut(M)
    assert np.array_equal(bits(rgba), bits(lut[ref]))


def tile_row_list(H, row_begin, row_end, row_block, row_stride):
    if not row_stride:
        return list(range(row_begin, row_end))
    return [r for r in range(row_begin, row_end) if (r - row_begin) % row_stride < row_block]


def test_every_entry_point(xctx, B):
    import torch
    L = B.lib()
    L.mc_mandelbrot_render_rgba8.argtypes = [C.c_void_p, C.POINTER(B.MandelbrotParams), C.c_void_p]
    L.mc_context_warmup_mandelbrot.argtypes = [C.c_void_p, C.POINTER(B.MandelbrotParams), C.c_int]
    W, H, M = 203, 131, 6000
    with deep_orbit(B, D.M33, "1e-1000", M) as o:
        xctx.bind_mandelbrot_orbit(o)
        p = pp(B, W, H, M)
        rgba, whole = xctx.mandelbrot(p)
        assert len(np.unique(whole)) >= 10
        for rb, re_ in ((0, 1), (5, 37), (37, H), (H - 1, H)):
            _, t = xctx.mandelbrot(pp(B, W, H, M, row_begin=rb, row_end=re_))
            assert np.array_equal(t, whole[rb:re_]), (rb, re_)
        for rb, blk, stride in ((0, 8, 16), (3, 5, 20)):
            _, t = xctx.mandelbrot(pp(B, W, H, M, row_begin=rb, row_end=H, row_block=blk, row_stride=stride))
            assert np.array_equal(t, whole[tile_row_list(H, rb, H, blk, stride)]), (rb, blk, stride)
        t16 = torch.zeros((H, W), dtype=torch.int16, device="cuda")
        xctx.mandelbrot_device(pp(B, W, H, M, flags=B.MANDEL_ITERS_U16), 0, t16.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(t16.cpu().numpy().view(np.uint16).astype(np.uint32), whole)
        d_rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        d_it = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        s = torch.cuda.Stream()
        xctx.mandelbrot_device(p, d_rgba.data_ptr(), d_it.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        assert np.array_equal(d_it.cpu().numpy().astype(np.uint32), whole) and np.array_equal(bits(d_rgba.cpu().numpy()), bits(rgba))
        whole8 = xctx.convert_rgba8(rgba, 255.0)
        out = np.zeros((H, W, 4), np.uint8)
        assert L.mc_mandelbrot_render_rgba8(xctx._h, C.byref(p), out.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(out, whole8)
        for band_rows in (1000, 37):
            for rgba8 in (False, True):
                img, _ = xctx.mandelbrot_banded(pp(B, W, H, M), band_rows, rgba8=rgba8)
                want = whole8 if rgba8 else rgba
                assert np.array_equal(img.view(np.uint8), want.view(np.uint8)), (band_rows, rgba8)
        with B.Multi(1) as mm:                                   # multi-GPU: unsupported
            with pytest.raises(B.McError) as e:
                mm.mandelbrot(p)
            assert e.value.status == 5
        with B.Context(0) as c2:                                 # warm-up on a fresh context, then the render
            c2.bind_mandelbrot_orbit(o)
            for rgba8 in (0, 1, 2):
                assert L.mc_context_warmup_mandelbrot(c2._h, C.byref(p), rgba8) == 0
                rg, it2 = c2.mandelbrot(p)
                assert np.array_equal(it2, whole) and np.array_equal(bits(rg), bits(rgba))


def test_binding_rules(xctx, B):
    W, H, M = 40, 32, 2000
    with deep_orbit(B, D.M33, "1e-300", M) as a, shallow_orbit(B, K4, (1e-8, 1e-8), M) as b:
        xctx.bind_mandelbrot_orbit(a)
        _, ia = xctx.mandelbrot(pp(B, W, H, M))
        assert np.array_equal(ia, BD.orbit_plane(a, W, H, M))
        xctx.bind_mandelbrot_orbit(b)                       # a rebind switches views
        _, ib = xctx.mandelbrot(pp(B, W, H, M))
        assert np.array_equal(ib, BD.orbit_plane(b, W, H, M)) and not np.array_equal(ia, ib)
        with pytest.raises(B.McError) as e:                 # max_iter above the orbit's
            xctx.mandelbrot(pp(B, W, H, M + 1))
        assert e.value.status == 1
        with pytest.raises(B.McError) as e:                 # nonzero view words
            xctx.mandelbrot(B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_PERTURB_BLA_DEEP))
        assert e.value.status == 1
        xctx.bind_mandelbrot_orbit(None)                    # unbound: refused
        with pytest.raises(B.McError) as e:
            xctx.mandelbrot(pp(B, W, H, M))
        assert e.value.status == 1
    c, m, E = D.view(D.M33, "1e-300")
    with B.Orbit(c[0], c[1], *m, M, E) as plain:             # bound without the deep table: refused, PERTURB renders
        xctx.bind_mandelbrot_orbit(plain)
        with pytest.raises(B.McError) as e:
            xctx.mandelbrot(pp(B, W, H, M))
        assert e.value.status == 1 and "mc_mandelbrot_orbit_bla_deep" in str(e.value)
        _, ip = xctx.mandelbrot(B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_PERTURB, centre=(0.0, 0.0),
                                                    scale=(0.0, 0.0)))
        assert np.array_equal(ip, D.orbit_plane(plain, W, H, M))
    o = deep_orbit(B, D.M41, "1e-1000", M)                  # destroying the orbit after the bind changes nothing
    want = BD.orbit_plane(o, W, H, M)
    xctx.bind_mandelbrot_orbit(o)
    o.close()
    _, it = xctx.mandelbrot(pp(B, W, H, M))
    assert np.array_equal(it, want)


def test_precision_4_and_perturb_unchanged_with_both_tables(xctx, B):
    W, H, M = 64, 48, 4000
    with B.Orbit(*K4, 1e-20, 1e-20, M) as o:
        o.bla()
        o.bla_deep()
        xctx.bind_mandelbrot_orbit(o)
        q = dict(centre=(0.0, 0.0), scale=(0.0, 0.0))
        _, i3 = xctx.mandelbrot(B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_PERTURB, **q))
        _, i4 = xctx.mandelbrot(B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_PERTURB_BLA, **q))
        _, t4 = xctx.mandelbrot(B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_PERTURB_BLA,
                                                    flags=B.MANDEL_BLA_COUNT_TRIPS, **q), want_rgba=False)
        _, i5 = xctx.mandelbrot(pp(B, W, H, M))
        assert np.array_equal(i3, R.plane(o.table(), o.length, W, H, M, o.scale))
        assert np.array_equal(i4, BR.plane(o.table(), o.length, o.bla_table(), W, H, M, o.scale))
        assert np.array_equal(t4, BR.plane(o.table(), o.length, o.bla_table(), W, H, M, o.scale, trips=True))
        assert np.array_equal(i5, i4)                       # the parity of include/mc_compute.h on this view
    with B.Orbit("-0.75", "0.1", 0.75, 0.5, 200, scale_exp2=-1000) as deep:   # precision 4 still refuses a deep orbit
        deep.bla_deep()
        xctx.bind_mandelbrot_orbit(deep)
        with pytest.raises(B.McError) as e:
            xctx.mandelbrot(B.mandelbrot_params(W, H, max_iter=200, precision=B.PRECISION_PERTURB_BLA, centre=(0.0, 0.0),
                                                scale=(0.0, 0.0)))
        assert e.value.status == 5


def test_multi_refuses(B):
    with B.Orbit(*K4, 1e-8, 1e-8, 500) as o, B.Multi(1) as mm:
        o.bla_deep()
        with pytest.raises(B.McError) as e:
            mm.mandelbrot(pp(B, 32, 32, 500))
        assert e.value.status == 5


def test_full_size_sampled_rows(xctx, B):
    W, H, M = 7680, 5120, 6000
    with deep_orbit(B, D.M33, "1e-1000", M) as o:
        xctx.bind_mandelbrot_orbit(o)
        _, it = xctx.mandelbrot(pp(B, W, H, M), want_rgba=False)
        rows, cols = [0, 1777, 2560, H - 1], np.arange(0, W, 7)
        ref = BD.orbit_plane(o, W, H, M, rows=rows, cols=cols)
    assert np.array_equal(it[rows][:, cols], ref), int((it[rows][:, cols] != ref).sum())
    assert len(np.unique(ref)) >= 10


def test_app_end_to_end(B, O, tmp_path):
    W, H, M = 128, 96, 6000
    c, _, _ = D.view(D.M33, "1e-1000")
    m, E = B.scale_from_text("1e-1000")
    out = tmp_path / "deep_bla.png"
    r = subprocess.run([APP, "--precision", "perturb-bla-deep", "--width", str(W), "--height", str(H), "--max-iter", str(M), "--centre",
                        c[0], c[1], "--scale", "1e-1000", "1e-1000", "--out", str(out), "--quiet"], capture_output=True, text=True,
                       cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with B.Orbit(c[0], c[1], m, m, M, E) as o:
        o.bla_deep()
        ref = BD.orbit_plane(o, W, H, M)
    assert len(np.unique(ref)) >= 10
    lut, _ = O.mandel_lut(M)
    with B.Context(0) as ctx:
        want = ctx.convert_rgba8(np.ascontiguousarray(lut[ref]), 255.0)
    from PIL import Image
    img = np.asarray(Image.open(out).convert("RGBA"))
    assert np.array_equal(img, want)
