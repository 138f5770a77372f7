"""MC_PRECISION_PERTURB on the MI355X: iteration planes bit-exact against the numpy float64 restatement of the contract in
include/mc_compute.h (tests/mandel_perturb_ref.py), fed the library's own orbit table; every entry point that takes mc_mandelbrot_params
against the blocking render; the binding rules; the app end to end; sampled rows at full K4 size.  The tests bind orbits to a context of
their own (module scope), never to the session's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mandel_perturb_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K4 = R.DEEP_CENTRE
REF = ("-0.445", "0")


@pytest.fixture(scope="module")
def pctx(B):
    c = B.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def boundary():
    """A boundary point 2^-70 deep whose own orbit escapes (L < M = 4000): counts spread at 1e-20 around it."""
    return R.mp_boundary_point(("-0.5", "0"), ("-0.5", "1"), 4000, 70, 134)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def pp(B, W, H, M, **kw):
    """Params of a PERTURB render: the view is the bound orbit's, so the eight view words are zero."""
    return B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_PERTURB, centre=(0.0, 0.0), scale=(0.0, 0.0), **kw)


def tile_row_list(H, row_begin, row_end, row_block, row_stride):
    if not row_stride:
        return list(range(row_begin, row_end))
    return [r for r in range(row_begin, row_end) if (r - row_begin) % row_stride < row_block]


def bound(B, ctx, centre, scale, M):
    o = B.Orbit(centre[0], centre[1], scale[0], scale[1], M)
    ctx.bind_mandelbrot_orbit(o)
    return o


def restated(o, W, H, M, rows=None):
    return R.plane(o.table(), o.length, W, H, M, o.scale, rows=rows)


@pytest.mark.parametrize("name,W,H,M,centre,scale", [
    ("reference view", 96, 64, 256, REF, (2.34, 2.34)),
    ("K4 1e-8", 64, 48, 20000, K4, (1e-8, 1e-8 * 2 / 3)),
    ("K4 1e-20", 64, 48, 20000, K4, (1e-20, 1e-20)),
    ("interior-heavy 1e-14", 64, 48, 5000, ("-0.1", "0.2"), (1e-14, 1e-14)),
    ("1e-100", 40, 24, 3000, ("-0.75", "0.1"), (1e-100, 1e-100)),
    ("2^-950", 24, 16, 2000, ("-1.25", "0.001"), (2.0 ** -950, 2.0 ** -950)),
    ("odd sizes, M % 8 != 0", 77, 45, 1003, ("-0.75", "0.1"), (0.05, 0.03)),
    ("M < 8", 13, 5, 7, REF, (2.34, 2.34)),
])
def test_iteration_plane_is_the_restatement(pctx, B, O, name, W, H, M, centre, scale):
    with bound(B, pctx, centre, scale, M) as o:
        rgba, it = pctx.mandelbrot(pp(B, W, H, M))
        ref = restated(o, W, H, M)
    assert np.array_equal(it, ref), (name, int((it != ref).sum()))
    lut, _ = O.mandel_lut(M)
    assert np.array_equal(bits(rgba), bits(lut[ref]))


def test_escaping_reference_orbit(pctx, B, boundary):
    W, H, M = 64, 48, 4000
    with bound(B, pctx, boundary, (1e-20, 1e-20), M) as o:
        assert o.length < M
        _, it = pctx.mandelbrot(pp(B, W, H, M))
        ref = restated(o, W, H, M)
    assert np.array_equal(it, ref), int((it != ref).sum())
    assert len(np.unique(ref)) >= 20


VIEW = dict(centre=K4, scale=(1e-20, 1e-20))


def test_row_tiles_and_u16_are_the_whole_image(pctx, B):
    W, H, M = 83, 70, 4000
    with bound(B, pctx, VIEW["centre"], VIEW["scale"], M):
        _, whole = pctx.mandelbrot(pp(B, W, H, M))
        for rb, re_ in ((0, 1), (5, 37), (37, H), (H - 1, H)):
            _, t = pctx.mandelbrot(pp(B, W, H, M, row_begin=rb, row_end=re_))
            assert np.array_equal(t, whole[rb:re_]), (rb, re_)
        for rb, blk, stride in ((0, 8, 16), (8, 8, 16), (3, 5, 20)):
            _, t = pctx.mandelbrot(pp(B, W, H, M, row_begin=rb, row_end=H, row_block=blk, row_stride=stride))
            assert np.array_equal(t, whole[tile_row_list(H, rb, H, blk, stride)]), (rb, blk, stride)
        import torch
        t16 = torch.zeros((H, W), dtype=torch.int16, device="cuda")
        pctx.mandelbrot_device(pp(B, W, H, M, flags=B.MANDEL_ITERS_U16), 0, t16.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(t16.cpu().numpy().view(np.uint16).astype(np.uint32), whole)


def test_device_async_rgba8_banded_and_warmup(pctx, B):
    import torch
    L = B.lib()
    L.mc_mandelbrot_render_rgba8.argtypes = [C.c_void_p, C.POINTER(B.MandelbrotParams), C.c_void_p]
    L.mc_context_warmup_mandelbrot.argtypes = [C.c_void_p, C.POINTER(B.MandelbrotParams), C.c_int]
    W, H, M = 203, 131, 3000
    with bound(B, pctx, ("-0.74364388703715870475219150611477", "0.13182590420531197049161621529"), (1e-25, 1e-25), M):
        p = pp(B, W, H, M)
        rgba, it = pctx.mandelbrot(p)
        d_rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        d_it = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        s = torch.cuda.Stream()
        pctx.mandelbrot_device(p, d_rgba.data_ptr(), d_it.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        assert np.array_equal(d_it.cpu().numpy().astype(np.uint32), it) and np.array_equal(bits(d_rgba.cpu().numpy()), bits(rgba))
        whole8 = pctx.convert_rgba8(rgba, 255.0)
        out = np.zeros((H, W, 4), np.uint8)
        assert L.mc_mandelbrot_render_rgba8(pctx._h, C.byref(p), out.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(out, whole8)
        for band_rows in (1000, 37, 8):
            for rgba8 in (False, True):
                img, _ = pctx.mandelbrot_banded(pp(B, W, H, M), band_rows, rgba8=rgba8)
                want = whole8 if rgba8 else rgba
                assert np.array_equal(img.view(np.uint8), want.view(np.uint8)), (band_rows, rgba8)
        # the banded callback reports rows in order, up to the whole image
        seen = []
        cb = C.CFUNCTYPE(None, C.c_uint32, C.c_void_p)(lambda rows, user: seen.append(rows))
        fn = L.mc_mandelbrot_render_banded
        fn.argtypes = [C.c_void_p, C.POINTER(B.MandelbrotParams), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        buf = np.zeros((H, W, 4), np.float32)
        assert fn(pctx._h, C.byref(p), buf.ctypes.data_as(C.c_void_p), None, 37, C.cast(cb, C.c_void_p), None) == 0
        assert seen == sorted(seen) and seen[-1] == H and np.array_equal(bits(buf), bits(rgba))
    # warm-up on a fresh context, then the render
    with B.Context(0) as c, B.Orbit("-0.74364388703715870475219150611477", "0.13182590420531197049161621529", 1e-25, 1e-25, M) as o:
        c.bind_mandelbrot_orbit(o)
        for rgba8 in (0, 1, 2):
            assert L.mc_context_warmup_mandelbrot(c._h, C.byref(p), rgba8) == 0
            rg, it2 = c.mandelbrot(p)
            assert np.array_equal(it2, it) and np.array_equal(bits(rg), bits(rgba))


def test_binding_rules(pctx, B):
    W, H, M = 40, 32, 2000
    with B.Orbit(*K4, 1e-8, 1e-8, M) as a, B.Orbit(*REF, 2.34, 2.34, M) as b:
        pctx.bind_mandelbrot_orbit(a)
        _, ia = pctx.mandelbrot(pp(B, W, H, M))
        assert np.array_equal(ia, restated(a, W, H, M))
        pctx.bind_mandelbrot_orbit(b)                       # a rebind switches views
        _, ib = pctx.mandelbrot(pp(B, W, H, M))
        assert np.array_equal(ib, restated(b, W, H, M)) and not np.array_equal(ia, ib)
        with pytest.raises(B.McError) as e:                 # max_iter above the orbit's
            pctx.mandelbrot(pp(B, W, H, M + 1))
        assert e.value.status == 1
        with pytest.raises(B.McError) as e:                 # nonzero view words
            pctx.mandelbrot(B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_PERTURB))
        assert e.value.status == 1
        p = pp(B, W, H, M)
        p.scale_y_lo = 1e-30
        with pytest.raises(B.McError) as e:
            pctx.mandelbrot(p)
        assert e.value.status == 1
        pctx.bind_mandelbrot_orbit(None)                    # unbound: refused
        with pytest.raises(B.McError) as e:
            pctx.mandelbrot(pp(B, W, H, M))
        assert e.value.status == 1
    o = B.Orbit(*K4, 1e-8, 1e-8, M)                         # destroying the orbit after the bind changes nothing
    want = restated(o, W, H, M)
    pctx.bind_mandelbrot_orbit(o)
    o.close()
    _, it = pctx.mandelbrot(pp(B, W, H, M))
    assert np.array_equal(it, want)
    with B.Multi(1) as m:                                   # multi-GPU: unsupported
        with pytest.raises(B.McError) as e:
            m.mandelbrot(pp(B, W, H, M))
        assert e.value.status == 5


def test_app_end_to_end(B, O, tmp_path):
    W, H, M = 256, 192, 3000
    cx, cy = "-0.7436438870371587047521915061147740", "0.1318259042053119704916162152934971"   # 40-digit centre
    out = tmp_path / "perturb.png"
    r = subprocess.run([os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "mandelbrot"), "--precision", "perturb", "--width", str(W),
                        "--height", str(H), "--max-iter", str(M), "--centre", cx, cy, "--scale", "1e-30", "1e-30", "--out", str(out),
                        "--quiet"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with B.Orbit(cx, cy, 1e-30, 1e-30, M) as o:
        ref = restated(o, W, H, M)
    lut, _ = O.mandel_lut(M)
    with B.Context(0) as c:
        want = c.convert_rgba8(np.ascontiguousarray(lut[ref]), 255.0)
    from PIL import Image
    img = np.asarray(Image.open(out).convert("RGBA"))
    assert np.array_equal(img, want)


def test_k4_full_size_sampled_rows(pctx, B):
    W, H, M = 7680, 5120, 20000
    with bound(B, pctx, K4, (1e-20, 1e-20 * 2 / 3), M) as o:
        _, it = pctx.mandelbrot(pp(B, W, H, M), want_rgba=False)
        rows = [0, 1777, 2560, H - 1]
        cols = np.arange(0, W, 7)
        ref = R.plane(o.table(), o.length, W, H, M, o.scale, rows=rows, cols=cols)
    assert np.array_equal(it[rows][:, cols], ref), int((it[rows][:, cols] != ref).sum())


def test_binding_a_closed_orbit_is_refused(pctx, B):
    """A closed Orbit's handle is NULL, which the C call would read as "unbind": the binding refuses it and the binding stays."""
    W, H, M = 24, 16, 500
    with bound(B, pctx, REF, (2.34, 2.34), M) as o:
        want = restated(o, W, H, M)
    closed = B.Orbit(*K4, 1e-8, 1e-8, M)
    closed.close()
    with pytest.raises(ValueError):
        pctx.bind_mandelbrot_orbit(closed)
    _, it = pctx.mandelbrot(pp(B, W, H, M))
    assert np.array_equal(it, want)
