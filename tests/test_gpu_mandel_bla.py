"""MC_PRECISION_PERTURB_BLA on the MI355X: iteration planes and trip-count planes bit-exact against the numpy float64 restatement of the
contract in include/mc_compute.h (tests/mandel_bla_ref.py), fed the library's own orbit and BLA tables; every entry point that takes
mc_mandelbrot_params against the blocking render; the binding rules; the app end to end; sampled rows at full K4 size.  The tests bind
orbits to a context of their own (module scope), never to the session's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mandel_bla_ref as BR
import mandel_perturb_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K4 = R.DEEP_CENTRE
REF = ("-0.445", "0")


@pytest.fixture(scope="module")
def bctx(B):
    c = B.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def pp(B, W, H, M, **kw):
    """Params of a BLA render: the view is the bound orbit's, so the eight view words are zero."""
    return B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_PERTURB_BLA, centre=(0.0, 0.0), scale=(0.0, 0.0), **kw)


def tile_row_list(H, row_begin, row_end, row_block, row_stride):
    if not row_stride:
        return list(range(row_begin, row_end))
    return [r for r in range(row_begin, row_end) if (r - row_begin) % row_stride < row_block]


def bound(B, ctx, centre, scale, M):
    o = B.Orbit(centre[0], centre[1], scale[0], scale[1], M)
    o.bla()
    ctx.bind_mandelbrot_orbit(o)
    return o


def restated(o, W, H, M, rows=None, cols=None, trips=False):
    return BR.plane(o.table(), o.length, o.bla_table(), W, H, M, o.scale, rows=rows, cols=cols, trips=trips)


VIEWS = [
    ("reference view", 96, 64, 256, REF, (2.34, 2.34)),
    ("K4 1e-8", 64, 48, 20000, K4, (1e-8, 1e-8 * 2 / 3)),
    ("K4 1e-20", 64, 48, 20000, K4, (1e-20, 1e-20)),
    ("interior-heavy 1e-14", 64, 48, 5000, ("-0.1", "0.2"), (1e-14, 1e-14)),
    ("interior 1e-200", 64, 48, 20000, ("-0.1", "0.2"), (1e-200, 1e-200)),
    ("1e-100", 40, 24, 3000, ("-0.75", "0.1"), (1e-100, 1e-100)),
    ("2^-950", 24, 16, 2000, ("-1.25", "0.001"), (2.0 ** -950, 2.0 ** -950)),
    ("centre -1 (zeros in the orbit)", 40, 24, 1000, ("-1", "0"), (1e-10, 1e-10)),
    ("odd sizes, M % 8 != 0", 77, 45, 1003, ("-0.75", "0.1"), (0.05, 0.03)),
    ("M < 8", 13, 5, 7, REF, (2.34, 2.34)),
]


@pytest.mark.parametrize("name,W,H,M,centre,scale", VIEWS)
def test_iteration_plane_is_the_restatement(bctx, B, O, name, W, H, M, centre, scale):
    with bound(B, bctx, centre, scale, M) as o:
        rgba, it = bctx.mandelbrot(pp(B, W, H, M))
        ref = restated(o, W, H, M)
    assert np.array_equal(it, ref), (name, int((it != ref).sum()))
    lut, _ = O.mandel_lut(M)
    assert np.array_equal(bits(rgba), bits(lut[ref]))


@pytest.mark.parametrize("name,W,H,M,centre,scale", [v for v in VIEWS if v[0] in ("K4 1e-20", "interior 1e-200", "1e-100",
                                                                                   "odd sizes, M % 8 != 0", "reference view")])
def test_trip_counts_are_the_restatement(bctx, B, name, W, H, M, centre, scale):
    with bound(B, bctx, centre, scale, M) as o:
        _, tr = bctx.mandelbrot(pp(B, W, H, M, flags=B.MANDEL_BLA_COUNT_TRIPS), want_rgba=False)
        ref = restated(o, W, H, M, trips=True)
    assert np.array_equal(tr, ref), (name, int((tr != ref).sum()))
    assert tr.min() >= 1 and tr.max() <= M


def test_boundary_view_and_skipping(bctx, B):
    """An escaping reference (L < M) at 1e-20 around a boundary point: planes equal, and the trips are fewer than the counts (the
    offset outgrows the radii early near the boundary: about a quarter of the iterations are skipped here)."""
    W, H, M = 64, 48, 4000
    centre = R.mp_boundary_point(("-0.5", "0"), ("-0.5", "1"), M, 70, 134)
    with bound(B, bctx, centre, (1e-20, 1e-20), M) as o:
        assert o.length < M
        _, it = bctx.mandelbrot(pp(B, W, H, M))
        _, tr = bctx.mandelbrot(pp(B, W, H, M, flags=B.MANDEL_BLA_COUNT_TRIPS), want_rgba=False)
        ref = restated(o, W, H, M)
    assert np.array_equal(it, ref), int((it != ref).sum())
    assert len(np.unique(ref)) >= 20
    assert tr.astype(np.float64).mean() < 0.9 * np.minimum(it.astype(np.int64) + 1, M).mean()


VIEW = dict(centre=K4, scale=(1e-20, 1e-20))


def test_row_tiles_and_u16_are_the_whole_image(bctx, B):
    W, H, M = 83, 70, 4000
    with bound(B, bctx, VIEW["centre"], VIEW["scale"], M):
        _, whole = bctx.mandelbrot(pp(B, W, H, M))
        for rb, re_ in ((0, 1), (5, 37), (37, H), (H - 1, H)):
            _, t = bctx.mandelbrot(pp(B, W, H, M, row_begin=rb, row_end=re_))
            assert np.array_equal(t, whole[rb:re_]), (rb, re_)
        for rb, blk, stride in ((0, 8, 16), (8, 8, 16), (3, 5, 20)):
            _, t = bctx.mandelbrot(pp(B, W, H, M, row_begin=rb, row_end=H, row_block=blk, row_stride=stride))
            assert np.array_equal(t, whole[tile_row_list(H, rb, H, blk, stride)]), (rb, blk, stride)
        import torch
        t16 = torch.zeros((H, W), dtype=torch.int16, device="cuda")
        bctx.mandelbrot_device(pp(B, W, H, M, flags=B.MANDEL_ITERS_U16), 0, t16.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(t16.cpu().numpy().view(np.uint16).astype(np.uint32), whole)


def test_device_async_rgba8_banded_and_warmup(bctx, B):
    import torch
    L = B.lib()
    L.mc_mandelbrot_render_rgba8.argtypes = [C.c_void_p, C.POINTER(B.MandelbrotParams), C.c_void_p]
    L.mc_context_warmup_mandelbrot.argtypes = [C.c_void_p, C.POINTER(B.MandelbrotParams), C.c_int]
    W, H, M = 203, 131, 3000
    centre = ("-0.74364388703715870475219150611477", "0.13182590420531197049161621529")
    with bound(B, bctx, centre, (1e-25, 1e-25), M):
        p = pp(B, W, H, M)
        rgba, it = bctx.mandelbrot(p)
        d_rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        d_it = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        s = torch.cuda.Stream()
        bctx.mandelbrot_device(p, d_rgba.data_ptr(), d_it.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        assert np.array_equal(d_it.cpu().numpy().astype(np.uint32), it) and np.array_equal(bits(d_rgba.cpu().numpy()), bits(rgba))
        whole8 = bctx.convert_rgba8(rgba, 255.0)
        out = np.zeros((H, W, 4), np.uint8)
        assert L.mc_mandelbrot_render_rgba8(bctx._h, C.byref(p), out.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(out, whole8)
        for band_rows in (1000, 37, 8):
            for rgba8 in (False, True):
                img, _ = bctx.mandelbrot_banded(pp(B, W, H, M), band_rows, rgba8=rgba8)
                want = whole8 if rgba8 else rgba
                assert np.array_equal(img.view(np.uint8), want.view(np.uint8)), (band_rows, rgba8)
    # warm-up on a fresh context, then the render
    with B.Context(0) as c, B.Orbit(centre[0], centre[1], 1e-25, 1e-25, M) as o:
        o.bla()
        c.bind_mandelbrot_orbit(o)
        for rgba8 in (0, 1, 2):
            assert L.mc_context_warmup_mandelbrot(c._h, C.byref(p), rgba8) == 0
            rg, it2 = c.mandelbrot(p)
            assert np.array_equal(it2, it) and np.array_equal(bits(rg), bits(rgba))


def test_binding_rules(bctx, B):
    W, H, M = 40, 32, 2000
    with B.Orbit(*K4, 1e-8, 1e-8, M) as a, B.Orbit(*REF, 2.34, 2.34, M) as b:
        a.bla()
        b.bla()
        bctx.bind_mandelbrot_orbit(a)
        _, ia = bctx.mandelbrot(pp(B, W, H, M))
        assert np.array_equal(ia, restated(a, W, H, M))
        bctx.bind_mandelbrot_orbit(b)                       # a rebind switches views
        _, ib = bctx.mandelbrot(pp(B, W, H, M))
        assert np.array_equal(ib, restated(b, W, H, M)) and not np.array_equal(ia, ib)
        with pytest.raises(B.McError) as e:                 # max_iter above the orbit's
            bctx.mandelbrot(pp(B, W, H, M + 1))
        assert e.value.status == 1
        with pytest.raises(B.McError) as e:                 # nonzero view words
            bctx.mandelbrot(B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_PERTURB_BLA))
        assert e.value.status == 1
        with B.Multi(1) as m:                               # multi-GPU: unsupported
            with pytest.raises(B.McError) as e:
                m.mandelbrot(pp(B, W, H, M))
            assert e.value.status == 5
        bctx.bind_mandelbrot_orbit(None)                    # unbound: refused
        with pytest.raises(B.McError) as e:
            bctx.mandelbrot(pp(B, W, H, M))
        assert e.value.status == 1
    with B.Orbit(*K4, 1e-8, 1e-8, M) as plain:              # bound without a table: BLA refused, PERTURB renders
        bctx.bind_mandelbrot_orbit(plain)
        with pytest.raises(B.McError) as e:
            bctx.mandelbrot(pp(B, W, H, M))
        assert e.value.status == 1 and "mc_mandelbrot_orbit_bla" in str(e.value)
        _, ip = bctx.mandelbrot(B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_PERTURB, centre=(0.0, 0.0),
                                                    scale=(0.0, 0.0)))
        assert np.array_equal(ip, R.plane(plain.table(), plain.length, W, H, M, plain.scale))
    with B.Orbit("-0.75", "0.1", 0.75, 0.5, 200, scale_exp2=-1000) as deep:   # a deep orbit: unsupported
        assert deep.deep
        bctx.bind_mandelbrot_orbit(deep)
        with pytest.raises(B.McError) as e:
            bctx.mandelbrot(pp(B, W, H, 200))
        assert e.value.status == 5
    o = B.Orbit(*K4, 1e-8, 1e-8, M)                         # destroying the orbit after the bind changes nothing
    o.bla()
    want = restated(o, W, H, M)
    bctx.bind_mandelbrot_orbit(o)
    o.close()
    _, it = bctx.mandelbrot(pp(B, W, H, M))
    assert np.array_equal(it, want)


def test_perturb_on_a_bla_binding_is_unchanged(bctx, B):
    """An orbit with a table still renders PERTURB exactly as the PERTURB restatement says."""
    W, H, M = 64, 48, 4000
    with bound(B, bctx, K4, (1e-20, 1e-20), M) as o:
        _, it = bctx.mandelbrot(B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_PERTURB, centre=(0.0, 0.0),
                                                    scale=(0.0, 0.0)))
        assert np.array_equal(it, R.plane(o.table(), o.length, W, H, M, o.scale))


def test_app_end_to_end(B, O, tmp_path):
    W, H, M = 256, 192, 3000
    cx, cy = "-0.7436438870371587047521915061147740", "0.1318259042053119704916162152934971"   # 40-digit centre
    out = tmp_path / "bla.png"
    r = subprocess.run([os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "mandelbrot"), "--precision", "perturb-bla", "--width",
                        str(W), "--height", str(H), "--max-iter", str(M), "--centre", cx, cy, "--scale", "1e-30", "1e-30", "--out",
                        str(out), "--quiet"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with B.Orbit(cx, cy, 1e-30, 1e-30, M) as o:
        o.bla()
        ref = restated(o, W, H, M)
    lut, _ = O.mandel_lut(M)
    with B.Context(0) as c:
        want = c.convert_rgba8(np.ascontiguousarray(lut[ref]), 255.0)
    from PIL import Image
    img = np.asarray(Image.open(out).convert("RGBA"))
    assert np.array_equal(img, want)


def test_k4_full_size_sampled_rows(bctx, B):
    W, H, M = 7680, 5120, 20000
    with bound(B, bctx, K4, (1e-20, 1e-20 * 2 / 3), M) as o:
        _, it = bctx.mandelbrot(pp(B, W, H, M), want_rgba=False)
        rows = [0, 1777, 2560, H - 1]
        cols = np.arange(0, W, 7)
        ref = restated(o, W, H, M, rows=rows, cols=cols)
    assert np.array_equal(it[rows][:, cols], ref), int((it[rows][:, cols] != ref).sum())
