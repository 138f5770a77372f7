"""MC_PRECISION_F64 on the MI355X: iteration planes bit-exact against the numpy float64 restatement of the contract in include/mc_compute.h
(tests/mandel_f64_ref.py) on the reference view, a deep view that tells F64 from the two-float variant, an interior-heavy view (the
cycle exit), odd sizes and iteration counts (the tail), and the two views where |z|^2 lands on 2.0 exactly (the fast filter's false
positive); then every entry point that takes mc_mandelbrot_params against the blocking render."""
import ctypes as C

import numpy as np
import pytest

import mandel_f64_ref as R

pytestmark = pytest.mark.gpu

DEEP = dict(centre=R.DEEP_CENTRE, scale=(1e-12, 0.75e-12))           # 64 x 48, M = 20 000: ~46 % of pixels differ from DS
K4_VIEW = dict(centre=(-0.7436438870371587, 0.13182590420531198), scale=(1e-8, 1e-8 * 2.0 / 3.0))   # bench.K4_VIEW


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def f64(B, W, H, M, centre=(-0.445, 0.0), scale=(2.34, 2.34), **kw):
    return B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_F64, centre=centre, scale=scale, **kw)


def tile_row_list(H, row_begin, row_end, row_block, row_stride):
    """The storage rows of a tile, in the order the tile stores them (mc_mandelbrot_params: row_block / row_stride)."""
    if not row_stride:
        return list(range(row_begin, row_end))
    return [r for r in range(row_begin, row_end) if (r - row_begin) % row_stride < row_block]


@pytest.mark.parametrize("W,H,M,view", [
    (96, 64, 256, dict()),                                               # the reference view
    (64, 48, 20000, DEEP),                                               # deep: not DS's plane (below)
    (64, 48, 20000, dict(centre=(-0.3, 0.0), scale=(1.2, 0.9))),         # mostly interior, high M: the cycle exit
    (77, 45, 1003, dict(centre=(-0.75, 0.1), scale=(0.05, 0.03))),       # W, H not multiples of 8, M % 8 != 0
    (13, 5, 7, dict()),                                                  # M < U: only the tail
    (16, 12, 1000, dict(centre=(1.0, 1.0), scale=(1e-3, 1e-3))),         # c = (1, 1): |z_1|^2 = 2.0
    (16, 12, 1000, dict(centre=(0.0, 1.0), scale=(1e-3, 1e-3))),         # c = i: |z|^2 = 2.0 in every other iteration
])
def test_iteration_plane_is_the_restatement(ctx, B, O, W, H, M, view):
    rgba, it = ctx.mandelbrot(f64(B, W, H, M, **view))
    ref = R.mandelbrot_iters_f64(W, H, M, view.get("centre", (-0.445, 0.0)), view.get("scale", (2.34, 2.34)))
    assert np.array_equal(it, ref), int((it != ref).sum())
    lut, _ = O.mandel_lut(M)
    assert np.array_equal(bits(rgba), bits(lut[ref]))
    if view == DEEP:
        ds = O.mandelbrot_iters(W, H, M, view=O.make_view(*view["centre"], *view["scale"]), precision=1)
        assert (it != ds).mean() > 0.3
    if view.get("centre") in ((1.0, 1.0), (0.0, 1.0)):
        assert it[H // 2, W // 2] == (1 if view["centre"] == (1.0, 1.0) else M)


def test_row_tiles_are_rows_of_the_whole_image(ctx, B):
    W, H, M = 83, 70, 2000
    _, whole = ctx.mandelbrot(f64(B, W, H, M, **DEEP))
    for rb, re_ in ((0, 1), (5, 37), (37, H), (H - 1, H)):
        _, t = ctx.mandelbrot(f64(B, W, H, M, row_begin=rb, row_end=re_, **DEEP))
        assert np.array_equal(t, whole[rb:re_]), (rb, re_)
    for rb, blk, stride in ((0, 8, 16), (8, 8, 16), (3, 5, 20), (16, 8, 64)):
        _, t = ctx.mandelbrot(f64(B, W, H, M, row_begin=rb, row_end=H, row_block=blk, row_stride=stride, **DEEP))
        assert np.array_equal(t, whole[tile_row_list(H, rb, H, blk, stride)]), (rb, blk, stride)


def test_u16_counts_and_the_exchange_assembly(ctx, B):
    """The multi-GPU exchange form: 16-bit counts per interleaved tile, assembled into the image by mc_mandelbrot_assemble_device_async."""
    import torch
    W, H, M, n = 72, 50, 3000, 2
    whole_rgba, whole_it = ctx.mandelbrot(f64(B, W, H, M, **DEEP))
    p = f64(B, W, H, M, flags=B.MANDEL_ITERS_U16, **DEEP)
    t16 = torch.zeros((H, W), dtype=torch.int16, device="cuda")
    ctx.mandelbrot_device(p, 0, t16.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(t16.cpu().numpy().view(np.uint16).astype(np.uint32), whole_it)
    blk = B.lib().mc_row_block()
    padded = len([r for r in range(H) if (r // blk) % n == 0])
    tiles = torch.zeros((n, padded, W), dtype=torch.int16, device="cuda")
    for rank in range(n):
        q = f64(B, W, H, M, row_begin=rank * blk, row_end=H, row_block=blk, row_stride=n * blk, flags=B.MANDEL_ITERS_U16, **DEEP)
        ctx.mandelbrot_device(q, 0, tiles[rank].data_ptr())
    full = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    full_it = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    ctx.mandelbrot_assemble_device(f64(B, W, H, M, **DEEP), tiles.data_ptr(), 2, n, blk, padded, full.data_ptr(), full_it.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(full_it.cpu().numpy().astype(np.uint32), whole_it)
    assert np.array_equal(bits(full.cpu().numpy()), bits(whole_rgba))


def test_device_async_form(ctx, B):
    import torch
    W, H, M = 64, 48, 5000
    rgba, it = ctx.mandelbrot(f64(B, W, H, M, **DEEP))
    d_rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    d_it = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    ctx.mandelbrot_device(f64(B, W, H, M, **DEEP), d_rgba.data_ptr(), d_it.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(d_it.cpu().numpy().astype(np.uint32), it) and np.array_equal(bits(d_rgba.cpu().numpy()), bits(rgba))


def test_rgba8_and_banded_are_the_blocking_render_converted(ctx, B):
    L = B.lib()
    L.mc_mandelbrot_render_rgba8.argtypes = [C.c_void_p, C.POINTER(B.MandelbrotParams), C.c_void_p]
    W, H, M = 203, 131, 4000
    p = f64(B, W, H, M, **DEEP)
    whole, _ = ctx.mandelbrot(p, want_iters=False)
    whole8 = ctx.convert_rgba8(whole, 255.0)
    out = np.zeros((H, W, 4), np.uint8)
    assert L.mc_mandelbrot_render_rgba8(ctx._h, C.byref(p), out.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(out, whole8)
    for band_rows in (1000, 37):
        for rgba8 in (False, True):
            img, _ = ctx.mandelbrot_banded(f64(B, W, H, M, **DEEP), band_rows, rgba8=rgba8)
            want = whole8 if rgba8 else whole
            assert np.array_equal(img.view(np.uint8), want.view(np.uint8)), (band_rows, rgba8)


def test_warmup_then_render(ctx, B):
    L = B.lib()
    L.mc_context_warmup_mandelbrot.argtypes = [C.c_void_p, C.POINTER(B.MandelbrotParams), C.c_int]
    W, H, M = 120, 81, 3000
    p = f64(B, W, H, M, **DEEP)
    want, want_it = ctx.mandelbrot(p)
    for rgba8 in (0, 1):
        with B.Context(0) as c:
            assert L.mc_context_warmup_mandelbrot(c._h, C.byref(p), rgba8) == 0
            rg, it = c.mandelbrot(p)
            assert np.array_equal(it, want_it) and np.array_equal(bits(rg), bits(want))


def test_k4_view_full_size_sampled_rows(ctx, B):
    W, H, M = 7680, 5120, 50000
    _, it = ctx.mandelbrot(f64(B, W, H, M, **K4_VIEW), want_rgba=False)
    rows = [0, 1777, 2560, 4095, H - 1]
    ref = R.mandelbrot_iters_f64(W, H, M, K4_VIEW["centre"], K4_VIEW["scale"], rows=rows)
    assert np.array_equal(it[rows], ref), int((it[rows] != ref).sum())


def n_devices():
    import torch
    return torch.cuda.device_count()


@pytest.mark.skipif("n_devices() < 2", reason="needs two GPUs")
def test_multi_two_devices_equal_single(ctx, B):
    p = f64(B, 333, 170, 5000, **DEEP)
    with B.Multi(2) as m:
        rgba, it = m.mandelbrot(p)
    r1, i1 = ctx.mandelbrot(p)
    assert np.array_equal(it, i1) and np.array_equal(bits(rgba), bits(r1))


def test_multi_one_device(B):
    W, H, M = 77, 45, 3000
    with B.Multi(1) as m:
        rgba, it = m.mandelbrot(f64(B, W, H, M, **DEEP))
    assert np.array_equal(it, R.mandelbrot_iters_f64(W, H, M, DEEP["centre"], DEEP["scale"]))


def test_precision_beyond_f64_is_refused(ctx, B):
    for prec in (3, 4, 0xFFFFFFFF):
        p = B.mandelbrot_params(16, 16, max_iter=10, precision=prec)
        with pytest.raises(B.McError) as e:
            ctx.mandelbrot(p)
        assert e.value.status == 1    # MC_ERR_INVALID_ARGUMENT
