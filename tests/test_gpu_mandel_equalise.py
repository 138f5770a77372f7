"""MC_MANDEL_COLOUR_EQUALISED on the MI355X: the histogram kernel against numpy.bincount exactly (the library's own planes in all six
precisions, uint32 and uint16; synthetic planes that stress the wave combining, the tails and both table schemes), the whole-image calls
against lut[map[n]] restated from their own counts (tests/mandel_equalise_ref.py), the by-hand route over interleaved tiles, every
refusal, the app end to end, one full-size frame."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mandel_equalise_ref as E
import mandel_perturb_deep_ref as D
import mandel_perturb_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "mandelbrot")
K4 = R.DEEP_CENTRE
K4F = (float(K4[0]), float(K4[1]))
ZERO = dict(centre=(0.0, 0.0), scale=(0.0, 0.0))
ONE_RANGE = 16383          # the largest max_iter whose table is one LDS range (16384 bins, 64 KB); 16384: the first with two
LDS_LAST = 64 * 16384 - 1  # the largest max_iter histogrammed through LDS ranges (64 of them); beyond: atomics on the global table
INVALID, UNSUPPORTED = 1, 5


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def device_histogram(ctx, plane, M, into=None):
    """The library's histogram of a torch plane (int32: uint32 counts, int16: uint16 counts), as a numpy uint32 table."""
    import torch
    hist = torch.zeros(M + 1, dtype=torch.int32, device="cuda") if into is None else into
    torch.cuda.synchronize()
    ctx.mandelbrot_histogram_device(plane.data_ptr(), plane.element_size(), plane.numel(), M, hist.data_ptr())
    ctx.synchronize()
    return hist.cpu().numpy().view(np.uint32)


def upload(values, u16=False):
    import torch
    a = np.ascontiguousarray(values, np.uint16 if u16 else np.uint32)
    return torch.from_numpy(a.view(np.int16 if u16 else np.int32)).cuda()


def check_histogram(ctx, values, M, u16=False):
    got = device_histogram(ctx, upload(values, u16), M)
    want = E.histogram(values, M)
    assert got.shape == want.shape and np.array_equal(got, want), (M, u16, int((got != want).sum()))
    assert int(got.sum(dtype=np.uint64)) == np.asarray(values).size


# ---- the library's own planes ---------------------------------------------------------------------------------------------------
def six_views(B):
    """(name, params keywords, orbit or None) per precision: the views of the existing GPU tests, small."""
    c33, m33, e33 = D.view(D.M33, "1e-1000")
    return [
        ("f32", dict(max_iter=256, precision=B.PRECISION_F32), None),
        ("ds", dict(max_iter=500, precision=B.PRECISION_DS, centre=K4F, scale=(1e-6, 1e-6)), None),
        ("f64", dict(max_iter=20000, precision=B.PRECISION_F64, centre=K4F, scale=(1e-12, 1e-12 * 2 / 3)), None),
        ("perturb", dict(max_iter=20000, precision=B.PRECISION_PERTURB, **ZERO), lambda: B.Orbit(K4[0], K4[1], 1e-20, 1e-20, 20000)),
        ("perturb-bla", dict(max_iter=20000, precision=B.PRECISION_PERTURB_BLA, **ZERO), lambda: B.Orbit(K4[0], K4[1], 1e-20, 1e-20, 20000)),
        ("perturb-bla-deep", dict(max_iter=6000, precision=B.PRECISION_PERTURB_BLA_DEEP, **ZERO),
         lambda: B.Orbit(c33[0], c33[1], m33[0], m33[1], 6000, e33)),
    ]


class bound_view:
    """Binds the view's orbit (with the tables its precision needs) to ctx for the block, and unbinds it afterwards."""

    def __init__(self, B, ctx, kw, make):
        self.B, self.ctx, self.kw, self.make, self.o = B, ctx, kw, make, None

    def __enter__(self):
        if self.make:
            self.o = self.make()
            if self.kw["precision"] == self.B.PRECISION_PERTURB_BLA:
                self.o.bla()
            if self.kw["precision"] == self.B.PRECISION_PERTURB_BLA_DEEP:
                self.o.bla_deep()
            self.ctx.bind_mandelbrot_orbit(self.o)
        return self

    def __exit__(self, *a):
        if self.o is not None:
            self.ctx.bind_mandelbrot_orbit(None)
            self.o.close()


@pytest.mark.parametrize("which", range(6), ids=["f32", "ds", "f64", "perturb", "perturb-bla", "perturb-bla-deep"])
def test_histogram_of_the_librarys_own_planes(ctx, B, which):
    import torch
    name, kw, make = six_views(B)[which]
    W, H, M = 203, 131, kw["max_iter"]
    with bound_view(B, ctx, kw, make):
        _, whole = ctx.mandelbrot(B.mandelbrot_params(W, H, **kw), want_rgba=False)
        assert len(np.unique(whole)) >= 10, name
        d32 = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        d16 = torch.zeros((H, W), dtype=torch.int16, device="cuda")
        ctx.mandelbrot_device(B.mandelbrot_params(W, H, **kw), 0, d32.data_ptr())
        ctx.mandelbrot_device(B.mandelbrot_params(W, H, flags=B.MANDEL_ITERS_U16, **kw), 0, d16.data_ptr())
        ctx.synchronize()
        want = E.histogram(whole, M)
        for plane in (d32, d16):
            got = device_histogram(ctx, plane, M)
            assert np.array_equal(got, want), (name, plane.dtype, int((got != want).sum()))


# ---- synthetic planes -----------------------------------------------------------------------------------------------------------
MS = [1, 100, ONE_RANGE, ONE_RANGE + 1, 50000, 200000, LDS_LAST, LDS_LAST + 1]


@pytest.mark.parametrize("M", MS)
def test_histogram_of_synthetic_planes(ctx, M):
    n = 300 * 1024 + 77
    rng = np.random.default_rng(M)
    lane = np.arange(n)
    wave = lane // 64
    planes = {
        "every pixel interior": np.full(n, M),
        "every pixel distinct": lane % (M + 1),
        "two values alternating lane by lane": np.where(lane % 2 == 0, M // 2, M),
        "a wave of 64 distinct values next to a wave of one": np.where(wave % 2 == 0, (lane * 7 + 3) % (M + 1), M // 3),
        "runs of equal values": (lane // 37) % (M + 1),
        "uniformly random": rng.integers(0, M + 1, n),
        "skewed random": np.minimum(rng.geometric(0.01, n) - 1, M),
        "values above M": rng.integers(0, 2 * M + 2, n),
    }
    for name, v in planes.items():
        check_histogram(ctx, v, M)
        if M <= 65535:
            check_histogram(ctx, np.minimum(v, 65535), M, u16=True)
    assert device_histogram(ctx, upload(planes["values above M"]), M)[M] == int((planes["values above M"] >= M).sum())


@pytest.mark.parametrize("n", [1, 3, 255, 257, 1000003])
def test_histogram_sizes_and_alignment(ctx, n):
    import torch
    M = 1000
    rng = np.random.default_rng(n)
    v = rng.integers(0, M + 1, n + 9)
    for u16 in (False, True):
        check_histogram(ctx, v[:n], M, u16=u16)
        whole = upload(v, u16)
        for off in (1, 3, 5):   # a plane that starts off a 16-byte boundary: the head is counted value by value
            part = whole[off:off + n]
            got = device_histogram(ctx, part, M)
            assert np.array_equal(got, E.histogram(v[off:off + n], M)), (n, u16, off)
    for M2 in (ONE_RANGE, ONE_RANGE + 1, 50000):
        check_histogram(ctx, rng.integers(0, M2 + 1, n), M2)


def test_histogram_adds_and_is_reproducible(ctx):
    import torch
    M = 50000
    rng = np.random.default_rng(3)
    a, b = rng.integers(0, M + 1, 500000), np.minimum(rng.geometric(0.001, 700001), M)
    for m_, va, vb in ((M, a, b), (500, a % 501, b % 501)):
        hist = torch.zeros(m_ + 1, dtype=torch.int32, device="cuda")
        first = device_histogram(ctx, upload(va), m_, into=hist).copy()
        both = device_histogram(ctx, upload(vb, u16=True), m_, into=hist)     # a second call adds to the first, whatever its format
        assert np.array_equal(first, E.histogram(va, m_))
        assert np.array_equal(both, E.histogram(np.concatenate([va, vb]), m_))
        again = device_histogram(ctx, upload(va), m_)
        assert np.array_equal(again, first)                                    # two runs, identical tables
    plane, hist = upload(a), torch.zeros(M + 1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.mandelbrot_histogram_device(plane.data_ptr(), 4, 0, M, hist.data_ptr())   # no pixels: nothing added
    ctx.synchronize()
    assert int(hist.cpu().numpy().sum()) == 0


def test_range_borders_and_the_switch_to_the_global_table(ctx):
    rng = np.random.default_rng(9)
    for M in (ONE_RANGE, ONE_RANGE + 1, 50000, 200000, LDS_LAST, LDS_LAST + 1):
        v = np.minimum(rng.geometric(0.003, 400001), M)
        check_histogram(ctx, v, M)
        check_histogram(ctx, M - v, M)                                                                     # the skew at the top range
        check_histogram(ctx, np.where(np.arange(100003) % 2 == 0, 16383, min(M, 16384)), M)              # astride a range border
        check_histogram(ctx, np.repeat(np.arange(0, M + 1, 16384), 300), M)                                # the first bin of every range


# ---- the whole-image calls ------------------------------------------------------------------------------------------------------
def check_whole_image(ctx, B, W, H, kw):
    M = kw["max_iter"]
    p = B.mandelbrot_params(W, H, flags=B.MANDEL_COLOUR_EQUALISED, **kw)
    plain = B.mandelbrot_params(W, H, **kw)
    rgba, it = ctx.mandelbrot(p)
    rgba_plain, it_plain = ctx.mandelbrot(plain)
    assert np.array_equal(it, it_plain)                                         # out_iters: the plain counts
    lut = B.colour_lut(M)
    want = E.colour(it, M, lut)
    assert np.array_equal(bits(rgba), bits(want)), int((bits(rgba) != bits(want)).any(axis=-1).sum())
    assert np.array_equal(bits(rgba_plain), bits(lut[it_plain]))               # without the flag: lut[n], as ever
    only_rgba, none = ctx.mandelbrot(p, want_iters=False)
    assert none is None and np.array_equal(bits(only_rgba), bits(want))
    _, only_it = ctx.mandelbrot(p, want_rgba=False)
    assert np.array_equal(only_it, it)
    assert np.array_equal(ctx.mandelbrot_rgba8(p), ctx.convert_rgba8(rgba, 255.0))
    assert np.array_equal(ctx.mandelbrot_rgba8(plain), ctx.convert_rgba8(rgba_plain, 255.0))
    k, c = ctx.last_timing()
    assert k > 0 and c >= 0
    return it, rgba


@pytest.mark.parametrize("which", range(6), ids=["f32", "ds", "f64", "perturb", "perturb-bla", "perturb-bla-deep"])
def test_whole_image_ragged(ctx, B, which):
    name, kw, make = six_views(B)[which]
    with bound_view(B, ctx, kw, make):
        it, rgba = check_whole_image(ctx, B, 203, 131, kw)
    assert len(np.unique(it)) >= 10


def test_whole_image_k4_width_band_height(ctx, B):
    kw = dict(max_iter=50000, precision=B.PRECISION_F64, centre=K4F, scale=(1e-8, 1e-8 / 12))   # K4's view, a 640-row band's aspect
    it, rgba = check_whole_image(ctx, B, 7680, 640, kw)
    M = 50000
    m = E.rank_map(E.histogram(it, M), M)
    assert E.percentile_span(it / M) < 0.05 and E.percentile_span(m[it] / M) > 0.9


def test_whole_image_all_interior_and_warmup(B):
    """E = 0: every pixel keeps the t = 1 colour; and a fresh context warmed up with the flag renders the same bytes."""
    L = B.lib()
    L.mc_context_warmup_mandelbrot.argtypes = [C.c_void_p, C.POINTER(B.MandelbrotParams), C.c_int]
    kw = dict(max_iter=300, precision=B.PRECISION_F32, centre=(-0.1, 0.0), scale=(0.01, 0.01))
    with B.Context(0) as c2:
        p = B.mandelbrot_params(64, 40, flags=B.MANDEL_COLOUR_EQUALISED, **kw)
        for how in (0, 1, 2, 3):
            assert L.mc_context_warmup_mandelbrot(c2._h, C.byref(p), how) == 0
        rgba, it = c2.mandelbrot(p)
        assert (it == 300).all()
        assert np.array_equal(bits(rgba), bits(np.broadcast_to(B.colour_lut(300)[300], rgba.shape)))
        q = B.mandelbrot_params(203, 131, max_iter=256, flags=B.MANDEL_COLOUR_EQUALISED)
        assert L.mc_context_warmup_mandelbrot(c2._h, C.byref(q), 1) == 0
        rgba, it = c2.mandelbrot(q)
        assert np.array_equal(bits(rgba), bits(E.colour(it, 256, B.colour_lut(256))))


# ---- by hand --------------------------------------------------------------------------------------------------------------------
def test_by_hand_over_interleaved_tiles(ctx, B):
    import torch
    W, H, M, blk, n_tiles = 203, 131, 20000, 8, 2
    kw = dict(max_iter=M, precision=B.PRECISION_F64, centre=K4F, scale=(1e-12, 1e-12 * 2 / 3))
    whole, it = ctx.mandelbrot(B.mandelbrot_params(W, H, flags=B.MANDEL_COLOUR_EQUALISED, **kw))
    tiles = [B.mandelbrot_params(W, H, row_begin=t * blk, row_end=H, row_block=blk, row_stride=blk * n_tiles, flags=B.MANDEL_ITERS_U16, **kw)
             for t in range(n_tiles)]
    padded = B.tile_rows(tiles[0])
    counts = torch.zeros((n_tiles, padded, W), dtype=torch.int16, device="cuda")
    colours = torch.zeros((n_tiles, padded, W, 4), dtype=torch.float32, device="cuda")
    hist = torch.zeros(M + 1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for t, p in enumerate(tiles):
        ctx.mandelbrot_device(p, 0, counts[t].data_ptr())
        ctx.mandelbrot_histogram_device(counts[t].data_ptr(), 2, B.tile_rows(p) * W, M, hist.data_ptr())
    ctx.synchronize()
    h = hist.cpu().numpy().view(np.uint32)
    assert np.array_equal(h, E.histogram(it, M))
    m = B.equalise_map(M, h)
    for t, p in enumerate(tiles):
        ctx.mandelbrot_recolour_device(p, counts[t].data_ptr(), 2, m, colours[t].data_ptr())
    out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    ctx.deinterleave_rows_device(colours.data_ptr(), W, H, n_tiles, blk, padded, 16, out.data_ptr())
    ctx.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(whole))
    # the same map again (the cached composed table), another map, and a map entry beyond M
    ctx.mandelbrot_recolour_device(tiles[0], counts[0].data_ptr(), 2, m, colours[0].data_ptr())
    ident = np.arange(M + 1, dtype=np.uint32)
    d32 = torch.from_numpy(it.view(np.int32)).cuda()
    full = B.mandelbrot_params(W, H, **kw)
    ctx.mandelbrot_recolour_device(full, d32.data_ptr(), 4, ident, out.data_ptr())
    ctx.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(B.colour_lut(M)[it]))   # the identity map: the plain colouring
    ident[5] = M + 1
    with pytest.raises(B.McError) as e:
        ctx.mandelbrot_recolour_device(full, d32.data_ptr(), 4, ident, out.data_ptr())
    assert e.value.status == INVALID


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, B):
    import torch
    W, H, M = 64, 48, 200
    f = B.MANDEL_COLOUR_EQUALISED
    d_rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    d_it = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def refused(call, status=INVALID, names=True):
        with pytest.raises(B.McError) as e:
            call()
        assert e.value.status == status, e.value
        if names:
            for s in ("mc_mandelbrot_histogram_device_async", "mc_mandelbrot_equalise_map", "mc_mandelbrot_recolour_device_async"):
                assert s in str(e.value), e.value

    refused(lambda: ctx.mandelbrot(B.mandelbrot_params(W, H, max_iter=M, row_begin=0, row_end=H - 1, flags=f)))
    refused(lambda: ctx.mandelbrot(B.mandelbrot_params(W, H, max_iter=M, row_begin=8, row_end=H, flags=f)))
    refused(lambda: ctx.mandelbrot(B.mandelbrot_params(W, H, max_iter=M, row_block=8, row_stride=16, flags=f)))
    refused(lambda: ctx.mandelbrot_rgba8(B.mandelbrot_params(W, H, max_iter=M, row_begin=0, row_end=H - 1, flags=f)))
    refused(lambda: ctx.mandelbrot_device(B.mandelbrot_params(W, H, max_iter=M, flags=f), d_rgba.data_ptr(), d_it.data_ptr()))
    refused(lambda: ctx.mandelbrot_banded(B.mandelbrot_params(W, H, max_iter=M, flags=f), 16))
    refused(lambda: ctx.mandelbrot_banded(B.mandelbrot_params(W, H, max_iter=M, flags=f), 16, rgba8=True))
    refused(lambda: ctx.mandelbrot_assemble_device(B.mandelbrot_params(W, H, max_iter=M, flags=f), d_it.data_ptr(), 4, 1, 8, H,
                                                   d_rgba.data_ptr()))
    with B.Multi(1) as mm:
        refused(lambda: mm.mandelbrot(B.mandelbrot_params(W, H, max_iter=M, flags=f)), UNSUPPORTED, names=False)
        refused(lambda: mm.mandelbrot_rgba8(B.mandelbrot_params(W, H, max_iter=M, flags=f)), UNSUPPORTED, names=False)
    refused(lambda: ctx.mandelbrot_histogram_device(d_it.data_ptr(), 3, W * H, M, d_rgba.data_ptr()), names=False)
    refused(lambda: ctx.mandelbrot_histogram_device(d_it.data_ptr(), 4, 2 ** 32, M, d_rgba.data_ptr()), names=False)
    refused(lambda: ctx.mandelbrot_histogram_device(d_it.data_ptr(), 4, W * H, 0, d_rgba.data_ptr()), names=False)
    # the context still renders, plain and equalised
    p = B.mandelbrot_params(W, H, max_iter=M, flags=f)
    rgba, it = ctx.mandelbrot(p)
    assert np.array_equal(bits(rgba), bits(E.colour(it, M, B.colour_lut(M))))
    rgba, it = ctx.mandelbrot(B.mandelbrot_params(W, H, max_iter=M))
    assert np.array_equal(bits(rgba), bits(B.colour_lut(M)[it]))


# ---- the app --------------------------------------------------------------------------------------------------------------------
def run_app(tmp_path, name, *args):
    out = tmp_path / name
    r = subprocess.run([APP, "--out", str(out), "--quiet"] + list(args), capture_output=True, text=True, cwd=tmp_path, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    from PIL import Image
    return np.asarray(Image.open(out).convert("RGBA")), r.stdout


def test_app_end_to_end(ctx, B, tmp_path):
    W, H = 160, 96
    f = B.MANDEL_COLOUR_EQUALISED
    size = ["--width", str(W), "--height", str(H)]
    # a shallow view (the reference's, M = 300)
    shallow = ["--max-iter", "300"] + size
    want_eq = ctx.mandelbrot_rgba8(B.mandelbrot_params(W, H, max_iter=300, flags=f))
    want_plain = ctx.mandelbrot_rgba8(B.mandelbrot_params(W, H, max_iter=300))
    assert not np.array_equal(want_eq, want_plain)
    for extra in ([], ["--gpu-postprocess"], ["--streamed-save"], ["--gpu-postprocess", "--streamed-save"]):
        img, text = run_app(tmp_path, "eq.png", "--colour", "equalised", *shallow, *extra)
        assert np.array_equal(img, want_eq), extra
        assert ("--streamed-save has no effect" in text) == ("--streamed-save" in extra)
    for extra in ([], ["--colour", "reference"], ["--gpu-postprocess"]):
        img, _ = run_app(tmp_path, "plain.png", *shallow, *extra)
        assert np.array_equal(img, want_plain), extra
    # a perturbation view
    M = 20000
    deep = ["--precision", "perturb", "--centre", K4[0], K4[1], "--scale", "1e-20", "1e-20", "--max-iter", str(M)] + size
    with B.Orbit(K4[0], K4[1], 1e-20, 1e-20, M) as o:
        ctx.bind_mandelbrot_orbit(o)
        try:
            want_eq = ctx.mandelbrot_rgba8(B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_PERTURB, flags=f, **ZERO))
            want_plain = ctx.mandelbrot_rgba8(B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_PERTURB, **ZERO))
        finally:
            ctx.bind_mandelbrot_orbit(None)
    img, _ = run_app(tmp_path, "deep_eq.png", "--colour", "equalised", "--gpu-postprocess", *deep)
    assert np.array_equal(img, want_eq)
    img, _ = run_app(tmp_path, "deep_plain.png", *deep)
    assert np.array_equal(img, want_plain)


# ---- full size ------------------------------------------------------------------------------------------------------------------
def test_k4_full_size(ctx, B):
    import torch
    W, H, M = 7680, 5120, 50000
    with B.Orbit(K4[0], K4[1], 1e-8, 1e-8 * 2 / 3, M) as o:
        ctx.bind_mandelbrot_orbit(o)
        try:
            d_it = torch.zeros((H, W), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ctx.mandelbrot_device(B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_PERTURB, **ZERO), 0, d_it.data_ptr())
            got = device_histogram(ctx, d_it, M)
        finally:
            ctx.bind_mandelbrot_orbit(None)
    plane = d_it.cpu().numpy().view(np.uint32)
    assert int(got.sum(dtype=np.uint64)) == 39321600
    assert np.array_equal(got, E.histogram(plane, M))
    again = device_histogram(ctx, d_it, M)
    assert np.array_equal(again, got)
