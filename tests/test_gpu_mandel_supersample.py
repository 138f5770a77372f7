"""MC_MANDEL_SUPERSAMPLE on the MI355X, every comparison bit for bit: the resolve kernel alone on synthetic sample planes (both count widths,
every factor, widths that make unaligned sample rows, heads and tails, with and without a map, contiguous and interleaved tiles), the
whole-image calls in all six precisions against the restatement (tests/mandel_supersample_ref.py) applied to the library's OWN plain count
plane of the sample grid, equalised + supersampled, bands and tiles, the identities (s = 0, 1; an all-interior view), every refusal, the app
end to end, one full-size frame."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mandel_equalise_ref as E
import mandel_perturb_deep_ref as D
import mandel_perturb_ref as R
import mandel_supersample_ref as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "mandelbrot")
K4 = R.DEEP_CENTRE
K4F = (float(K4[0]), float(K4[1]))
ZERO = dict(centre=(0.0, 0.0), scale=(0.0, 0.0))
INVALID, UNSUPPORTED = 1, 5
NEW_CALLS = ("mc_mandelbrot_supersample_params", "mc_mandelbrot_resolve_device_async")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want, what=""):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g, w), (what, int((g != w).any(axis=-1).sum()), "pixels differ")


def upload(values, u16, offset=0):
    """A torch device plane of the counts, `offset` elements into its allocation (offset > 0: a pointer aligned to the count's size only)."""
    import torch
    a = np.ascontiguousarray(values, np.uint16 if u16 else np.uint32).reshape(-1)
    buf = torch.zeros(a.size + offset, dtype=torch.int16 if u16 else torch.int32, device="cuda")
    buf[offset:] = torch.from_numpy(a.view(np.int16 if u16 else np.int32)).cuda()
    return buf, buf[offset:]


# ---- the resolve kernel alone ---------------------------------------------------------------------------------------------------
WIDTHS = [1, 2, 3, 63, 64, 65, 1001]


@pytest.mark.parametrize("u16", [False, True], ids=["u32", "u16"])
@pytest.mark.parametrize("s", S.FACTORS)
def test_resolve_of_synthetic_planes(ctx, B, s, u16):
    import torch
    M = 1000
    lut = B.colour_lut(M)
    rng = np.random.default_rng(100 * s + u16)
    map_ = np.sort(rng.integers(0, M + 1, size=M + 1)).astype(np.uint32)
    for W in WIDTHS:
        for tiling in (dict(), dict(row_begin=8, row_block=8, row_stride=24)):     # contiguous: 13 rows; interleaved: rows 8..15, 32..36
            H = 37 if tiling else 13
            p = B.mandelbrot_params(W, H, max_iter=M, supersample=s, **tiling)
            rows = B.tile_rows(p)
            assert rows == 13
            kinds = {
                "random": rng.integers(0, M + 1, size=(rows * s, W * s)),
                "equal": np.full((rows * s, W * s), 777),
                "above": rng.integers(M - 3, min(M + 500, 65535) + 1, size=(rows * s, W * s)),   # counts above max_iter: entry max_iter
                "blocks": np.repeat(np.repeat(rng.integers(0, M + 1, size=(rows, W)), s, axis=0), s, axis=1),   # every pixel flat
            }
            for kind, plane in kinds.items():
                for offset in (0, 1):
                    keep, d = upload(plane, u16, offset)
                    out = torch.full((rows, W, 4), -1.0, dtype=torch.float32, device="cuda")
                    guard = out.clone()
                    torch.cuda.synchronize()
                    for m in (None, map_):
                        ctx.mandelbrot_resolve_device(p, d.data_ptr(), 2 if u16 else 4, m, out.data_ptr())
                        ctx.synchronize()
                        same(out.cpu().numpy(), S.resolve(plane, s, M, lut, m), (W, kind, offset, m is not None, bool(tiling)))
                    assert (guard == -1.0).all()
                    del keep
            flat = S.resolve(kinds["blocks"], s, M, lut)
            same(flat, lut[kinds["blocks"][::s, ::s]], "flat pixels: the plain colour")


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


def sample_plane(ctx, B, p):
    """The library's own plain count plane of p's sample grid (the existing suites pin it to the oracle / the restatements)."""
    q = B.supersample_params(p)
    _, plane = ctx.mandelbrot(q, want_rgba=False)
    return q, plane


@pytest.mark.parametrize("which", range(6), ids=["f32", "ds", "f64", "perturb", "perturb-bla", "perturb-bla-deep"])
def test_whole_image_ragged(ctx, B, O, which):
    name, kw, make = six_views(B)[which]
    W, H, M = 101, 67, kw["max_iter"]
    lut = B.colour_lut(M)
    with bound_view(B, ctx, kw, make):
        for s in (2, 4, 8) if name in ("f32", "f64") else (2, 4):
            p = B.mandelbrot_params(W, H, supersample=s, **kw)
            q, plane = sample_plane(ctx, B, p)
            assert plane.shape == (s * H, s * W) and len(np.unique(plane)) >= 10, name
            if name == "f32":
                assert np.array_equal(plane, O.mandelbrot_iters(s * W, s * H, M))
            want = S.resolve(plane, s, M, lut)
            rgba, none = ctx.mandelbrot(p, want_iters=False)
            assert none is None
            same(rgba, want, (name, s))
            k, c = ctx.last_timing()
            assert k > 0 and c >= 0
            u8 = ctx.mandelbrot_rgba8(p)
            assert np.array_equal(u8, S.rgba8(want)), (name, s)
            assert np.array_equal(u8, ctx.convert_rgba8(rgba, 255.0))
            mixed, _ = S.mixed_share(plane, s)
            assert mixed > 0, (name, s)   # (the view exercises real sums, not only flat pixels)


def test_counts_beyond_uint16(ctx, B):
    """max_iter > 65535: the sample plane is uint32_t."""
    M, W, H, s = 70000, 64, 40, 2
    kw = dict(max_iter=M, precision=B.PRECISION_F32, centre=(-0.75, 0.05), scale=(0.3, 0.2))
    p = B.mandelbrot_params(W, H, supersample=s, **kw)
    _, plane = sample_plane(ctx, B, p)
    assert plane.max() > 65535
    rgba, _ = ctx.mandelbrot(p, want_iters=False)
    same(rgba, S.resolve(plane, s, M, B.colour_lut(M)))
    pe = B.mandelbrot_params(W, H, supersample=s, flags=B.MANDEL_COLOUR_EQUALISED, **kw)
    rgba, _ = ctx.mandelbrot(pe, want_iters=False)
    same(rgba, S.resolve(plane, s, M, B.colour_lut(M), E.rank_map(E.histogram(plane, M), M)))


# ---- equalised + supersampled ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 2, 3], ids=["f32", "f64", "perturb"])
def test_equalised_whole_image(ctx, B, which):
    name, kw, make = six_views(B)[which]
    W, H, M = 101, 67, kw["max_iter"]
    lut = B.colour_lut(M)
    with bound_view(B, ctx, kw, make):
        for s in (2, 4):
            p = B.mandelbrot_params(W, H, supersample=s, flags=B.MANDEL_COLOUR_EQUALISED, **kw)
            _, plane = sample_plane(ctx, B, p)
            hist = E.histogram(plane, M)
            assert int(hist.sum()) == s * s * W * H                       # the histogram of ALL samples
            m = E.rank_map(hist, M)
            want = S.resolve(plane, s, M, lut, m)
            rgba, _ = ctx.mandelbrot(p, want_iters=False)
            same(rgba, want, (name, s))
            assert np.array_equal(ctx.mandelbrot_rgba8(p), S.rgba8(want))
            plain, _ = ctx.mandelbrot(B.mandelbrot_params(W, H, supersample=s, **kw), want_iters=False)
            assert not np.array_equal(bits(plain), bits(rgba))


def test_by_hand_over_interleaved_tiles(ctx, B):
    import torch
    W, H, M, blk, n_tiles, s = 101, 67, 20000, 8, 2, 2
    kw = dict(max_iter=M, precision=B.PRECISION_F64, centre=K4F, scale=(1e-12, 1e-12 * 2 / 3))
    whole_eq, _ = ctx.mandelbrot(B.mandelbrot_params(W, H, supersample=s, flags=B.MANDEL_COLOUR_EQUALISED, **kw), want_iters=False)
    whole_plain, _ = ctx.mandelbrot(B.mandelbrot_params(W, H, supersample=s, **kw), want_iters=False)
    tiles = [B.mandelbrot_params(W, H, row_begin=t * blk, row_end=H, row_block=blk, row_stride=blk * n_tiles, supersample=s, **kw)
             for t in range(n_tiles)]
    padded = B.tile_rows(tiles[0])
    counts = torch.zeros((n_tiles, padded * s, W * s), dtype=torch.int16, device="cuda")
    colours = torch.zeros((n_tiles, padded, W, 4), dtype=torch.float32, device="cuda")
    hist = torch.zeros(M + 1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for t, p in enumerate(tiles):
        q = B.supersample_params(p)
        q.flags |= B.MANDEL_ITERS_U16
        assert B.tile_rows(q) == s * B.tile_rows(p)
        ctx.mandelbrot_device(q, 0, counts[t].data_ptr())
        ctx.mandelbrot_histogram_device(counts[t].data_ptr(), 2, B.tile_rows(q) * W * s, M, hist.data_ptr())
    ctx.synchronize()
    h = hist.cpu().numpy().view(np.uint32)
    assert int(h.sum()) == s * s * W * H
    m = B.equalise_map(M, h)
    out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    for map_, whole in ((m, whole_eq), (None, whole_plain), (m, whole_eq)):   # (the last: the cached composed table again)
        for t, p in enumerate(tiles):
            ctx.mandelbrot_resolve_device(p, counts[t].data_ptr(), 2, map_, colours[t].data_ptr())
        ctx.deinterleave_rows_device(colours.data_ptr(), W, H, n_tiles, blk, padded, 16, out.data_ptr())
        ctx.synchronize()
        same(out.cpu().numpy(), whole, map_ is not None)
    bad = m.copy()
    bad[5] = M + 1
    with pytest.raises(B.McError) as e:
        ctx.mandelbrot_resolve_device(tiles[0], counts[0].data_ptr(), 2, bad, colours[0].data_ptr())
    assert e.value.status == INVALID and "mc_mandelbrot_resolve_device_async" in str(e.value)


# ---- bands and tiles ------------------------------------------------------------------------------------------------------------
def test_bands_and_tiles_concatenate_to_the_whole_image(ctx, B):
    W, H, M = 101, 67, 20000
    kw = dict(max_iter=M, precision=B.PRECISION_F64, centre=K4F, scale=(1e-12, 1e-12 * 2 / 3))
    for s in (2, 4):
        whole, _ = ctx.mandelbrot(B.mandelbrot_params(W, H, supersample=s, **kw), want_iters=False)
        whole8 = ctx.mandelbrot_rgba8(B.mandelbrot_params(W, H, supersample=s, **kw))
        cuts = [0, 1, 8, 9, 40, H]
        tiles = [ctx.mandelbrot(B.mandelbrot_params(W, H, row_begin=a, row_end=b, supersample=s, **kw), want_iters=False)[0]
                 for a, b in zip(cuts, cuts[1:])]
        same(np.concatenate(tiles), whole, s)
        bands = [ctx.mandelbrot_rgba8(B.mandelbrot_params(W, H, row_begin=a, row_end=b, supersample=s, **kw)) for a, b in zip(cuts, cuts[1:])]
        assert np.array_equal(np.concatenate(bands), whole8)
        # an interleaved row tile of mc_mandelbrot_render: the rows it names, compactly
        p = B.mandelbrot_params(W, H, row_begin=8, row_end=H, row_block=8, row_stride=24, supersample=s, **kw)
        rows = [r for r in range(8, H) if (r - 8) % 24 < 8]
        tile, _ = ctx.mandelbrot(p, want_iters=False)
        same(tile, whole[rows], s)


# ---- identities -----------------------------------------------------------------------------------------------------------------
def test_factor_0_and_1_are_the_plain_image(ctx, B):
    W, H, M = 101, 67, 300
    for extra in (0, B.MANDEL_COLOUR_EQUALISED):
        plain, it = ctx.mandelbrot(B.mandelbrot_params(W, H, max_iter=M, flags=extra))
        plain8 = ctx.mandelbrot_rgba8(B.mandelbrot_params(W, H, max_iter=M, flags=extra))
        for s in (0, 1):
            p = B.mandelbrot_params(W, H, max_iter=M, flags=extra, supersample=s)
            rgba, it_s = ctx.mandelbrot(p)                      # out_iters is accepted: the existing path
            same(rgba, plain)
            assert np.array_equal(it_s, it)
            assert np.array_equal(ctx.mandelbrot_rgba8(p), plain8)
    p1 = B.mandelbrot_params(W, H, max_iter=M, supersample=1)
    banded, heard = ctx.mandelbrot_banded(p1, 16)               # calls that refuse s >= 2 take s = 1 as ever
    same(banded, B.colour_lut(M)[it])


def test_all_interior_view_equals_its_plain_image(ctx, B):
    """The flat-pixel identity on the device: -0.1 + 0.2 i at 1e-200 lies inside the main cardioid; every sample has n = M."""
    W, H, M = 53, 31, 400
    with B.Orbit("-0.1", "0.2", 1e-200, 1e-200, M) as o:
        ctx.bind_mandelbrot_orbit(o)
        try:
            kw = dict(max_iter=M, precision=B.PRECISION_PERTURB, **ZERO)
            plain, it = ctx.mandelbrot(B.mandelbrot_params(W, H, **kw))
            assert (it == M).all()
            for s in S.FACTORS:
                for extra in (0, B.MANDEL_COLOUR_EQUALISED):
                    rgba, _ = ctx.mandelbrot(B.mandelbrot_params(W, H, supersample=s, flags=extra, **kw), want_iters=False)
                    same(rgba, plain, (s, extra))
        finally:
            ctx.bind_mandelbrot_orbit(None)


def test_warmup_accepts_the_flag(B):
    L = B.lib()
    L.mc_context_warmup_mandelbrot.argtypes = [C.c_void_p, C.POINTER(B.MandelbrotParams), C.c_int]
    W, H, M = 64, 40, 300
    with B.Context(0) as c2:
        for s in S.FACTORS:
            for extra in (0, B.MANDEL_COLOUR_EQUALISED):
                p = B.mandelbrot_params(W, H, max_iter=M, supersample=s, flags=extra)
                for how in (0, 1, 3):
                    assert L.mc_context_warmup_mandelbrot(c2._h, C.byref(p), how) == 0
                _, plane = sample_plane(c2, B, p)
                m = E.rank_map(E.histogram(plane, M), M) if extra else None
                rgba, _ = c2.mandelbrot(p, want_iters=False)
                same(rgba, S.resolve(plane, s, M, B.colour_lut(M), m), (s, extra))
        bad = B.mandelbrot_params(W, H, max_iter=M, supersample=3)
        assert L.mc_context_warmup_mandelbrot(c2._h, C.byref(bad), 0) == INVALID


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, B):
    import torch
    W, H, M, s = 64, 48, 200, 2
    d_rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    d_it = torch.zeros((H * s, W * s), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def usable():
        rgba, it = ctx.mandelbrot(B.mandelbrot_params(W, H, max_iter=M))
        same(rgba, B.colour_lut(M)[it])

    def refused(call, status=INVALID, names=NEW_CALLS):
        with pytest.raises(B.McError) as e:
            call()
        assert e.value.status == status, e.value
        for n in names:
            assert n in str(e.value), e.value
        usable()

    ss = B.mandelbrot_params(W, H, max_iter=M, supersample=s)
    refused(lambda: ctx.mandelbrot_device(ss, d_rgba.data_ptr(), d_it.data_ptr()))
    refused(lambda: ctx.mandelbrot_banded(ss, 16))
    refused(lambda: ctx.mandelbrot_banded(ss, 16, rgba8=True))
    refused(lambda: ctx.mandelbrot_assemble_device(ss, d_it.data_ptr(), 4, 1, 8, H, d_rgba.data_ptr()))
    with B.Multi(1) as mm:
        refused(lambda: mm.mandelbrot(ss), UNSUPPORTED)
        refused(lambda: mm.mandelbrot_rgba8(ss), UNSUPPORTED)
    # out_iters: a pixel has no single count
    refused(lambda: ctx.mandelbrot(ss), names=("mc_mandelbrot_supersample_params",))
    refused(lambda: ctx.mandelbrot(ss, want_rgba=False), names=("mc_mandelbrot_supersample_params",))
    # invalid factors
    for bad in (3, 5, 6, 7, 9, 15):
        pb = B.mandelbrot_params(W, H, max_iter=M, supersample=bad)
        refused(lambda: ctx.mandelbrot(pb, want_iters=False), names=(f"MC_MANDEL_SUPERSAMPLE({bad})",))
        refused(lambda: ctx.mandelbrot_rgba8(pb), names=(f"MC_MANDEL_SUPERSAMPLE({bad})",))
        refused(lambda: ctx.mandelbrot_resolve_device(pb, d_it.data_ptr(), 4, None, d_rgba.data_ptr()), names=(f"MC_MANDEL_SUPERSAMPLE({bad})",))
    refused(lambda: ctx.mandelbrot_resolve_device(B.mandelbrot_params(W, H, max_iter=M), d_it.data_ptr(), 4, None, d_rgba.data_ptr()), names=())
    # equalised: whole images only, as without supersampling
    eq = B.MANDEL_COLOUR_EQUALISED
    refused(lambda: ctx.mandelbrot(B.mandelbrot_params(W, H, max_iter=M, row_end=H - 1, flags=eq, supersample=s), want_iters=False),
            names=("mc_mandelbrot_histogram_device_async",))
    refused(lambda: ctx.mandelbrot_rgba8(B.mandelbrot_params(W, H, max_iter=M, row_begin=8, flags=eq, supersample=s)),
            names=("mc_mandelbrot_histogram_device_async",))
    # an interleaved tile of render_rgba8, uint16 counts beyond 65535, a misaligned colour buffer
    refused(lambda: ctx.mandelbrot_rgba8(B.mandelbrot_params(W, H, max_iter=M, row_block=8, row_stride=16, supersample=s)), names=())
    refused(lambda: ctx.mandelbrot_resolve_device(B.mandelbrot_params(W, H, max_iter=70000, supersample=s), d_it.data_ptr(), 2, None,
                                                  d_rgba.data_ptr()), names=())
    refused(lambda: ctx.mandelbrot_resolve_device(ss, d_it.data_ptr(), 4, None, d_rgba.data_ptr() + 4), names=())
    # and the supersampled render still works
    _, plane = sample_plane(ctx, B, ss)
    rgba, _ = ctx.mandelbrot(ss, want_iters=False)
    same(rgba, S.resolve(plane, s, M, B.colour_lut(M)))


# ---- the app --------------------------------------------------------------------------------------------------------------------
def run_app(tmp_path, name, *args):
    out = tmp_path / name
    r = subprocess.run([APP, "--out", str(out), "--quiet"] + list(args), capture_output=True, text=True, cwd=tmp_path, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    from PIL import Image
    return np.asarray(Image.open(out).convert("RGBA")), r.stdout


def test_app_end_to_end(ctx, B, tmp_path):
    W, H, M, s = 160, 96, 300, 2
    size = ["--width", str(W), "--height", str(H), "--max-iter", str(M)]
    p = B.mandelbrot_params(W, H, max_iter=M, supersample=s)
    _, plane = sample_plane(ctx, B, p)
    lut = B.colour_lut(M)
    want_plain = S.rgba8(S.resolve(plane, s, M, lut))
    want_eq = S.rgba8(S.resolve(plane, s, M, lut, E.rank_map(E.histogram(plane, M), M)))
    assert not np.array_equal(want_plain, want_eq)
    for extra in ([], ["--gpu-postprocess"], ["--streamed-save"], ["--gpu-postprocess", "--streamed-save"]):
        img, text = run_app(tmp_path, "ss.png", "--supersample", "2", *size, *extra)
        assert np.array_equal(img, want_plain), extra
        assert ("--streamed-save has no effect" in text) == ("--streamed-save" in extra)
        img, _ = run_app(tmp_path, "ss_eq.png", "--supersample", "2", "--colour", "equalised", *size, *extra)
        assert np.array_equal(img, want_eq), extra
    img, _ = run_app(tmp_path, "one.png", "--supersample", "1", *size)
    assert np.array_equal(img, ctx.mandelbrot_rgba8(B.mandelbrot_params(W, H, max_iter=M)))
    # a perturbation view
    Md = 20000
    deep = ["--precision", "perturb", "--centre", K4[0], K4[1], "--scale", "1e-20", "1e-20", "--width", str(W), "--height", str(H),
            "--max-iter", str(Md)]
    with B.Orbit(K4[0], K4[1], 1e-20, 1e-20, Md) as o:
        ctx.bind_mandelbrot_orbit(o)
        try:
            _, plane = sample_plane(ctx, B, B.mandelbrot_params(W, H, max_iter=Md, precision=B.PRECISION_PERTURB, supersample=s, **ZERO))
        finally:
            ctx.bind_mandelbrot_orbit(None)
    img, _ = run_app(tmp_path, "deep.png", "--supersample", "2", "--gpu-postprocess", *deep)
    assert np.array_equal(img, S.rgba8(S.resolve(plane, s, Md, B.colour_lut(Md))))


# ---- full size ------------------------------------------------------------------------------------------------------------------
def test_k4_full_size(ctx, B):
    """K4's view, F64, s = 2, 7680 x 5120 (315 MB of uint16_t counts): sampled rows against the restatement."""
    W, H, M, s = 7680, 5120, 50000, 2
    kw = dict(max_iter=M, precision=B.PRECISION_F64, centre=K4F, scale=(1e-8, 1e-8 * 2 / 3))
    out = ctx.mandelbrot_rgba8(B.mandelbrot_params(W, H, supersample=s, **kw))
    assert out.shape == (H, W, 4)
    lut = B.colour_lut(M)
    mixed = []
    for r in (0, 1, 639, 640, 2559, 2560, 4097, H - 1):
        q = B.mandelbrot_params(W * s, H * s, row_begin=r * s, row_end=(r + 1) * s, **kw)
        _, plane = ctx.mandelbrot(q, want_rgba=False)
        assert np.array_equal(out[r], S.rgba8(S.resolve(plane, s, M, lut))[0]), r
        mixed.append(S.mixed_share(plane, s)[0])
    assert max(mixed) > 0   # (real sums, not only flat pixels)
    band = ctx.mandelbrot_rgba8(B.mandelbrot_params(W, H, row_begin=2560, row_end=2568, supersample=s, **kw))
    assert np.array_equal(band, out[2560:2568])
