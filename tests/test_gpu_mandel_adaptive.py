"""MC_MANDEL_SUPERSAMPLE_ADAPTIVE on the MI355X, every comparison bit for bit: the refine list alone on synthetic planes (both count
widths; the list compared SORTED, its order is unspecified), the whole-image calls in all six precisions against the restatement
(tests/mandel_adaptive_ref.py) applied to the library's OWN plain count plane of the sample grid, the report, equalised + adaptive, an
all-interior view (an empty list launches nothing), counts beyond uint16_t, run-to-run identity, the warm-up, every refusal, the app."""
import ctypes as C

import numpy as np
import pytest

import mandel_adaptive_ref as A
import mandel_block_audit_cases as K
import mandel_equalise_ref as E
import mandel_perturb_ref as R
import mandel_supersample_ref as S
from test_gpu_mandel_supersample import ZERO, bits, bound_view, run_app, same, sample_plane, six_views, upload

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 5


# ---- the refine list alone ------------------------------------------------------------------------------------------------------
def refine(ctx, plane, u16):
    import torch
    plane = np.asarray(plane)
    H, W = plane.shape
    keep, d = upload(plane, u16)
    lst = torch.full((W * H + 8,), -1, dtype=torch.int32, device="cuda")
    count = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.test_mandel_refine(d.data_ptr(), 2 if u16 else 4, W, H, lst.data_ptr(), count.data_ptr())
    ctx.synchronize()
    n = int(count.cpu().numpy().view(np.uint32)[0])
    assert count.cpu().tolist()[1:] == [77, 77, 77]
    out = lst.cpu().numpy().view(np.uint32)
    assert n <= W * H and (out[n:] == 0xffffffff).all()       # nothing written beyond the list's length
    del keep
    return np.sort(out[:n])


@pytest.mark.parametrize("u16", [False, True], ids=["u32", "u16"])
def test_refine_list_of_synthetic_planes(ctx, u16):
    rng = np.random.default_rng(7 + u16)
    top = 65535 if u16 else 2 ** 32 - 1

    def check(plane, what):
        got = refine(ctx, plane, u16)
        assert np.array_equal(got, A.refined_list(plane)), what
        return got

    # one odd pixel in a flat plane: exactly its 3 x 3 block, clipped at corners and borders
    for H, W in ((9, 13), (5, 64), (70, 3)):
        for y, x in ((H // 2, W // 2), (0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H // 2, 0), (H - 1, W // 2), (H // 2, W - 1)):
            plane = np.full((H, W), 500)
            plane[y, x] = top                                             # (the full width of the count)
            got = check(plane, (H, W, y, x))
            want = [yy * W + xx for yy in range(max(y - 1, 0), min(y + 2, H)) for xx in range(max(x - 1, 0), min(x + 2, W))]
            assert got.tolist() == want
    # W = 1, H = 1, 1 x 1
    check(np.array([[3]]), "1 x 1")
    assert refine(ctx, np.array([[3]]), u16).size == 0
    col = rng.integers(0, 3, size=(200, 1))
    row = rng.integers(0, 3, size=(1, 200))
    check(col, "W = 1")
    check(row, "H = 1")
    # a checkerboard: all refined; a flat plane: length 0
    for W in (63, 64, 65, 1001):
        board = np.indices((37, W)).sum(axis=0) % 2
        assert check(board, ("board", W)).size == 37 * W
        assert check(np.full((37, W), 12345), ("flat", W)).size == 0
        # banded and random planes at the widths that put wave and row boundaries everywhere
        check(np.repeat(rng.integers(0, 1000, size=(37, (W + 6) // 7)), 7, axis=1)[:, :W], ("bands", W))
        check(rng.integers(0, 2, size=(37, W)) * rng.integers(0, 2, size=(37, W)) * 9, ("random", W))
        blocks = np.repeat(np.repeat(rng.integers(0, 50, size=(5, (W + 15) // 16)), 8, axis=0), 16, axis=1)[:37, :W]
        check(blocks, ("blocks", W))


# ---- the library's own planes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(6), ids=["f32", "ds", "f64", "perturb", "perturb-bla", "perturb-bla-deep"])
def test_whole_image_ragged(ctx, B, O, which):
    name, kw, make = six_views(B)[which]
    W, H, M = 101, 67, kw["max_iter"]
    lut = B.colour_lut(M)
    with bound_view(B, ctx, kw, make):
        plain_rgba, plain_it = ctx.mandelbrot(B.mandelbrot_params(W, H, **kw))
        for s in (2, 4, 8) if name in ("f32", "f64") else (2, 4):
            p = B.mandelbrot_params(W, H, supersample=s, adaptive=True, **kw)
            q, plane = sample_plane(ctx, B, p)
            assert plane.shape == (s * H, s * W) and q.flags & B.MANDEL_SUPERSAMPLE_ADAPTIVE == 0
            assert np.array_equal(A.anchor_plane(plane, s), plain_it), (name, s)        # the anchor identity on the device
            want, mask = A.image(plane, s, M, lut)
            full = S.resolve(plane, s, M, lut)
            miss = A.missed(plane, s, mask)
            print(f"{name} s = {s}: refined {int(mask.sum())} of {W * H}, missed {int(miss.sum())}, "
                  f"differing from full supersampling {int((bits(want) != bits(full)).any(axis=-1).sum())}")
            assert 0 < mask.sum() < W * H, (name, s)
            rgba, none = ctx.mandelbrot(p, want_iters=False)
            assert none is None
            same(rgba, want, (name, s))
            assert ctx.last_refined() == (int(mask.sum()), W * H), (name, s)
            same(rgba[~mask], plain_rgba[~mask], (name, s, "unrefined: the plain colour"))
            k, c = ctx.last_timing()
            assert k > 0 and c >= 0
            u8 = ctx.mandelbrot_rgba8(p)
            assert np.array_equal(u8, S.rgba8(want)), (name, s)
            assert np.array_equal(u8, ctx.convert_rgba8(rgba, 255.0))
            assert ctx.last_refined() == (int(mask.sum()), W * H)
            if name == "f32":   # the oracle's numbers (tests/test_mandel_adaptive_host.py): this is not the full grid's image
                assert np.array_equal(plane, O.mandelbrot_iters(s * W, s * H, M))
                assert int(mask.sum()) == 2614 and int(miss.sum()) == {2: 2, 4: 7, 8: 16}[s]
                assert (bits(rgba) != bits(full)).any()
                full_lib, _ = ctx.mandelbrot(B.mandelbrot_params(W, H, supersample=s, **kw), want_iters=False)
                same(full_lib, full)
                differ = (bits(rgba) != bits(full_lib)).any(axis=-1)
                assert differ.any() and not differ[~miss].any()


@pytest.mark.parametrize("which", range(6), ids=["f32", "ds", "f64", "perturb", "perturb-bla", "perturb-bla-deep"])
def test_equalised_whole_image(ctx, B, which):
    name, kw, make = six_views(B)[which]
    W, H, M = 101, 67, kw["max_iter"]
    lut = B.colour_lut(M)
    eq = B.MANDEL_COLOUR_EQUALISED
    with bound_view(B, ctx, kw, make):
        plain_eq, plain_it = ctx.mandelbrot(B.mandelbrot_params(W, H, flags=eq, **kw))
        for s in (2, 4):
            p = B.mandelbrot_params(W, H, supersample=s, adaptive=True, flags=eq, **kw)
            _, plane = sample_plane(ctx, B, p)
            want, mask = A.image(plane, s, M, lut, equalised=True)
            rgba, _ = ctx.mandelbrot(p, want_iters=False)
            same(rgba, want, (name, s))
            assert ctx.last_refined() == (int(mask.sum()), W * H)
            same(rgba[~mask], plain_eq[~mask], "unrefined: the plain equalised image")   # (the ANCHOR plane's histogram)
            assert np.array_equal(ctx.mandelbrot_rgba8(p), S.rgba8(want))
            # and it is not the fully supersampled equalised image's map (that one's histogram is of all samples)
            not_eq, _ = ctx.mandelbrot(B.mandelbrot_params(W, H, supersample=s, adaptive=True, **kw), want_iters=False)
            assert not np.array_equal(bits(not_eq), bits(rgba))


# ---- the two engines of the list mapping that the six views do not reach (DESIGN.md §3.29's table) ---------------------------------
# 24 x 20 pixels: partial tiles on both axes; s = 2 and s = 8: sixteen pixels per wave and one pixel per wave.
@pytest.mark.parametrize("s", [2, 8])
def test_list_render_of_the_contracted_fp32_loop(ctx, B, s):
    """MC_MANDEL_FMA (StateF32<true>): the sample grid's plane by the tile kernel against the contracted loop restated on the host, the
    adaptive image by the list kernel against the restatement over that plane."""
    W, H, M = 24, 20, 256
    p = B.mandelbrot_params(W, H, max_iter=M, supersample=s, adaptive=True, flags=B.MANDEL_FMA)
    q, plane = sample_plane(ctx, B, p)
    assert q.flags & B.MANDEL_FMA
    assert np.array_equal(plane, K.fma_iters(s * W, s * H, M, (-0.445, 0.0), (2.34, 2.34)))
    want, mask = A.image(plane, s, M, B.colour_lut(M))
    assert 0 < mask.sum() < W * H
    rgba, _ = ctx.mandelbrot(p, want_iters=False)
    same(rgba, want, s)
    assert ctx.last_refined() == (int(mask.sum()), W * H)


@pytest.mark.parametrize("s", [2, 8])
def test_list_render_by_the_forced_deep_kernel(ctx, B, s):
    """MC_PRECISION_PERTURB under MC_MANDEL_PERTURB_FORCE_DEEP (StateDeep) on a short shallow orbit: the sample grid's plane by the tile
    kernel against PERTURB's loop restated on the host, the adaptive image by the list kernel against the restatement over that plane."""
    W, H, M = 24, 20, 200
    kw = dict(max_iter=M, precision=B.PRECISION_PERTURB, flags=B.MANDEL_PERTURB_FORCE_DEEP, **ZERO)
    with bound_view(B, ctx, kw, lambda: B.Orbit("-0.75", "0.1", 0.75, 0.5, M)) as v:
        p = B.mandelbrot_params(W, H, supersample=s, adaptive=True, **kw)
        q, plane = sample_plane(ctx, B, p)
        assert q.flags & B.MANDEL_PERTURB_FORCE_DEEP
        assert np.array_equal(plane, R.plane(v.o.table(), v.o.length, s * W, s * H, M, v.o.scale))
        want, mask = A.image(plane, s, M, B.colour_lut(M))
        assert 0 < mask.sum() < W * H
        rgba, _ = ctx.mandelbrot(p, want_iters=False)
        same(rgba, want, s)
        assert ctx.last_refined() == (int(mask.sum()), W * H)


def test_all_interior_view_launches_nothing(ctx, B):
    """-0.1 + 0.2 i at 1e-200 lies inside the main cardioid: every anchor is M, the list is empty, the image is the plain image."""
    W, H, M = 53, 31, 400
    with B.Orbit("-0.1", "0.2", 1e-200, 1e-200, M) as o:
        ctx.bind_mandelbrot_orbit(o)
        try:
            kw = dict(max_iter=M, precision=B.PRECISION_PERTURB, **ZERO)
            plain, it = ctx.mandelbrot(B.mandelbrot_params(W, H, **kw))
            assert (it == M).all()
            for s in S.FACTORS:
                for extra in (0, B.MANDEL_COLOUR_EQUALISED):
                    p = B.mandelbrot_params(W, H, supersample=s, adaptive=True, flags=extra, **kw)
                    rgba, _ = ctx.mandelbrot(p, want_iters=False)
                    same(rgba, plain, (s, extra))
                    assert ctx.last_refined() == (0, W * H)
                    assert np.array_equal(ctx.mandelbrot_rgba8(p), S.rgba8(plain))
        finally:
            ctx.bind_mandelbrot_orbit(None)
    flat = B.mandelbrot_params(W, H, max_iter=50, centre=(0.0, 0.0), scale=(0.01, 0.01), supersample=2, adaptive=True)   # f32, inside
    rgba, _ = ctx.mandelbrot(flat, want_iters=False)
    assert ctx.last_refined() == (0, W * H) and (bits(rgba) == bits(B.colour_lut(50)[50])).all()


def test_counts_beyond_uint16(ctx, B):
    """max_iter > 65535: the anchor plane is uint32_t."""
    M, W, H, s = 70000, 64, 40, 2
    kw = dict(max_iter=M, precision=B.PRECISION_F32, centre=(-0.75, 0.05), scale=(0.3, 0.2))
    lut = B.colour_lut(M)
    for extra in (0, B.MANDEL_COLOUR_EQUALISED):
        p = B.mandelbrot_params(W, H, supersample=s, adaptive=True, flags=extra, **kw)
        _, plane = sample_plane(ctx, B, p)
        assert A.anchor_plane(plane, s).max() > 65535
        want, mask = A.image(plane, s, M, lut, equalised=bool(extra))
        rgba, _ = ctx.mandelbrot(p, want_iters=False)
        same(rgba, want, extra)
        assert ctx.last_refined() == (int(mask.sum()), W * H) and 0 < mask.sum() < W * H


def test_two_calls_give_identical_bytes(ctx, B):
    """The list's order varies from run to run; the image does not."""
    W, H, M = 640, 400, 300
    p = B.mandelbrot_params(W, H, max_iter=M, supersample=4, adaptive=True)
    a, _ = ctx.mandelbrot(p, want_iters=False)
    ra = ctx.last_refined()
    a8 = ctx.mandelbrot_rgba8(p)
    for _ in range(3):
        b, _ = ctx.mandelbrot(p, want_iters=False)
        assert np.array_equal(bits(a), bits(b)) and ctx.last_refined() == ra
        assert np.array_equal(ctx.mandelbrot_rgba8(p), a8)
    _, plane = sample_plane(ctx, B, p)
    want, mask = A.image(plane, 4, M, B.colour_lut(M))
    same(a, want)
    assert ra == (int(mask.sum()), W * H)
    # views alternate on one context: neither cached table serves the other call
    other = B.mandelbrot_params(W, H, max_iter=M, centre=(-0.75, 0.1), scale=(0.5, 0.3), supersample=2, adaptive=True)
    o1, _ = ctx.mandelbrot(other, want_iters=False)
    plain, it = ctx.mandelbrot(B.mandelbrot_params(W, H, max_iter=M))
    same(plain, B.colour_lut(M)[it])
    b, _ = ctx.mandelbrot(p, want_iters=False)
    assert np.array_equal(bits(a), bits(b))
    o2, _ = ctx.mandelbrot(other, want_iters=False)
    assert np.array_equal(bits(o1), bits(o2))
    _, plane = sample_plane(ctx, B, other)
    same(o1, A.image(plane, 2, M, B.colour_lut(M))[0])


def test_last_refined_before_the_first_adaptive_render(B):
    with B.Context(0) as c2:
        with pytest.raises(B.McError) as e:
            c2.last_refined()
        assert e.value.status == INVALID
        c2.mandelbrot(B.mandelbrot_params(64, 40, supersample=2), want_iters=False)        # full supersampling is no adaptive call
        with pytest.raises(B.McError):
            c2.last_refined()
        c2.mandelbrot(B.mandelbrot_params(64, 40, supersample=2, adaptive=True), want_iters=False)
        r, n = c2.last_refined()
        assert 0 < r < n == 64 * 40
        L = B.lib()
        one = C.c_uint64(0)
        assert L.mc_context_last_refined(c2._h, None, None) == 0
        assert L.mc_context_last_refined(c2._h, C.byref(one), None) == 0 and one.value == r
        assert L.mc_context_last_refined(c2._h, None, C.byref(one)) == 0 and one.value == n


def test_warmup_accepts_the_bit(B):
    L = B.lib()
    L.mc_context_warmup_mandelbrot.argtypes = [C.c_void_p, C.POINTER(B.MandelbrotParams), C.c_int]
    W, H, M = 64, 40, 300
    with B.Context(0) as c2:
        for s in S.FACTORS:
            for extra in (0, B.MANDEL_COLOUR_EQUALISED):
                p = B.mandelbrot_params(W, H, max_iter=M, supersample=s, adaptive=True, flags=extra)
                for how in (0, 1, 3):
                    assert L.mc_context_warmup_mandelbrot(c2._h, C.byref(p), how) == 0
                _, plane = sample_plane(c2, B, p)
                rgba, _ = c2.mandelbrot(p, want_iters=False)
                same(rgba, A.image(plane, s, M, B.colour_lut(M), equalised=bool(extra))[0], (s, extra))
        alone = B.mandelbrot_params(W, H, max_iter=M, adaptive=True)
        assert L.mc_context_warmup_mandelbrot(c2._h, C.byref(alone), 0) == INVALID


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, B):
    import torch
    W, H, M, s = 64, 48, 200, 2
    d_rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    d_it = torch.zeros((H * s, W * s), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def refused(call, words, status=INVALID):
        with pytest.raises(B.McError) as e:
            call()
        assert e.value.status == status, e.value
        for w in words:
            assert w in str(e.value), e.value
        rgba, it = ctx.mandelbrot(B.mandelbrot_params(W, H, max_iter=M))          # the context stays usable
        same(rgba, B.colour_lut(M)[it])

    only = ("MC_MANDEL_SUPERSAMPLE_ADAPTIVE is valid only together with MC_MANDEL_SUPERSAMPLE",)
    for f in (0, 1):   # the bit without s >= 2
        alone = B.mandelbrot_params(W, H, max_iter=M, supersample=f, adaptive=True)
        refused(lambda: ctx.mandelbrot(alone, want_iters=False), only)
        refused(lambda: ctx.mandelbrot(alone), only)
        refused(lambda: ctx.mandelbrot_rgba8(alone), only)
        refused(lambda: ctx.mandelbrot_device(alone, d_rgba.data_ptr(), d_it.data_ptr()), only)
        refused(lambda: ctx.mandelbrot_banded(alone, 16), only)
        refused(lambda: ctx.mandelbrot_assemble_device(alone, d_it.data_ptr(), 4, 1, 8, H, d_rgba.data_ptr()), only)
        with B.Multi(1) as mm:
            refused(lambda: mm.mandelbrot(alone), ("MC_MANDEL_SUPERSAMPLE_ADAPTIVE",), UNSUPPORTED)
    ad = B.mandelbrot_params(W, H, max_iter=M, supersample=s, adaptive=True)
    # tiles and bands
    whole = ("MC_MANDEL_SUPERSAMPLE_ADAPTIVE needs the whole image", "cannot see its neighbours")
    for kw in (dict(row_begin=8), dict(row_end=H - 1), dict(row_begin=8, row_block=8, row_stride=16)):
        tile = B.mandelbrot_params(W, H, max_iter=M, supersample=s, adaptive=True, **kw)
        refused(lambda: ctx.mandelbrot(tile, want_iters=False), whole)
        refused(lambda: ctx.mandelbrot_rgba8(tile), whole)
    # out_iters, the full-plane resolve, the calls that refuse every s >= 2
    refused(lambda: ctx.mandelbrot(ad), ("out_iters must be NULL",))
    refused(lambda: ctx.mandelbrot_resolve_device(ad, d_it.data_ptr(), 4, None, d_rgba.data_ptr()), ("MC_MANDEL_SUPERSAMPLE_ADAPTIVE", "FULL sample plane"))
    names = ("mc_mandelbrot_supersample_params", "mc_mandelbrot_resolve_device_async")
    refused(lambda: ctx.mandelbrot_device(ad, d_rgba.data_ptr(), d_it.data_ptr()), names)
    refused(lambda: ctx.mandelbrot_banded(ad, 16), names)
    refused(lambda: ctx.mandelbrot_assemble_device(ad, d_it.data_ptr(), 4, 1, 8, H, d_rgba.data_ptr()), names)
    with B.Multi(1) as mm:
        refused(lambda: mm.mandelbrot(ad), (), UNSUPPORTED)
        refused(lambda: mm.mandelbrot_rgba8(ad), (), UNSUPPORTED)
    for bad in (3, 5, 15):
        pb = B.mandelbrot_params(W, H, max_iter=M, supersample=bad, adaptive=True)
        refused(lambda: ctx.mandelbrot(pb, want_iters=False), (f"MC_MANDEL_SUPERSAMPLE({bad})",))
        refused(lambda: ctx.mandelbrot_rgba8(pb), (f"MC_MANDEL_SUPERSAMPLE({bad})",))
    # and the adaptive render still works
    _, plane = sample_plane(ctx, B, ad)
    rgba, _ = ctx.mandelbrot(ad, want_iters=False)
    same(rgba, A.image(plane, s, M, B.colour_lut(M))[0])


# ---- the app --------------------------------------------------------------------------------------------------------------------
def test_app_end_to_end(ctx, B, tmp_path):
    W, H, M, s = 160, 96, 300, 2
    size = ["--width", str(W), "--height", str(H), "--max-iter", str(M)]
    lut = B.colour_lut(M)
    p = B.mandelbrot_params(W, H, max_iter=M, supersample=s, adaptive=True)
    _, plane = sample_plane(ctx, B, p)
    want, mask = A.image(plane, s, M, lut)
    want_eq, _ = A.image(plane, s, M, lut, equalised=True)
    assert np.array_equal(ctx.mandelbrot_rgba8(p), S.rgba8(want))
    line = f"refined {int(mask.sum())} of {W * H} pixels"
    for extra in ([], ["--gpu-postprocess"], ["--streamed-save"], ["--gpu-postprocess", "--streamed-save"]):
        img, text = run_app(tmp_path, "ad.png", "--supersample", "2", "--adaptive", *size, *extra)
        assert np.array_equal(img, S.rgba8(want)), extra
        assert line in text, text
        assert ("--streamed-save has no effect" in text) == ("--streamed-save" in extra)
        img, text = run_app(tmp_path, "ad_eq.png", "--adaptive", "--supersample", "2", "--colour", "equalised", *size, *extra)
        assert np.array_equal(img, S.rgba8(want_eq)), extra
        assert line in text
    _, text = run_app(tmp_path, "full.png", "--supersample", "2", *size)
    assert "refined" not in text
