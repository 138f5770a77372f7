"""MC_MANDEL_COLOUR_SMOOTH_EQUALISED on the MI355X: the histogram stage on uploaded synthetic smooth planes against
tests/mandel_smooth_equalise_ref.py bit for bit (tiny sizes, unaligned heads and tails, one range, three ranges, the global-table route,
accumulation, repeatability), the remap stage (both outputs, each alone, contiguous and interleaved tiles, guard words, a replaced table),
the whole chain in every precision against the restatement and against the chain made by hand, degenerate views, a zoom frame, every
refusal, the warm-up, the app."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mandel_f64_ref as F
import mandel_smooth_equalise_ref as Q
import mandel_smooth_ref as S
from test_gpu_mandel_distance import chain_views
from test_gpu_mandel_equalise import bound_view

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "mandelbrot")
INVALID, UNSUPPORTED = 1, 5
FLAG = "MC_MANDEL_COLOUR_SMOOTH_EQUALISED"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def sparams(B, w, h, flags=0, **kw):
    return B.mandelbrot_params(w, h, flags=B.MANDEL_COLOUR_SMOOTH_EQUALISED | flags, **kw)


def upload(q, offset=0):
    """The values of q on the device, starting `offset` uint32 past a 256-byte aligned allocation: (tensor kept alive, device pointer)."""
    import torch
    flat = np.ascontiguousarray(q, np.uint32).reshape(-1)
    buf = torch.zeros(flat.size + offset, dtype=torch.int32, device="cuda")
    buf[offset:] = torch.from_numpy(flat.view(np.int32)).cuda()
    return buf, buf.data_ptr() + 4 * offset


def device_hist(ctx, B, q, M, offset=0, into=None):
    """mc_mandelbrot_smooth_histogram_device_async over the uploaded values, added into a zeroed table (or `into`) between two guard words."""
    import torch
    buf, ptr = upload(q, offset)
    tab = into if into is not None else torch.zeros(M + 3, dtype=torch.int32, device="cuda")
    if into is None:
        tab[0] = tab[M + 2] = -7
    torch.cuda.synchronize()
    ctx.mandelbrot_smooth_histogram_device(ptr, int(np.asarray(q).size), M, tab.data_ptr() + 4)
    ctx.synchronize()
    host = tab.cpu().numpy()
    assert host[0] == -7 and host[M + 2] == -7, "a write outside the table"
    return host[1:M + 2].view(np.uint32).copy(), tab


def check_hist(ctx, B, q, M, what, offset=0):
    got, _ = device_hist(ctx, B, q, M, offset)
    want = Q.histogram(q, M)
    assert np.array_equal(got, want), (what, int((got != want).sum()), np.flatnonzero(got != want)[:4])
    return got


# ---- the histogram stage ---------------------------------------------------------------------------------------------------------
def test_histogram_of_tiny_planes_and_offsets(ctx, B):
    M = 200
    rng = np.random.default_rng(11)
    for size in range(1, 21):
        q = rng.integers(0, 256 * M + 300, size).astype(np.uint32)
        for offset in range(4):                                          # the unaligned head and tail
            check_hist(ctx, B, q, M, (size, offset), offset)


@pytest.mark.parametrize("M", [200, 40000], ids=["one-range", "three-ranges"])
@pytest.mark.parametrize("W,H", [(203, 131), (260, 9)], ids=["203x131", "260x9"])
def test_histogram_is_the_restatement(ctx, B, W, H, M):
    for name, q in Q.synthetic_planes(W, H, M):
        for offset in (0, 1, 2, 3) if name in ("random", "skewed") else (0,):
            check_hist(ctx, B, q, M, (name, W, H, M, offset), offset)


def test_histogram_scalar_restatement_agrees():
    for name, q in Q.synthetic_planes(67, 35, 200):
        assert np.array_equal(Q.histogram(q, 200), Q.histogram_scalar(q, 200)), name


def test_histogram_by_the_global_table_route(ctx, B):
    M = 1 << 20                                                          # 65 ranges: above kHistMaxRanges
    for name, q in Q.synthetic_planes(67, 35, M):
        check_hist(ctx, B, q, M, (name, M))
    check_hist(ctx, B, Q.synthetic_planes(67, 35, M)[0][1], M, ("random, offset", M), offset=3)


def test_histogram_accumulates_and_repeats(ctx, B):
    M = 40000
    planes = dict(Q.synthetic_planes(203, 131, M))
    a, b = planes["random"], planes["skewed"]
    first, tab = device_hist(ctx, B, a, M)
    both, _ = device_hist(ctx, B, b, M, offset=1, into=tab)              # a second call adds into the same table
    assert np.array_equal(both, Q.histogram(np.concatenate((a.ravel(), b.ravel())), M))
    again, _ = device_hist(ctx, B, a, M)
    assert np.array_equal(first, again)                                  # two runs, one table


# ---- the remap stage ---------------------------------------------------------------------------------------------------------------
def stage(ctx, B, q, qmap, M, tile=None, want_ranked=True, want_rgba=True, offset=0):
    """mc_mandelbrot_smooth_remap_device_async on the uploaded compact tile q (rows x W): (q', rgba), None where not wanted.  Each output
    lies between two guard rows, which must come back untouched."""
    import torch
    rows, W = q.shape
    buf, ptr = upload(q, offset)
    d_r = torch.full((rows + 2, W), -7, dtype=torch.int32, device="cuda")
    d_rgba = torch.full((rows + 2, W, 4), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    p = sparams(B, W, tile["height"] if tile else rows, max_iter=M, **({k: v for k, v in tile.items() if k != "height"} if tile else {}))
    assert B.tile_rows(p) == rows
    ctx.mandelbrot_smooth_remap_device(p, ptr, qmap, d_r[1:].data_ptr() if want_ranked else 0, d_rgba[1:].data_ptr() if want_rgba else 0)
    ctx.synchronize()
    r, rgba = d_r.cpu().numpy(), d_rgba.cpu().numpy()
    for a in (r, rgba):
        assert (a[0] == -7).all() and (a[-1] == -7).all(), "a write outside the tile"
    if not want_ranked:
        assert (r == -7).all()
    if not want_rgba:
        assert (rgba == -7.0).all()
    return (r[1:-1].view(np.uint32) if want_ranked else None), (rgba[1:-1] if want_rgba else None)


def check_stage(ctx, B, q, qmap, M, lut, what, **kw):
    r, rgba = stage(ctx, B, q, qmap, M, **kw)
    want = Q.remap(np.minimum(q, 256 * M), qmap, M)                      # (a q above 256 M on the device is taken as interior)
    if r is not None:
        assert np.array_equal(r, want), (what, "q'", int((r != want).sum()))
    if rgba is not None:
        bad = (bits(rgba) != bits(S.colour(want, M, lut))).any(axis=-1)
        assert not bad.any(), (what, "rgba", int(bad.sum()))


@pytest.mark.parametrize("M", [200, 40000], ids=["M200", "M40000"])
@pytest.mark.parametrize("W,H", [(203, 131), (260, 9)], ids=["203x131", "260x9"])
def test_remap_is_the_restatement(ctx, B, W, H, M):
    lut = B.colour_lut(M)
    planes = Q.synthetic_planes(W, H, M)
    for name, q in planes:
        qmap = Q.knot_map(Q.histogram(q, M), M)
        assert np.array_equal(qmap, B.smooth_equalise_map(M, Q.histogram(q, M)))
        check_stage(ctx, B, q, qmap, M, lut, (name, W, H, M))            # every call replaces the cached table with another map
    q = dict(planes)["skewed"]
    qmap = Q.knot_map(Q.histogram(q, M), M)
    check_stage(ctx, B, q, qmap, M, lut, "q' only", want_rgba=False)
    check_stage(ctx, B, q, qmap, M, lut, "rgba only", want_ranked=False)
    check_stage(ctx, B, q, qmap, M, lut, "offset input", offset=1)
    other = Q.knot_map(Q.histogram(dict(planes)["random"], M), M)        # the same plane under a different map, then the first again
    assert not np.array_equal(other, qmap)
    check_stage(ctx, B, q, other, M, lut, "a second map")
    check_stage(ctx, B, q, qmap, M, lut, "the first map again")


def test_remap_of_tiles_and_tiny_planes(ctx, B):
    M = 200
    lut = B.colour_lut(M)
    rng = np.random.default_rng(3)
    qmap = Q.knot_map(rng.integers(0, 1000, M + 1).astype(np.uint32), M)
    for size in range(1, 21):
        q = rng.integers(0, 256 * M + 1, (1, size)).astype(np.uint32)
        check_stage(ctx, B, q, qmap, M, lut, ("tiny", size))
    W, H = 67, 40
    band = dict(height=H, row_begin=8, row_end=29)                        # a contiguous band: 21 rows, stored compactly
    q = rng.integers(0, 256 * M + 1, (21, W)).astype(np.uint32)
    check_stage(ctx, B, q, qmap, M, lut, "band", tile=band)
    inter = dict(height=H, row_begin=8, row_end=H, row_block=8, row_stride=16)   # rows 8..15, 24..31: 16 rows, stored compactly
    q = rng.integers(0, 256 * M + 1, (16, W)).astype(np.uint32)
    check_stage(ctx, B, q, qmap, M, lut, "interleaved", tile=inter)


# ---- the chain ------------------------------------------------------------------------------------------------------------------------
def by_hand(ctx, B, p_flag, q, M):
    """The three public calls on the uploaded q plane: (q', rgba)."""
    import torch
    H, W = q.shape
    buf, ptr = upload(q)
    tab = torch.zeros(M + 1, dtype=torch.int32, device="cuda")
    d_r = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    d_rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.mandelbrot_smooth_histogram_device(ptr, W * H, M, tab.data_ptr())
    ctx.synchronize()
    qmap = B.smooth_equalise_map(M, tab.cpu().numpy().view(np.uint32))
    ctx.mandelbrot_smooth_remap_device(p_flag, ptr, qmap, d_r.data_ptr(), d_rgba.data_ptr())
    ctx.synchronize()
    return d_r.cpu().numpy().view(np.uint32), d_rgba.cpu().numpy()


@pytest.mark.parametrize("which", range(7), ids=["f32", "ds", "f64", "perturb", "perturb-bla", "deep-orbit", "perturb-bla-deep"])
def test_chain_in_every_precision(ctx, B, O, which):
    name, kw, make, _ = chain_views(B)[which]
    W, H = 203, 131
    Mv = kw["max_iter"]
    lut = B.colour_lut(Mv)
    with bound_view(B, ctx, kw, make):
        _, n, q = ctx.mandelbrot_smooth(B.mandelbrot_params(W, H, flags=B.MANDEL_COLOUR_SMOOTH, **kw), want_rgba=False)
        p = sparams(B, W, H, **kw)
        rgba, n2, q2, r = ctx.mandelbrot_smooth_equalised(p)
        assert np.array_equal(n2, n) and np.array_equal(q2, q), name
        want_r = Q.ranked(q, Mv)
        want = S.colour(want_r, Mv, lut)
        assert np.array_equal(r, want_r), (name, int((r != want_r).sum()))
        assert np.array_equal(bits(rgba), bits(want)), name
        assert (r[q < 256 * Mv] < 256 * Mv).all() and (r[q == 256 * Mv] == 256 * Mv).all()
        assert len(np.unique(r)) > 10, name
        rgba1, n1 = ctx.mandelbrot(p)
        assert np.array_equal(bits(rgba1), bits(want)) and np.array_equal(n1, n), name
        u8 = ctx.mandelbrot_rgba8(p)
        assert np.array_equal(u8, ctx.convert_rgba8(want, 255.0)), name
        hand_r, hand_rgba = by_hand(ctx, B, p, q, Mv)
        assert np.array_equal(hand_r, r) and np.array_equal(bits(hand_rgba), bits(rgba)), name
        again = ctx.mandelbrot_smooth_equalised(p)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(again, (rgba, n2, q2, r))), name
        only = ctx.mandelbrot_smooth_equalised(p, want_rgba=False, want_iters=False, want_smooth=False)
        assert only[:3] == (None, None, None) and np.array_equal(only[3], want_r)
        only = ctx.mandelbrot_smooth_equalised(p, want_iters=False, want_smooth=False, want_ranked=False)
        assert only[1:] == (None, None, None) and np.array_equal(bits(only[0]), bits(want))
        kms, cms = ctx.last_timing()
        assert kms > 0 and cms >= 0
    if name in ("f32", "f64"):                                           # the whole plane restated: equal end to end
        st = S.f32_capture(W, H, Mv) if name == "f32" else S.f64_plane_capture(F, W, H, Mv, kw.get("centre", (-0.445, 0.0)),
                                                                                 kw.get("scale", (2.34, 2.34)))
        q_ref = S.smooth_count(O, st[0], Mv, *st[1:])
        assert np.array_equal(st[0], n) and np.array_equal(q_ref, q), name
        assert np.array_equal(Q.ranked(q_ref, Mv), r) and np.array_equal(bits(Q.colour(q_ref, Mv, lut)), bits(rgba)), name


def test_chain_on_degenerate_views(ctx, B):
    Mv = 128
    lut = B.colour_lut(Mv)
    p = sparams(B, 40, 24, max_iter=Mv, centre=(0.0, 0.0), scale=(0.1, 0.1))           # all interior: E = 0
    rgba, n, q, r = ctx.mandelbrot_smooth_equalised(p)
    assert (n == Mv).all() and (q == 256 * Mv).all() and (r == 256 * Mv).all()
    assert np.array_equal(bits(rgba), bits(np.broadcast_to(lut[Mv], rgba.shape)))
    assert np.array_equal(ctx.mandelbrot_rgba8(p), ctx.convert_rgba8(rgba, 255.0))
    p = sparams(B, 40, 24, max_iter=Mv, centre=(2.0, 2.0), scale=(0.1, 0.1))           # every pixel escapes at once
    rgba, n, q, r = ctx.mandelbrot_smooth_equalised(p)
    assert (n == 0).all() and (q < 256 * Mv).all()
    assert np.array_equal(r, Q.ranked(q, Mv)) and np.array_equal(bits(rgba), bits(Q.colour(q, Mv, lut))) and (r < 256 * Mv).all()
    p = sparams(B, 1, 1, max_iter=Mv)                                                   # one pixel
    rgba, n, q, r = ctx.mandelbrot_smooth_equalised(p)
    assert rgba.shape == (1, 1, 4) and np.array_equal(r, Q.ranked(q, Mv)) and np.array_equal(bits(rgba), bits(Q.colour(q, Mv, lut)))
    assert np.array_equal(bits(ctx.mandelbrot(p)[0]), bits(rgba))


def test_zoom_frame_is_the_plain_call(ctx, B):
    W, H, Mv = 67, 35, 128
    p = sparams(B, W, H, max_iter=Mv)
    want, _ = ctx.mandelbrot(p)
    with ctx.zoom(W, H) as z:
        z.push(p)
        rgba, u8 = z.frame(1.0, want_rgba=True, want_rgba8=True)
    assert np.array_equal(bits(rgba), bits(want))
    assert np.array_equal(u8, ctx.mandelbrot_rgba8(p))


# ---- refusals, the warm-up ------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, B):
    import torch
    w, h, Mv = 64, 48, 200
    d_rgba = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    d_it = torch.zeros((4 * h, 4 * w), dtype=torch.int32, device="cuda")
    d_D = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    L = B.lib()
    L.mc_context_warmup_mandelbrot.argtypes = [C.c_void_p, C.POINTER(B.MandelbrotParams), C.c_int]

    def refused(call, status=INVALID, says=FLAG):
        with pytest.raises(B.McError) as e:
            call()
        assert e.value.status == status, e.value
        if says:
            assert says in str(e.value), e.value

    p = sparams(B, w, h, max_iter=Mv)
    ident = np.arange(Mv + 1, dtype=np.uint32)
    knots = 256 * ident
    # a row tile, band or interleave of the two calls that honour the flag, and of the four-plane call
    for tile in (dict(row_begin=0, row_end=8), dict(row_begin=8, row_end=h), dict(row_begin=0, row_end=h, row_block=8, row_stride=16)):
        t = sparams(B, w, h, max_iter=Mv, **tile)
        for call in (lambda: ctx.mandelbrot(t), lambda: ctx.mandelbrot_rgba8(t), lambda: ctx.mandelbrot_smooth_equalised(t)):
            refused(call)
            refused(call, says="mc_mandelbrot_smooth_remap_device_async")   # the by-hand calls are named
    # the calls that never take the flag
    never = [lambda: ctx.mandelbrot_device(p, d_rgba.data_ptr(), d_it.data_ptr()),
             lambda: ctx.mandelbrot_banded(p, 16), lambda: ctx.mandelbrot_banded(p, 16, rgba8=True),
             lambda: ctx.mandelbrot_smooth(p), lambda: ctx.mandelbrot_smooth_device(p, d_rgba.data_ptr(), d_it.data_ptr(), 0),
             lambda: ctx.mandelbrot_distance(p), lambda: ctx.mandelbrot_distance_device(p, d_it.data_ptr(), 1.0, d_D.data_ptr(), 0),
             lambda: ctx.mandelbrot_recolour_device(p, d_it.data_ptr(), 4, ident, d_rgba.data_ptr()),
             lambda: ctx.mandelbrot_resolve_device(sparams(B, w, h, max_iter=Mv, supersample=2), d_it.data_ptr(), 4, None, d_rgba.data_ptr()),
             lambda: ctx.mandelbrot_assemble_device(p, d_it.data_ptr(), 4, 1, 8, h, d_rgba.data_ptr())]
    for call in never:
        refused(call)
        refused(call, says="mc_mandelbrot_smooth_histogram_device_async")
    with B.Multi(1) as mm:
        refused(lambda: mm.mandelbrot(p), UNSUPPORTED)
        refused(lambda: mm.mandelbrot_rgba8(p), UNSUPPORTED)
    # the flag together with another colouring, a resolve or the contraction switch
    combos = [(dict(flags=B.MANDEL_COLOUR_SMOOTH), "MC_MANDEL_COLOUR_SMOOTH "),
              (dict(flags=B.MANDEL_COLOUR_EQUALISED), "MC_MANDEL_COLOUR_EQUALISED"),
              (dict(flags=B.MANDEL_COLOUR_DISTANCE), "MC_MANDEL_COLOUR_DISTANCE"),
              (dict(supersample=2), "MC_MANDEL_SUPERSAMPLE"),
              (dict(supersample=8), "MC_MANDEL_SUPERSAMPLE"),
              (dict(supersample=4, adaptive=True), "MC_MANDEL_SUPERSAMPLE_ADAPTIVE"),
              (dict(adaptive=True), "MC_MANDEL_SUPERSAMPLE_ADAPTIVE"),
              (dict(flags=B.MANDEL_FMA), "MC_MANDEL_FMA")]
    for extra, word in combos:
        flags = extra.pop("flags", 0)
        c = sparams(B, w, h, flags=flags, max_iter=Mv, **extra)
        for call in (lambda: ctx.mandelbrot(c), lambda: ctx.mandelbrot(c, want_iters=False), lambda: ctx.mandelbrot_rgba8(c),
                     lambda: ctx.mandelbrot_smooth_equalised(c),
                     lambda: ctx.mandelbrot_smooth_remap_device(c, d_it.data_ptr(), knots, d_it.data_ptr() + 4 * w * h, d_rgba.data_ptr())):
            refused(call)
            refused(call, says=word)
        assert L.mc_context_warmup_mandelbrot(ctx._h, C.byref(c), 1) == INVALID
        assert FLAG in L.mc_last_error_detail().decode()
    # MC_MANDEL_COLOUR_SMOOTH | MC_MANDEL_COLOUR_EQUALISED without the new flag stays refused and names the integer flag
    old = B.mandelbrot_params(w, h, max_iter=Mv, flags=B.MANDEL_COLOUR_SMOOTH | B.MANDEL_COLOUR_EQUALISED)
    refused(lambda: ctx.mandelbrot(old), says="MC_MANDEL_COLOUR_EQUALISED")
    # the new calls' own rules
    plain = B.mandelbrot_params(w, h, max_iter=Mv)
    refused(lambda: ctx.mandelbrot_smooth_equalised(plain), says="must carry " + FLAG)
    refused(lambda: ctx.mandelbrot_smooth_remap_device(plain, d_it.data_ptr(), knots, 0, d_rgba.data_ptr()), says="must carry " + FLAG)
    refused(lambda: ctx.mandelbrot_smooth_equalised(p, want_rgba=False, want_iters=False, want_smooth=False, want_ranked=False), says=None)
    refused(lambda: ctx.mandelbrot_smooth_remap_device(p, d_it.data_ptr(), knots, 0, 0), says=None)
    refused(lambda: ctx.mandelbrot_smooth_remap_device(p, 0, knots, 0, d_rgba.data_ptr()), says=None)
    refused(lambda: ctx.mandelbrot_smooth_remap_device(p, d_it.data_ptr() + 2, knots, 0, d_rgba.data_ptr()), says=None)
    refused(lambda: ctx.mandelbrot_smooth_remap_device(p, d_it.data_ptr(), knots, d_it.data_ptr() + 2, 0), says=None)
    refused(lambda: ctx.mandelbrot_smooth_remap_device(p, d_it.data_ptr(), knots, 0, d_rgba.data_ptr() + 4), says=None)
    bad = knots.copy()
    bad[5] = bad[6] + 1
    refused(lambda: ctx.mandelbrot_smooth_remap_device(p, d_it.data_ptr(), bad, 0, d_rgba.data_ptr()), says="decrease")
    bad = knots.copy()
    bad[Mv] -= 1
    refused(lambda: ctx.mandelbrot_smooth_remap_device(p, d_it.data_ptr(), bad, 0, d_rgba.data_ptr()), says="qmap[max_iter]")
    bad = knots.copy()
    bad[Mv - 1] = 256 * Mv + 1
    refused(lambda: ctx.mandelbrot_smooth_remap_device(p, d_it.data_ptr(), bad, 0, d_rgba.data_ptr()), says="above 256 * max_iter")
    refused(lambda: ctx.mandelbrot_smooth_histogram_device(d_it.data_ptr(), 2 ** 32, Mv, d_it.data_ptr()), says="2^32")
    refused(lambda: ctx.mandelbrot_smooth_histogram_device(d_it.data_ptr(), 64, S.MAX_ITER_LIMIT + 1, d_it.data_ptr()), says="2^24 - 1")
    refused(lambda: ctx.mandelbrot_smooth_histogram_device(d_it.data_ptr() + 2, 64, Mv, d_it.data_ptr()), says=None)
    refused(lambda: ctx.mandelbrot(sparams(B, w, h, flags=B.MANDEL_ITERS_U16, max_iter=Mv)))
    big = sparams(B, 8, 8, max_iter=S.MAX_ITER_LIMIT + 1, centre=(2.0, 2.0), scale=(0.1, 0.1))
    for call in (lambda: ctx.mandelbrot(big), lambda: ctx.mandelbrot_rgba8(big), lambda: ctx.mandelbrot_smooth_equalised(big)):
        refused(call, says="2^24 - 1")
    assert B.supersample_params(sparams(B, w, h, max_iter=Mv, supersample=2)).flags & B.MANDEL_COLOUR_SMOOTH_EQUALISED
    # after all that the context still renders plain, smooth and smooth equalised images
    lut = B.colour_lut(Mv)
    rgba, n = ctx.mandelbrot(plain)
    assert np.array_equal(bits(rgba), bits(lut[n]))
    srgba, n2, q = ctx.mandelbrot_smooth(B.mandelbrot_params(w, h, max_iter=Mv, flags=B.MANDEL_COLOUR_SMOOTH))
    assert np.array_equal(n2, n) and np.array_equal(bits(srgba), bits(S.colour(q, Mv, lut)))
    ergba, n3, q3, r = ctx.mandelbrot_smooth_equalised(p)
    assert np.array_equal(n3, n) and np.array_equal(q3, q) and np.array_equal(r, Q.ranked(q, Mv))
    assert np.array_equal(bits(ergba), bits(Q.colour(q, Mv, lut)))


def test_render_after_a_warm_up_with_the_flag(B):
    L = B.lib()
    L.mc_context_warmup_mandelbrot.argtypes = [C.c_void_p, C.POINTER(B.MandelbrotParams), C.c_int]
    W, H, Mv = 67, 35, 128
    with B.Context(0) as c2:
        p = sparams(B, W, H, max_iter=Mv)
        for how in (0, 1, 2, 3):
            assert L.mc_context_warmup_mandelbrot(c2._h, C.byref(p), how) == 0
        a = c2.mandelbrot_smooth_equalised(p)
        u8 = c2.mandelbrot_rgba8(p)
        p64 = sparams(B, 40, 24, max_iter=Mv, precision=B.PRECISION_F64)
        assert L.mc_context_warmup_mandelbrot(c2._h, C.byref(p64), 1) == 0
        a64 = c2.mandelbrot_smooth_equalised(p64)
    with B.Context(0) as c3:                                            # the same renders on a context never warmed up
        b = c3.mandelbrot_smooth_equalised(p)
        b64 = c3.mandelbrot_smooth_equalised(p64)
        assert np.array_equal(c3.mandelbrot_rgba8(p), u8)
    for x, y in zip(a + a64, b + b64):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert np.array_equal(a[3], Q.ranked(a[2], Mv))


# ---- the app --------------------------------------------------------------------------------------------------------------------------------
def test_app_colour_smooth_equalised(ctx, B, tmp_path):
    from PIL import Image
    w, h, Mv = 64, 48, 300
    p = sparams(B, w, h, max_iter=Mv)
    want = ctx.mandelbrot_rgba8(p)
    q = ctx.mandelbrot_smooth_equalised(p, want_rgba=False, want_iters=False, want_ranked=False)[2]
    assert not np.array_equal(want, ctx.mandelbrot_rgba8(B.mandelbrot_params(w, h, max_iter=Mv, flags=B.MANDEL_COLOUR_SMOOTH)))
    esc = q < 256 * Mv
    line = f"smooth equalised: {int(esc.sum())} of {w * h} pixels escaped, {np.unique(q[esc] >> 8).size} of {Mv} bins occupied"
    for extra in (["--gpu-postprocess"], []):
        out = tmp_path / "smooth_equalised.png"
        r = subprocess.run([APP, "--out", str(out), "--quiet", "--colour", "smooth-equalised", "--width", str(w), "--height", str(h),
                            "--max-iter", str(Mv)] + extra, capture_output=True, text=True, cwd=tmp_path, timeout=180)
        assert r.returncode == 0, r.stdout + r.stderr
        assert np.array_equal(np.asarray(Image.open(out).convert("RGBA")), want), extra
        assert line in r.stdout, r.stdout
