"""MC_MANDEL_COLOUR_SMOOTH on the MI355X: the n, q and colour planes of all seven smooth kernels against tests/mandel_smooth_ref.py bit for
bit (whole planes for F32, DS, F64 and PERTURB; sampled pixels for the BLA and deep loops, plus the identities that tie those kernels'
capture to PERTURB's), the places where the capture can go wrong (first block, tail loop, replayed fast block, tiny images), every route
to the same bytes, every refusal, the app."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import mandel_f64_ref as F
import mandel_perturb_deep_ref as D
import mandel_perturb_ref as R
import mandel_smooth_ref as S
from test_gpu_mandel_equalise import bound_view, six_views

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "mandelbrot")
K4 = R.DEEP_CENTRE
ZERO = dict(centre=(0.0, 0.0), scale=(0.0, 0.0))
W, H = 203, 131            # ragged against the 8 x 8 tile
INVALID, UNSUPPORTED = 1, 5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def smooth_params(B, w, h, flags=0, **kw):
    return B.mandelbrot_params(w, h, flags=B.MANDEL_COLOUR_SMOOTH | flags, **kw)


def check_planes(B, got, want_n, want_q, M, what):
    rgba, n, q = got
    assert np.array_equal(n, want_n), (what, "n", int((n != want_n).sum()))
    bad = q != want_q
    assert not bad.any(), (what, "q", int(bad.sum()), q[bad][:4], want_q[bad][:4])
    want = S.colour(q, M, B.colour_lut(M))
    assert np.array_equal(bits(rgba), bits(want)), (what, "rgba", int((bits(rgba) != bits(want)).any(axis=-1).sum()))


# ---- F32, DS, F64, PERTURB: whole planes ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def restated(which):
    """(n, q) of six_views()[which] at W x H from the capture variants; computed once."""
    import __graft_entry__ as entry
    O, B = entry.load_oracle(), entry.load_package().bindings
    name, kw, make = six_views(B)[which]
    M = kw["max_iter"]
    if name == "f32":
        st = S.f32_capture(W, H, M)
    elif name == "ds":
        st = S.ds_capture(O, W, H, M, O.make_view(kw["centre"][0], kw["centre"][1], kw["scale"][0], kw["scale"][1]))
    elif name == "f64":
        st = S.f64_plane_capture(F, W, H, M, kw["centre"], kw["scale"])
    else:
        with make() as o:
            st = S.perturb_plane_capture(R, o.table(), o.length, W, H, M, o.scale)
    n, zx, zy, cx, cy = st
    return n, S.smooth_count(O, n, M, zx, zy, cx, cy)


@pytest.mark.parametrize("which", range(4), ids=["f32", "ds", "f64", "perturb"])
def test_whole_plane_is_the_restatement(ctx, B, which):
    name, kw, make = six_views(B)[which]
    M = kw["max_iter"]
    want_n, want_q = restated(which)
    assert len(np.unique(want_n)) >= 10 and len(np.unique(want_q)) > len(np.unique(want_n))
    with bound_view(B, ctx, kw, make):
        got = ctx.mandelbrot_smooth(smooth_params(B, W, H, **kw))
        check_planes(B, got, want_n, want_q, M, name)
        # mc_mandelbrot_render with the flag: the same colours, out_iters still n; any subset of the three outputs
        rgba, n = ctx.mandelbrot(smooth_params(B, W, H, **kw))
        assert np.array_equal(bits(rgba), bits(got[0])) and np.array_equal(n, want_n)
        only_q = ctx.mandelbrot_smooth(smooth_params(B, W, H, **kw), want_rgba=False, want_iters=False)
        assert only_q[0] is None and only_q[1] is None and np.array_equal(only_q[2], want_q)
        # without the flag: lut[n], as ever
        plain, n = ctx.mandelbrot(B.mandelbrot_params(W, H, **kw))
        assert np.array_equal(bits(plain), bits(B.colour_lut(M)[n])) and np.array_equal(n, want_n)


# ---- the BLA and deep loops: sampled pixels ---------------------------------------------------------------------------------------------
def spanning_pixels(n, k):
    """At least k pixels (gy, gx) of the plane n: one pixel of each of up to k distinct counts, evenly spaced over the sorted distinct
    counts and ALL kept, filled up to k with pixels evenly spaced over the plane sorted by count."""
    flat = n.ravel()
    order = np.argsort(flat, kind="stable")
    firsts = order[np.concatenate([[0], np.flatnonzero(np.diff(flat[order])) + 1])]      # one pixel per distinct count
    pick = firsts[np.unique(np.linspace(0, firsts.size - 1, min(k, firsts.size)).astype(int))]
    rest = order[np.linspace(0, order.size - 1, 2 * k).astype(int)]
    fill = rest[~np.isin(rest, pick)][: max(k - pick.size, 0)]
    idx = np.concatenate([pick, fill])
    assert idx.size >= min(k, flat.size) and np.unique(idx).size == idx.size
    return [(int(i // n.shape[1]), int(i % n.shape[1])) for i in idx]


def check_sampled(B, O, got, M, scalar, what):
    rgba, n, q = got
    px = spanning_pixels(n, 48)
    counts = {int(n[p]) for p in px}
    assert len(px) >= 48 and len(counts) >= min(48, len(np.unique(n))) >= 10, what      # the sample spans the view's counts
    assert min(counts) == int(n.min()) and max(counts) == int(n.max()), what
    st = np.array([scalar(gx, gy) for gy, gx in px], np.float64)
    want_n = st[:, 0].astype(np.uint32)
    want_q = S.smooth_count(O, want_n, M, st[:, 1], st[:, 2], st[:, 3], st[:, 4])
    got_n = np.array([n[p] for p in px], np.uint32)
    got_q = np.array([q[p] for p in px], np.uint32)
    assert np.array_equal(got_n, want_n), (what, "n")
    assert np.array_equal(got_q, want_q), (what, "q", got_q[got_q != want_q][:4], want_q[got_q != want_q][:4])
    want = S.colour(q, M, B.colour_lut(M))
    assert np.array_equal(bits(rgba), bits(want)), (what, "rgba")
    assert (q[n == M] == 256 * M).all() and (q[n < M] < 256 * M).all() and (q[n < M] >> 8 >= n[n < M]).all()


def test_bla_sampled_pixels(ctx, B, O):
    name, kw, make = six_views(B)[4]
    M = kw["max_iter"]
    with bound_view(B, ctx, kw, make) as v:
        got = ctx.mandelbrot_smooth(smooth_params(B, W, H, **kw))
        Z, L, T, scale = v.o.table().tolist(), v.o.length, v.o.bla_table().tolist(), v.o.scale
    dcx, dcy = R.dc_axis(W, scale[0]), R.dc_axis(H, scale[1])
    check_sampled(B, O, got, M, lambda gx, gy: S.bla_scalar(Z, L, T, float(dcx[gx]), float(dcy[gy]), M), name)


@pytest.mark.parametrize("precision", ["perturb", "perturb-bla-deep"])
def test_deep_sampled_pixels(ctx, B, O, precision):
    name, kw, make = six_views(B)[5]
    M = kw["max_iter"]
    if precision == "perturb":
        kw = dict(kw, precision=B.PRECISION_PERTURB)   # a deep orbit bound: PERTURB renders by the deep kernel
    with bound_view(B, ctx, kw, make) as v:
        assert v.o.deep
        got = ctx.mandelbrot_smooth(smooth_params(B, W, H, **kw))
        Z, L, E, mant = v.o.table().tolist(), v.o.length, v.o.scale_exp2, v.o.scale
        if precision != "perturb":
            m_, e_ = v.o.bla_deep_table()
            tab = (m_.tolist(), e_.tolist())
    ux, uy = D.u_axis(W, mant[0]), D.u_axis(H, mant[1])
    if precision == "perturb":
        scalar = lambda gx, gy: S.deep_scalar(Z, L, float(ux[gx]), float(uy[gy]), E, M)
    else:
        scalar = lambda gx, gy: S.bla_deep_scalar(Z, L, tab, float(ux[gx]), float(uy[gy]), E, M)
    check_sampled(B, O, got, M, scalar, precision)


# ---- identities between the kernels -------------------------------------------------------------------------------------------------------
def test_forced_deep_kernel_gives_perturbs_plane(ctx, B):
    name, kw, make = six_views(B)[3]
    want_n, want_q = restated(3)
    with bound_view(B, ctx, kw, make):
        got = ctx.mandelbrot_smooth(smooth_params(B, W, H, flags=B.MANDEL_PERTURB_FORCE_DEEP, **kw))
    check_planes(B, got, want_n, want_q, kw["max_iter"], "PERTURB under FORCE_DEEP")


def test_bla_deep_on_a_shallow_orbit_gives_blas_plane(ctx, B):
    M = 20000
    with B.Orbit(K4[0], K4[1], 1e-20, 1e-20, M) as o:
        o.bla()
        o.bla_deep()
        ctx.bind_mandelbrot_orbit(o)
        try:
            a = ctx.mandelbrot_smooth(smooth_params(B, W, H, max_iter=M, precision=B.PRECISION_PERTURB_BLA, **ZERO))
            b = ctx.mandelbrot_smooth(smooth_params(B, W, H, max_iter=M, precision=B.PRECISION_PERTURB_BLA_DEEP, **ZERO))
        finally:
            ctx.bind_mandelbrot_orbit(None)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(bits(a[0]), bits(b[0]))
    assert len(np.unique(a[2])) > len(np.unique(a[1])) >= 10


def test_bla_with_an_empty_table_gives_perturbs_plane(ctx, B, O):
    M = 300
    with B.Orbit("-1.2", "0.9", 3.0, 3.0, M) as o:
        assert o.length == 1                                         # the reference escapes at once: no BLA entry
        o.bla()
        o.bla_deep()
        Z, L = o.table(), o.length
        ctx.bind_mandelbrot_orbit(o)
        try:
            planes = [ctx.mandelbrot_smooth(smooth_params(B, W, H, max_iter=M, precision=p, flags=f, **ZERO))
                      for p, f in ((B.PRECISION_PERTURB, 0), (B.PRECISION_PERTURB_BLA, 0), (B.PRECISION_PERTURB_BLA_DEEP, 0),
                                   (B.PRECISION_PERTURB, B.MANDEL_PERTURB_FORCE_DEEP))]
        finally:
            ctx.bind_mandelbrot_orbit(None)
    n, zx, zy, cx, cy = S.perturb_plane_capture(R, Z, L, W, H, M, (3.0, 3.0))
    want_q = S.smooth_count(O, n, M, zx, zy, cx, cy)
    assert len(np.unique(n)) >= 10 and (n == M).any()
    for got in planes:
        check_planes(B, got, n, want_q, M, "L = 1")


# ---- where the capture can go wrong -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_capture_in_every_part_of_the_loop(ctx, B, O, precision):
    prec = B.PRECISION_F32 if precision == "f32" else B.PRECISION_F64
    centre, scale = (-0.445, 0.0), (2.34, 2.34)

    def want(w, h, M):
        if precision == "f32":
            st = S.f32_capture(w, h, M, centre, scale)
        else:
            st = S.f64_plane_capture(F, w, h, M, centre, scale)
        return st[0], S.smooth_count(O, st[0], M, *st[1:])

    for M in (1, 5, 8, 13, 128):      # the first block only; the tail loop only; one block; block + tail; replayed fast blocks
        n, q = want(67, 45, M)
        got = ctx.mandelbrot_smooth(smooth_params(B, 67, 45, max_iter=M, precision=prec, centre=centre, scale=scale))
        check_planes(B, got, n, q, M, (precision, M))
        if M % 8:
            assert ((n >= 8 * (M // 8)) & (n < M)).any()             # some pixel escapes in the max_iter % 8 tail loop
    assert ((n > 16) & (n < M)).any() and (n < 8).any()              # M = 128: escapes in replayed fast blocks and in the first block
    interior = n == M
    assert interior.any() and (got[2][interior] == 256 * M).all()
    assert np.array_equal(bits(got[0][interior]), bits(np.broadcast_to(B.colour_lut(M)[M], got[0][interior].shape)))
    for w, h in ((1, 1), (8, 8), (9, 1)):
        n, q = want(w, h, 128)
        got = ctx.mandelbrot_smooth(smooth_params(B, w, h, max_iter=128, precision=prec, centre=centre, scale=scale))
        check_planes(B, got, n, q, 128, (precision, w, h))


# ---- every route gives the whole image's bytes --------------------------------------------------------------------------------------------
def test_every_route_gives_the_whole_images_bytes(ctx, B):
    import torch
    kw = dict(max_iter=256)
    p = smooth_params(B, W, H, **kw)
    rgba, n, q = ctx.mandelbrot_smooth(p)
    want_n, want_q = restated(0)
    assert np.array_equal(n, want_n) and np.array_equal(q, want_q)
    rgba8 = ctx.convert_rgba8(rgba, 255.0)
    assert not np.array_equal(rgba8, ctx.mandelbrot_rgba8(B.mandelbrot_params(W, H, **kw)))      # the colouring does change the picture
    # a row tile, of both host calls
    for r0, r1 in ((0, 8), (37, 90), (123, H)):
        t = ctx.mandelbrot_smooth(smooth_params(B, W, H, row_begin=r0, row_end=r1, **kw))
        assert np.array_equal(bits(t[0]), bits(rgba[r0:r1])) and np.array_equal(t[1], n[r0:r1]) and np.array_equal(t[2], q[r0:r1])
        t = ctx.mandelbrot(smooth_params(B, W, H, row_begin=r0, row_end=r1, **kw))
        assert np.array_equal(bits(t[0]), bits(rgba[r0:r1])) and np.array_equal(t[1], n[r0:r1])
        # a band of render_rgba8
        assert np.array_equal(ctx.mandelbrot_rgba8(smooth_params(B, W, H, row_begin=r0, row_end=r1, **kw)), rgba8[r0:r1])
    assert np.array_equal(ctx.mandelbrot_rgba8(p), rgba8)
    # interleaved tiles
    blk, n_tiles = 8, 3
    for t in range(n_tiles):
        rows = [r for r in range(H) if (r // blk) % n_tiles == t]
        tp = smooth_params(B, W, H, row_begin=t * blk, row_end=H, row_block=blk, row_stride=blk * n_tiles, **kw)
        assert B.tile_rows(tp) == len(rows)
        g = ctx.mandelbrot_smooth(tp)
        assert np.array_equal(bits(g[0]), bits(rgba[rows])) and np.array_equal(g[1], n[rows]) and np.array_equal(g[2], q[rows])
    # render_banded, both formats
    for band in (16, 50, H):
        out, heard = ctx.mandelbrot_banded(p, band)
        assert np.array_equal(bits(out), bits(rgba)) and heard[-1] == H
        out, _ = ctx.mandelbrot_banded(p, band, rgba8=True)
        assert np.array_equal(out, rgba8)
    # the device forms, uint32 and uint16 counts
    d_rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    d_n = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    d_n16 = torch.zeros((H, W), dtype=torch.int16, device="cuda")
    d_q = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.mandelbrot_device(p, d_rgba.data_ptr(), d_n.data_ptr())
    ctx.synchronize()
    assert np.array_equal(bits(d_rgba.cpu().numpy()), bits(rgba)) and np.array_equal(d_n.cpu().numpy().view(np.uint32), n)
    d_rgba.zero_(); d_n.zero_()
    torch.cuda.synchronize()
    ctx.mandelbrot_smooth_device(p, d_rgba.data_ptr(), d_n.data_ptr(), d_q.data_ptr())
    ctx.synchronize()
    assert np.array_equal(bits(d_rgba.cpu().numpy()), bits(rgba)) and np.array_equal(d_n.cpu().numpy().view(np.uint32), n)
    assert np.array_equal(d_q.cpu().numpy().view(np.uint32), q)
    d_rgba.zero_(); d_q.zero_()
    torch.cuda.synchronize()
    ctx.mandelbrot_smooth_device(smooth_params(B, W, H, flags=B.MANDEL_ITERS_U16, **kw), d_rgba.data_ptr(), d_n16.data_ptr(), d_q.data_ptr())
    ctx.synchronize()
    assert np.array_equal(d_n16.cpu().numpy().view(np.uint16), n.astype(np.uint16)) and np.array_equal(d_q.cpu().numpy().view(np.uint32), q)
    assert np.array_equal(bits(d_rgba.cpu().numpy()), bits(rgba))
    d_q.zero_()
    torch.cuda.synchronize()
    ctx.mandelbrot_smooth_device(p, 0, 0, d_q.data_ptr())            # the smooth plane alone
    ctx.synchronize()
    assert np.array_equal(d_q.cpu().numpy().view(np.uint32), q)


def test_render_after_a_warm_up_with_the_flag(B):
    L = B.lib()
    L.mc_context_warmup_mandelbrot.argtypes = [C.c_void_p, C.POINTER(B.MandelbrotParams), C.c_int]
    want_n, want_q = restated(0)
    with B.Context(0) as c2:
        p = smooth_params(B, W, H, max_iter=256)
        for how in (0, 1, 2, 3):
            assert L.mc_context_warmup_mandelbrot(c2._h, C.byref(p), how) == 0
        check_planes(B, c2.mandelbrot_smooth(p), want_n, want_q, 256, "after the warm-up")
        p64 = smooth_params(B, 40, 24, max_iter=128, precision=B.PRECISION_F64)
        assert L.mc_context_warmup_mandelbrot(c2._h, C.byref(p64), 1) == 0
        a = c2.mandelbrot_smooth(p64)
    with B.Context(0) as c3:
        b = c3.mandelbrot_smooth(p64)                               # the same render on a context never warmed up
    assert np.array_equal(a[2], b[2]) and np.array_equal(bits(a[0]), bits(b[0]))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, B):
    import torch
    w, h, M = 64, 48, 200
    d_rgba = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    d_it = torch.zeros((4 * h, 4 * w), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L = B.lib()
    L.mc_context_warmup_mandelbrot.argtypes = [C.c_void_p, C.POINTER(B.MandelbrotParams), C.c_int]

    def refused(call, status=INVALID, says=None):
        with pytest.raises(B.McError) as e:
            call()
        assert e.value.status == status, e.value
        if says:
            assert says in str(e.value), e.value

    combos = [(dict(flags=B.MANDEL_COLOUR_EQUALISED), "MC_MANDEL_COLOUR_EQUALISED"),
              (dict(supersample=2), "MC_MANDEL_SUPERSAMPLE"),
              (dict(supersample=8), "MC_MANDEL_SUPERSAMPLE"),
              (dict(supersample=4, adaptive=True), "MC_MANDEL_SUPERSAMPLE_ADAPTIVE"),
              (dict(adaptive=True), "MC_MANDEL_SUPERSAMPLE_ADAPTIVE"),
              (dict(flags=B.MANDEL_FMA), "MC_MANDEL_FMA")]
    for extra, word in combos:
        flags = extra.pop("flags", 0)
        p = smooth_params(B, w, h, flags=flags, max_iter=M, **extra)
        refused(lambda: ctx.mandelbrot(p), says=word)
        refused(lambda: ctx.mandelbrot(p, want_iters=False), says=word)
        refused(lambda: ctx.mandelbrot_smooth(p), says=word)
        refused(lambda: ctx.mandelbrot_rgba8(p), says=word)
        refused(lambda: ctx.mandelbrot_banded(p, 16), says=word)
        refused(lambda: ctx.mandelbrot_device(p, d_rgba.data_ptr(), d_it.data_ptr()), says=word)
        refused(lambda: ctx.mandelbrot_smooth_device(p, d_rgba.data_ptr(), d_it.data_ptr(), 0), says=word)
        assert L.mc_context_warmup_mandelbrot(ctx._h, C.byref(p), 1) == INVALID
    # the calls that build colours from a plane of integer counts
    p = smooth_params(B, w, h, max_iter=M)
    ident = np.arange(M + 1, dtype=np.uint32)
    refused(lambda: ctx.mandelbrot_recolour_device(p, d_it.data_ptr(), 4, ident, d_rgba.data_ptr()), says="MC_MANDEL_COLOUR_SMOOTH")
    refused(lambda: ctx.mandelbrot_resolve_device(smooth_params(B, w, h, max_iter=M, supersample=2), d_it.data_ptr(), 4, None,
                                                  d_rgba.data_ptr()), says="MC_MANDEL_COLOUR_SMOOTH")
    refused(lambda: ctx.mandelbrot_assemble_device(p, d_it.data_ptr(), 4, 1, 8, h, d_rgba.data_ptr()), says="MC_MANDEL_COLOUR_SMOOTH")
    with B.Multi(1) as mm:
        refused(lambda: mm.mandelbrot(p), UNSUPPORTED, "MC_MANDEL_COLOUR_SMOOTH")
        refused(lambda: mm.mandelbrot_rgba8(p), UNSUPPORTED, "MC_MANDEL_COLOUR_SMOOTH")
    # the new calls' own rules; max_iter above 2^24 - 1
    refused(lambda: ctx.mandelbrot_smooth(B.mandelbrot_params(w, h, max_iter=M)), says="must carry MC_MANDEL_COLOUR_SMOOTH")
    refused(lambda: ctx.mandelbrot_smooth_device(B.mandelbrot_params(w, h, max_iter=M), d_rgba.data_ptr(), 0, 0), says="must carry")
    refused(lambda: ctx.mandelbrot_smooth(p, want_rgba=False, want_iters=False, want_smooth=False))
    refused(lambda: ctx.mandelbrot_smooth_device(p, 0, 0, 0))
    refused(lambda: ctx.mandelbrot_smooth_device(p, 0, 0, d_it.data_ptr() + 2))
    refused(lambda: ctx.mandelbrot_smooth(smooth_params(B, w, h, flags=B.MANDEL_ITERS_U16, max_iter=M)))
    big = smooth_params(B, 8, 8, max_iter=S.MAX_ITER_LIMIT + 1, centre=(2.0, 2.0), scale=(0.1, 0.1))
    refused(lambda: ctx.mandelbrot_smooth(big), says="2^24 - 1")
    refused(lambda: ctx.mandelbrot(big), says="2^24 - 1")
    refused(lambda: ctx.mandelbrot_rgba8(big), says="2^24 - 1")
    # the largest max_iter renders (every pixel of this view escapes at once), and the context still renders, smooth and plain
    top = smooth_params(B, 8, 8, max_iter=S.MAX_ITER_LIMIT, centre=(2.0, 2.0), scale=(0.1, 0.1))
    _, n, q = ctx.mandelbrot_smooth(top, want_rgba=False)
    assert (n == 0).all() and (q < 5 * 256).all()
    rgba, n, q = ctx.mandelbrot_smooth(p)
    assert np.array_equal(bits(rgba), bits(S.colour(q, M, B.colour_lut(M))))
    rgba, n2 = ctx.mandelbrot(B.mandelbrot_params(w, h, max_iter=M))
    assert np.array_equal(n, n2) and np.array_equal(bits(rgba), bits(B.colour_lut(M)[n2]))


# ---- the app --------------------------------------------------------------------------------------------------------------------------------
def run_app(tmp_path, name, *args, ok=True):
    out = tmp_path / name
    r = subprocess.run([APP, "--out", str(out), "--quiet"] + list(args), capture_output=True, text=True, cwd=tmp_path, timeout=180)
    if not ok:
        assert r.returncode != 0, r.stdout + r.stderr
        return None, r.stdout
    assert r.returncode == 0, r.stdout + r.stderr
    from PIL import Image
    return np.asarray(Image.open(out).convert("RGBA")), r.stdout


def test_app_colour_smooth(ctx, B, tmp_path):
    w, h = 160, 96
    size = ["--width", str(w), "--height", str(h), "--max-iter", "300"]
    want = ctx.mandelbrot_rgba8(smooth_params(B, w, h, max_iter=300))
    assert not np.array_equal(want, ctx.mandelbrot_rgba8(B.mandelbrot_params(w, h, max_iter=300)))
    for extra in ([], ["--gpu-postprocess"], ["--streamed-save"], ["--gpu-postprocess", "--streamed-save"]):
        img, text = run_app(tmp_path, "smooth.png", "--colour", "smooth", *size, *extra)
        assert np.array_equal(img, want), extra
        assert "has no effect" not in text                          # the normal banded, streamed save
    _, text = run_app(tmp_path, "no.png", "--colour", "smooth", "--supersample", "2", *size, ok=False)
    assert "--colour smooth" in text
