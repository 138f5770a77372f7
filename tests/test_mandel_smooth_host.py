"""MC_MANDEL_COLOUR_SMOOTH without a GPU: the capture variants of tests/mandel_smooth_ref.py against the existing statements of every
precision; mc_mandelbrot_smooth_count against the restatement on random escape states and on the edge cases of the contract;
mc_mandelbrot_smooth_colour against the restated colour; the motivating fact (how many more distinct values the smooth count takes, and how
few pixels hit the continuation's cap) on the reference view."""
import ctypes
import math

import numpy as np
import pytest

import mandel_bla_deep_ref as BD
import mandel_bla_ref as BR
import mandel_f64_ref as F
import mandel_perturb_deep_ref as D
import mandel_perturb_ref as R
import mandel_smooth_ref as S

K4 = R.DEEP_CENTRE
K4F = (float(K4[0]), float(K4[1]))
INVALID = 1


def escaped_beyond_two(n, zx, zy, M):
    e = np.asarray(n) < M
    r = np.asarray(zx, np.float64)[e] ** 2 + np.asarray(zy, np.float64)[e] ** 2
    return e.any() and bool((r > 2.0).all())


def test_constant_and_symbols(B):
    assert B.MANDEL_COLOUR_SMOOTH == 64
    for name in ("mc_mandelbrot_render_smooth", "mc_mandelbrot_render_smooth_device_async", "mc_mandelbrot_smooth_count",
                 "mc_mandelbrot_smooth_colour"):
        assert name in B.declared_symbols() and hasattr(B.lib(), name), name


# ---- the capture variants count as the existing statements do --------------------------------------------------------------------------
def test_f32_capture_counts_as_the_oracle(O):
    W, H, M = 61, 47, 128
    n, zx, zy, cx, cy = S.f32_capture(W, H, M)
    assert np.array_equal(n, O.mandelbrot_iters(W, H, M, precision=0))
    assert escaped_beyond_two(n, zx, zy, M) and (n == M).any()
    assert np.array_equal(zx.astype(np.float32).astype(np.float64), zx) and np.array_equal(cx.astype(np.float32).astype(np.float64), cx)


def test_ds_capture_counts_as_the_oracle(O):
    W, H, M = 37, 29, 500
    view = O.make_view(K4F[0], K4F[1], 1e-6, 1e-6)
    n, zx, zy, cx, cy = S.ds_capture(O, W, H, M, view)
    assert np.array_equal(n, O.mandelbrot_iters(W, H, M, view=view, precision=1))
    assert escaped_beyond_two(n, zx, zy, M)
    assert len(np.unique(cx)) == W and len(np.unique(cy)) == H      # the low words tell neighbouring columns apart


def test_f64_capture_counts_as_the_f64_statement():
    W, H, M = 41, 31, 3000
    n, zx, zy, cx, cy = S.f64_plane_capture(F, W, H, M, K4F, (1e-12, 1e-12 * 2 / 3))
    assert np.array_equal(n, F.mandelbrot_iters_f64(W, H, M, K4F, (1e-12, 1e-12 * 2 / 3)))
    assert escaped_beyond_two(n, zx, zy, M)


def test_perturb_capture_counts_as_the_perturb_statement(B):
    W, H = 41, 31
    for centre, scale, M in ((K4, 1e-10, 3000), (("-0.445", "0"), 2.34, 300)):
        with B.Orbit(centre[0], centre[1], scale, scale, M) as o:
            Z, L = o.table(), o.length
        n, zx, zy, cx, cy = S.perturb_plane_capture(R, Z, L, W, H, M, (scale, scale))
        assert np.array_equal(n, R.plane(Z, L, W, H, M, (scale, scale)))
        assert escaped_beyond_two(n, zx, zy, M) and len(np.unique(n)) >= 10
        dcx, dcy = R.dc_axis(W, scale), R.dc_axis(H, scale)
        assert np.array_equal(cx, np.broadcast_to(Z[1, 0] + dcx[None, :], (H, W))) and len(np.unique(cx)) == W
        assert np.array_equal(cy, np.broadcast_to(Z[1, 1] + dcy[:, None], (H, W)))
        Zl = Z.tolist()
        for gx, gy in [(0, 0), (40, 30), (20, 15), (7, 23)]:
            got = S.perturb_scalar(Zl, L, float(dcx[gx]), float(dcy[gy]), M)
            assert got[0] == R.scalar_iters(Zl, L, float(dcx[gx]), float(dcy[gy]), M) == n[gy, gx]
            assert got[1:] == (zx[gy, gx], zy[gy, gx], cx[gy, gx], cy[gy, gx])


def pixels(W, H, k):
    rng = np.random.default_rng(W * H + k)
    return list(zip(rng.integers(0, W, k).tolist(), rng.integers(0, H, k).tolist()))


def test_scalar_captures_count_as_the_scalar_statements(B):
    W, H = 64, 48
    # the deep loop and the deep BLA loop on the M(3,3) view at 1e-1000
    c, m, E = D.view(D.M33, "1e-1000")
    M = 6000
    with B.Orbit(c[0], c[1], m[0], m[1], M, E) as o:
        assert o.deep
        o.bla_deep()
        Z, L = o.table().tolist(), o.length
        mant, exps = o.bla_deep_table()
    tab = (mant.tolist(), exps.tolist())
    ux, uy = D.u_axis(W, m[0]), D.u_axis(H, m[1])
    seen = set()
    for gx, gy in pixels(W, H, 10):
        a = S.deep_scalar(Z, L, float(ux[gx]), float(uy[gy]), E, M)
        assert a[0] == D.scalar_iters(Z, L, float(ux[gx]), float(uy[gy]), E, M)
        b = S.bla_deep_scalar(Z, L, tab, float(ux[gx]), float(uy[gy]), E, M)
        assert b[0] == BD.scalar_iters(Z, L, tab, float(ux[gx]), float(uy[gy]), E, M)
        for v in (a, b):
            assert v[0] == M or (v[1] * v[1]) + (v[2] * v[2]) > 2.0
            assert v[3:] == (Z[1][0], Z[1][1])                      # 2^E u is far below an ulp of c_ref
        seen.add(a[0])
    assert len(seen) >= 3
    # the BLA loop on K4 at 1e-10
    M = 3000
    with B.Orbit(K4[0], K4[1], 1e-10, 1e-10, M) as o:
        o.bla()
        Z, L, T = o.table().tolist(), o.length, o.bla_table().tolist()
    dcx, dcy = R.dc_axis(W, 1e-10), R.dc_axis(H, 1e-10)
    seen = set()
    for gx, gy in pixels(W, H, 10):
        a = S.bla_scalar(Z, L, T, float(dcx[gx]), float(dcy[gy]), M)
        assert a[0] == BR.scalar_iters(Z, L, T, float(dcx[gx]), float(dcy[gy]), M)
        assert a[0] == M or (a[1] * a[1]) + (a[2] * a[2]) > 2.0
        seen.add(a[0])
    assert len(seen) >= 3 and min(seen) < M


# ---- mc_mandelbrot_smooth_count -----------------------------------------------------------------------------------------------------------
def check_count(B, O, n, M, zx, zy, cx, cy):
    got = B.smooth_count(n, M, zx, zy, cx, cy)
    want = S.smooth_count(O, n, M, zx, zy, cx, cy)
    bad = got != want
    assert not bad.any(), (int(bad.sum()), np.asarray(n)[bad][:3], got[bad][:3], want[bad][:3])
    return got


def test_smooth_count_on_random_escape_states(B, O):
    # an escape is z = w^2 + c with |w|^2 <= 2 and |z|^2 > 2: |z| in (sqrt 2, 2 + |c|]; |c| <= 4
    N, M = 101000, 50000          # a margin over the 100 000 states the check needs: a draw with |z|^2 <= 2 after rounding is dropped
    rng = np.random.default_rng(20)
    cr, ca = 4.0 * np.sqrt(rng.random(N)), 2 * np.pi * rng.random(N)
    cx, cy = cr * np.cos(ca), cr * np.sin(ca)
    zr = np.sqrt(2.0) + (2.0 + cr - np.sqrt(2.0)) * rng.random(N)
    zr[: N // 10] = np.sqrt(2.0) * (1.0 + 1e-9 * rng.random(N // 10))   # a tenth barely outside
    za = 2 * np.pi * rng.random(N)
    zx, zy = zr * np.cos(za), zr * np.sin(za)
    keep = (zx * zx) + (zy * zy) > 2.0
    n = rng.integers(0, M, N).astype(np.uint32)
    q = check_count(B, O, n[keep], M, zx[keep], zy[keep], cx[keep], cy[keep])
    assert keep.sum() >= 100000
    assert (q >= 256 * n[keep].astype(np.uint64)).all() and (q < 256 * M).all()
    assert len(np.unique(q & 255)) == 256                           # every fraction occurs


def test_smooth_count_edge_cases(B, O):
    M = 1000
    up = math.nextafter
    rows = [
        # n, zx, zy, cx, cy
        (5, math.sqrt(up(2.0, 3.0)), 0.0, 0.3, 0.5),                # r barely above 2
        (5, 1.0, up(1.0, 2.0), -0.7, 0.2),
        (5, 256.0, up(0.0, 1.0), 0.1, 0.1),                         # r = 65536 and just above: k = 0 or 1
        (5, up(256.0, 257.0), 0.0, 0.1, 0.1),
        (5, 300.0, 0.0, 0.1, 0.1),                                  # r in (65536, 65536^2]
        (5, 65536.0, 0.0, 0.1, 0.1),                                # r = 65536^2: fraction 0
        (5, 60000.0, 20000.0, 1.0, -1.0),
        (5, 1e10, 1e10, 0.0, 0.0),                                  # beyond 65536^2: t clamps to 1
        (5, 1e19, 0.0, 0.0, 0.0),                                   # (float)r = 1e38
        (5, 1.9e19, 0.0, 0.0, 0.0),                                 # (float)r overflows: inf, taken as FLT_MAX
        (5, 1e200, 0.0, 0.0, 0.0),                                  # r = inf in double
        (5, math.inf, 0.0, 0.0, 0.0),
        (5, math.inf, math.inf, 0.0, 0.0),
        (5, math.nan, 0.0, 0.0, 0.0),                               # NaN runs to the cap
        (5, 1.5, 1.5, math.nan, 0.0),
        (5, 1.9 * 1.9 - 1.9, 0.0, -1.9, 0.0),                       # the antenna: c = -1.9 stays bounded, the cap is hit
        (5, 2.0, 0.0, -2.0, 0.0),                                   # c = -2: z = 2 is a fixed point with r = 4
        (5, -2.0, 0.0, -2.0, 0.0),
        (0, 1.5, 0.0, 1.5, 0.0),                                    # n = 0
        (M - 1, 1.5, 0.1, 0.3, 0.5),                                # n + k runs into the 256 M - 1 clamp
        (M - 1, 256.5, 0.0, 0.3, 0.5),                              # k = 0 at n = M - 1: no clamp unless F = 256
        (M - 1, 2.0, 0.0, -2.0, 0.0),                               # the cap at the clamp
        (M - 3, 1.5, 0.1, 0.3, 0.5),
        (M, 0.0, 0.0, 0.3, 0.5),                                    # n = M: interior
        (M, math.nan, math.inf, 0.3, 0.5),
    ]
    a = np.array(rows, np.float64)
    n = a[:, 0].astype(np.uint32)
    q = check_count(B, O, n, M, a[:, 1], a[:, 2], a[:, 3], a[:, 4])
    by = {r[:3]: int(v) for r, v in zip(rows, q)}
    assert by[(5, 256.0, up(0.0, 1.0))] == 256 * 6 + (by[(5, 256.0, up(0.0, 1.0))] & 255)      # r = 65536 is not beyond: one more step
    assert by[(5, 65536.0, 0.0)] == 256 * 5                          # +0: the value one iteration earlier would have given
    assert by[(5, 1e10, 1e10)] == 256 * 5 and by[(5, 1e200, 0.0)] == 256 * 5 and by[(5, math.inf, 0.0)] == 256 * 5
    assert int(q[13]) == 256 * (5 + 64) + 256                        # NaN: the cap, rf = 65536, F = 256
    assert by[(5, 2.0, 0.0)] == by[(5, -2.0, 0.0)] == 256 * (5 + 64) + 256
    assert int(q[15]) == 256 * (5 + 64) + 256                        # c = -1.9
    assert by[(M - 1, 1.5, 0.1)] == 256 * M - 1 and by[(M - 1, 2.0, 0.0)] == 256 * M - 1
    assert 256 * (M - 1) <= by[(M - 1, 256.5, 0.0)] < 256 * M
    assert int(q[-1]) == int(q[-2]) == 256 * M
    assert (q[:-2] < 256 * M).all()                                  # an escaped pixel never reaches 256 M
    # the largest max_iter; above it, n above max_iter and a NULL result are refused
    top = S.MAX_ITER_LIMIT
    q = check_count(B, O, np.array([top - 1, top - 70, top, 0], np.uint32), top, [1.5, 1.5, 0.0, 300.0], [0.1, 0.1, 0.0, 0.0], 0.3, 0.5)
    assert int(q[0]) == 256 * top - 1 and int(q[2]) == 256 * top and int(q[3]) < 256
    out = ctypes.c_uint32()
    fn = B.lib().mc_mandelbrot_smooth_count
    assert fn(0, top + 1, 1.5, 0.0, 0.0, 0.0, ctypes.byref(out)) == INVALID
    assert fn(0, 0, 1.5, 0.0, 0.0, 0.0, ctypes.byref(out)) == INVALID
    assert fn(11, 10, 1.5, 0.0, 0.0, 0.0, ctypes.byref(out)) == INVALID
    assert fn(1, 10, 1.5, 0.0, 0.0, 0.0, None) == INVALID


def test_smooth_count_is_continuous_across_the_radius(B, O):
    # the same orbit entered one iteration apart gives the same q: (n, z) and (n + 1, z^2 + c) wherever z is not yet beyond the radius
    rng = np.random.default_rng(7)
    N, M = 2000, 100000
    cx, cy = rng.uniform(-2, 2, N), rng.uniform(-2, 2, N)
    zr, za = rng.uniform(3.0, 200.0, N), rng.uniform(0, 2 * np.pi, N)
    zx, zy = zr * np.cos(za), zr * np.sin(za)
    n = rng.integers(0, 1000, N).astype(np.uint32)
    t = ((zx * zx) - (zy * zy)) + cx
    wy = ((2.0 * zx) * zy) + cy
    a = check_count(B, O, n, M, zx, zy, cx, cy)
    b = check_count(B, O, n + 1, M, t, wy, cx, cy)
    inside = ~((zx * zx) + (zy * zy) > 65536.0)
    assert inside.sum() > 1000 and np.array_equal(a[inside], b[inside])


# ---- mc_mandelbrot_smooth_colour ---------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("M,k_color", [(128, (0.1, 0.7, 0.6, 0.0)), (1, (0.1, 0.7, 0.6, 0.0)), (5000, (0.9, 0.2, 0.4, 0.5))])
def test_smooth_colour_is_the_restatement(B, M, k_color):
    lut = B.colour_lut(M, k_color)
    rng = np.random.default_rng(M)
    q = np.concatenate([np.arange(min(256 * M + 1, 4096)), rng.integers(0, 256 * M + 1, 20000), [256 * M, 256 * M - 1, 0]]).astype(np.uint32)
    got = B.smooth_colour(M, q, k_color)
    want = S.colour(q, M, lut)
    assert np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).any(axis=-1).sum())
    whole = (q & 255) == 0
    assert np.array_equal(bits(got[whole][:, :3]), bits(lut[q[whole] >> 8][:, :3]))     # fr = 0: lut[idx] exactly
    assert np.array_equal(bits(got[q == 256 * M]), bits(np.broadcast_to(lut[M], got[q == 256 * M].shape)))
    assert (got[..., 3] == 1.0).all()
    shaped = B.smooth_colour(M, q[:12].reshape(3, 4), k_color)
    assert shaped.shape == (3, 4, 4) and np.array_equal(bits(shaped.reshape(12, 4)), bits(got[:12]))


def test_smooth_colour_refusals(B):
    for q in ([256 * 128 + 1], [0, 5, 256 * 128 + 1, 3], [0xffffffff]):
        with pytest.raises(B.McError) as e:
            B.smooth_colour(128, np.array(q, np.uint32))
        assert e.value.status == INVALID and "above 256 * max_iter" in str(e.value)
    with pytest.raises(B.McError):
        B.smooth_colour(0, np.array([0], np.uint32))
    with pytest.raises(B.McError):
        B.smooth_colour(S.MAX_ITER_LIMIT + 1, np.array([0], np.uint32))
    assert B.smooth_colour(128, np.zeros(0, np.uint32)).shape == (0, 4)


# ---- the motivating fact ---------------------------------------------------------------------------------------------------------------
def test_smooth_counts_on_the_reference_view(B, O):
    W = H = 400
    M = 128
    n, zx, zy, cx, cy = S.f32_capture(W, H, M)
    esc = n < M
    q = check_count(B, O, n[esc], M, zx[esc], zy[esc], cx[esc], cy[esc])
    dn, dq = len(np.unique(n[esc])), len(np.unique(q))
    # the cap was hit: k = 64 and the fraction's radius taken as 65536 (F = 256); seen without the 256 M - 1 clamp, under a far larger M
    free = S.smooth_count(O, n[esc], 1 << 20, zx[esc], zy[esc], cx[esc], cy[esc])
    capped = free == 256 * (n[esc].astype(np.uint64) + 64) + 256
    print(f"escaped {int(esc.sum())}, distinct n {dn}, distinct q {dq} ({dq / dn:.1f} x), capped {int(capped.sum())} "
          f"({100.0 * capped.mean():.3f} %)")
    assert dq >= 20 * dn                                             # this restatement: 6913 / 127 = 54 x
    assert capped.mean() <= 0.001                                    # this restatement (F32 escape states): 52 pixels, 0.045 %
    assert (q >> 8 >= n[esc]).all()
    whole = S.smooth_count(O, n, M, zx, zy, cx, cy)
    assert (whole[~esc] == 256 * M).all() and (~esc).any()
