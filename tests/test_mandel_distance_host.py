"""MC_MANDEL_COLOUR_DISTANCE without a GPU: mc_mandelbrot_distance_plane / mc_mandelbrot_distance_colour (the kernel's own source, compiled
for the host) against tests/mandel_distance_ref.py bit for bit, the closed-form cases of the contract, the estimate's agreement with the
analytic 2 |z| ln |z| / |z'| on the reference view, every host refusal."""
import ctypes as C
import functools

import numpy as np
import pytest

import mandel_distance_ref as DR
import mandel_smooth_ref as S

INVALID = 1
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 3), (67, 35)]       # (W, H)
RW, RH, RM = 400, 400, 128                                         # the reference view of the accuracy figures


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def reference_view():
    """(q, cx, cy) of the reference view at 400 x 400, M = 128: the contract's own q (F32 loop, strict log2), computed once."""
    import __graft_entry__ as entry
    O = entry.load_oracle()
    n, zx, zy, cx, cy = S.f32_capture(RW, RH, RM)
    q = S.smooth_count(O, n, RM, zx, zy, cx, cy)
    for a in (q, cx, cy):
        a.setflags(write=False)
    return q, cx, cy


@functools.lru_cache(maxsize=None)
def big_lut():
    import __graft_entry__ as entry
    lut = entry.load_package().bindings.colour_lut(DR.BIG_M)
    lut.setflags(write=False)
    return lut


def check(B, q, M, what, lut=None, thresholds=(1.0, 0.5, 3.0)):
    want = DR.plane(q, M)
    got = B.distance_plane(M, q)
    bad = bits(got) != bits(want)
    assert not bad.any(), (what, "D", int(bad.sum()), got[bad][:4], want[bad][:4])
    lut = B.colour_lut(M) if lut is None else lut
    for T in thresholds:
        c = B.distance_colour(M, q, got, T)
        w = DR.colour(q, want, M, lut, T)
        assert np.array_equal(bits(c), bits(w)), (what, "rgba", T, int((bits(c) != bits(w)).any(axis=-1).sum()))
    return want


def test_constant_and_symbols(B):
    assert B.MANDEL_COLOUR_DISTANCE == 128
    for name in ("mc_mandelbrot_render_distance", "mc_mandelbrot_distance_device_async", "mc_mandelbrot_distance_plane",
                 "mc_mandelbrot_distance_colour"):
        assert name in B.declared_symbols() and hasattr(B.lib(), name), name
    assert B.lib().mc_abi_version() == 3


@pytest.mark.parametrize("W,H", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_synthetic_planes_are_the_restatement(B, W, H):
    M = 200
    seen = set()
    for name, q in DR.synthetic_planes(W, H, M):
        D = check(B, q, M, (name, W, H))
        seen |= set(np.unique(D).tolist())
        if name == "interior":
            assert (D == 0).all()
            assert np.array_equal(bits(B.distance_colour(M, q, D)), bits(np.broadcast_to(B.colour_lut(M)[M], q.shape + (4,))))
    if W * H >= 100:
        assert 0.0 in seen and 4096.0 in seen and len(seen) > 10       # interior contact, flat patches, and gradients in between


@pytest.mark.parametrize("W,H", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_large_differences_are_the_restatement(B, W, H):
    q = DR.large_plane(W, H)
    if W * H >= 4:
        assert DR.g2_of(q).max() > 2.0 ** 53                            # the sum of squares rounds: still one IEEE expression
    check(B, q, DR.BIG_M, ("large", W, H), lut=big_lut(), thresholds=(1.0,))


def test_reference_view_is_the_restatement(B):
    q, _, _ = reference_view()
    D = check(B, q, RM, "reference view")
    assert (D == 0).any() and len(np.unique(D)) > 1000


# ---- closed forms ---------------------------------------------------------------------------------------------------------------------
def test_closed_forms(B):
    M = 200
    lut = B.colour_lut(M)
    for W, H in ((2, 1), (9, 1), (13, 7)):
        q = np.broadcast_to((256 * np.arange(W, dtype=np.uint32))[None, :], (H, W)).copy()
        D = B.distance_plane(M, q)
        assert (bits(D) == bits(np.float32(1477.3197218702985 / 512))).all(), (W, H)      # the doubled border columns included
        assert np.array_equal(bits(B.distance_plane(M, q.T.copy())), bits(D.T))              # and along storage rows
    flat = np.full((6, 11), 12345, np.uint32)
    D = B.distance_plane(M, flat)
    assert (bits(D) == bits(np.float32(4096.0))).all()
    assert np.array_equal(bits(B.distance_colour(M, flat, D)), bits(S.colour(flat, M, lut)))    # D >= T: the smooth colour itself
    assert (bits(B.distance_plane(M, np.full((1, 1), 5, np.uint32))) == bits(np.float32(4096.0))).all()
    # beside an interior pixel: D = 0 and black; the interior pixel keeps lut[M]; diagonal neighbours are not 4-neighbours
    q = np.full((5, 5), 1000, np.uint32)
    q[2, 2] = 256 * M
    D = B.distance_plane(M, q)
    zero = np.zeros((5, 5), bool)
    zero[2, 1:4] = zero[1:4, 2] = True
    assert np.array_equal(D == 0, zero) and (D[~zero] > 0).all()
    rgba = B.distance_colour(M, q, D)
    assert np.array_equal(bits(rgba[2, 2]), bits(lut[M]))
    for y, x in ((1, 2), (3, 2), (2, 1), (2, 3)):
        assert (rgba[y, x, :3] == 0).all() and rgba[y, x, 3] == 1.0      # (a negative base component gives -0.0: black all the same)
    assert np.array_equal(bits(rgba[1, 1]), bits(S.colour(q, M, lut)[1, 1])) and D[1, 1] == np.float32(4096.0)
    # the weight: D / T below the threshold, 1 from the threshold on
    q1 = np.full(4, 300, np.uint32)
    d1 = np.array([0.25, 0.999, 1.0, 7.0], np.float32)
    base = S.colour(q1, M, lut)
    got = B.distance_colour(M, q1, d1, 1.0)
    assert np.array_equal(bits(got[2:]), bits(base[2:]))
    assert np.array_equal(bits(got[0, :3]), bits(base[0, :3] * np.float32(0.25))) and got[0, 3] == 1.0


# ---- accuracy against the analytic estimate ---------------------------------------------------------------------------------------
def test_agrees_with_the_analytic_estimate_on_the_reference_view(B):
    """Measured (printed below; DESIGN.md section 3.15 records them): finite-difference / analytic on the reference view at 400 x 400,
    M = 128, with the contract's own q: medians 0.992 (4-16 px), 0.999 (16-64 px), 0.999 (>= 64 px); the set is 87.3 % of the escaped
    pixels and its ratios lie in 0.724 - 1.891."""
    q, cx, cy = reference_view()
    D = B.distance_plane(RM, q).astype(np.float64)
    escaped = q < 256 * RM
    A = DR.analytic_distance(cx, cy, 2.34 / RW)
    ok = escaped & (A >= 4.0) & ~DR.near_interior(q, RM) & (DR.g2_of(q) > 0)
    ratio = D[ok] / A[ok]
    print(f"\nescaped {int(escaped.sum())}, in the set {int(ok.sum())} ({100.0 * ok.sum() / escaped.sum():.1f} %), "
          f"ratio min {ratio.min():.3f} max {ratio.max():.3f}")
    medians = []
    for lo, hi in ((4, 16), (16, 64), (64, np.inf)):
        r = D[ok & (A >= lo) & (A < hi)] / A[ok & (A >= lo) & (A < hi)]
        medians.append(float(np.median(r)))
        print(f"analytic d in [{lo}, {hi}): {r.size} pixels, median {np.median(r):.4f}, 5th-95th percentile "
              f"{np.percentile(r, 5):.3f} - {np.percentile(r, 95):.3f}")
    low = escaped & (A >= 2.0) & (A < 4.0) & ~DR.near_interior(q, RM) & (DR.g2_of(q) > 0)
    r = D[low] / A[low]
    print(f"analytic d in [2, 4): {r.size} pixels, median {np.median(r):.4f}, 5th-95th percentile {np.percentile(r, 5):.3f} - "
          f"{np.percentile(r, 95):.3f}, within a factor of 2: {100.0 * ((r >= 0.5) & (r <= 2.0)).mean():.1f} %")
    sure = escaped & (A > 0)
    print(f"thresholded at 1 pixel the two disagree on {100.0 * ((D[sure] < 1.0) != (A[sure] < 1.0)).mean():.2f} % of the escaped pixels")
    assert ok.sum() * 2 >= escaped.sum()                                 # the test cannot pass by leaving pixels out
    assert ((ratio >= 0.5) & (ratio <= 2.0)).all(), (ratio.min(), ratio.max())
    assert all(0.9 <= m <= 1.1 for m in medians), medians


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_host_refusals(B):
    L = B.lib()
    M = 200
    q = np.full((3, 4), 100, np.uint32)
    D = np.zeros((3, 4), np.float32)
    out = np.zeros((3, 4, 4), np.float32)
    k = (C.c_float * 4)(0.1, 0.7, 0.6, 0.0)
    pq, pD, po = (a.ctypes.data_as(C.c_void_p) for a in (q, D, out))
    plane, colour = L.mc_mandelbrot_distance_plane, L.mc_mandelbrot_distance_colour
    assert plane(4, 3, M, pq, pD) == 0
    assert plane(4, 3, M, None, pD) == INVALID and plane(4, 3, M, pq, None) == INVALID
    assert plane(0, 3, M, pq, pD) == INVALID and plane(4, 0, M, pq, pD) == INVALID and plane(4, 3, 0, pq, pD) == INVALID
    assert plane(4, 3, DR.BIG_M + 1, pq, pD) == INVALID
    assert colour(M, k, pq, pD, 12, 1.0, po) == 0
    assert colour(M, None, pq, pD, 12, 1.0, po) == INVALID and colour(M, k, None, pD, 12, 1.0, po) == INVALID
    assert colour(M, k, pq, None, 12, 1.0, po) == INVALID and colour(M, k, pq, pD, 12, 1.0, None) == INVALID
    assert colour(M, k, pq, pD, 0, 1.0, po) == INVALID and colour(0, k, pq, pD, 12, 1.0, po) == INVALID
    assert colour(DR.BIG_M + 1, k, pq, pD, 12, 1.0, po) == INVALID
    for T in (0.0, -1.0, float("inf"), float("nan")):
        assert colour(M, k, pq, pD, 12, T, po) == INVALID, T
        assert b"threshold_px" in L.mc_last_error_detail()
    q[1, 2] = 256 * M + 1
    assert plane(4, 3, M, pq, pD) == INVALID and b"above 256 * max_iter" in L.mc_last_error_detail()
    assert colour(M, k, pq, pD, 12, 1.0, po) == INVALID and b"above 256 * max_iter" in L.mc_last_error_detail()
    q[1, 2] = 256 * M                                                    # interior itself is a value of the plane
    assert plane(4, 3, M, pq, pD) == 0 and colour(M, k, pq, pD, 12, 1.0, po) == 0
