"""The exact counts of sampled pixels without a GPU (include/mc_compute.h: "exact counts"): mc_mandelbrot_exact_counts against the
Python-integer restatement (tests/mandel_exact_ref.py) from 3 to 20 limbs and with extra limbs; mc_mandelbrot_exact_pixel_offsets
against the perturbation references' own offset tables, bit for bit; the centre pixel's count against the orbit constructor's L;
a rescaled orbit; and every refusal with its status."""
import ctypes as C

import numpy as np
import pytest

import mandel_exact_ref as X
import mandel_perturb_deep_ref as D
import mandel_perturb_ref as R

W, H = 24, 16
INVALID, UNSUPPORTED = 1, 5


def lattice(count, w=W, h=H):
    """`count` pixels of the w x h view on a fixed lattice, the centre pixel first."""
    px = [(w // 2, h // 2)]
    for i in range(count - 1):
        px.append(((5 * i + 1) % w, (7 * i + 3) % h))
    return np.array(px, np.uint32)


def mis_centre(point, exp2):
    """A Misiurewicz point's text, accurate beyond the bits of a view of scale 2^exp2."""
    return D.misiurewicz(point[0], point[1], point[2], 1 - (exp2 + 1) + 96 + 64)


# (name, centre, (sx, sy), scale_exp2 or None, M, limbs)
CASES = {
    "k4_1e-8": (R.DEEP_CENTRE, (1e-8, 1e-8), None, 2000, 3),
    "m33_2^-100": (mis_centre(D.M33, -100), (1.0, 1.0), -100, 300, 5),
    "m41_2^-850": (mis_centre(D.M41, -850), (1.0, 1.0), -850, 300, 16),
    "m33_2^-900": (mis_centre(D.M33, -900), (1.0, 1.0), -900, 300, 17),
    "m41_2^-1100": (mis_centre(D.M41, -1100), (1.0, 0.75), -1100, 200, 20),   # a deep orbit: the offsets are u with dc_exp2 = E
}


def make(B, name):
    centre, scale, E, M, n = CASES[name]
    o = B.Orbit(centre[0], centre[1], scale[0], scale[1], M, E)
    assert X.limbs_of(o.bits) == n
    return o, centre, M


@pytest.mark.parametrize("name", list(CASES))
def test_pixel_offsets_are_the_kernels_own(B, name):
    o, _, _ = make(B, name)
    with o:
        px = lattice(48)
        dcx, dcy, e = o.exact_pixel_offsets(W, H, px)
        if o.deep:
            wx, wy = D.u_axis(W, o.scale[0], idx=px[:, 0]), D.u_axis(H, o.scale[1], idx=px[:, 1])
            assert e == o.scale_exp2
        else:
            wx, wy = R.dc_axis(W, o.scale[0], idx=px[:, 0]), R.dc_axis(H, o.scale[1], idx=px[:, 1])
            assert e == 0
        assert np.array_equal(dcx.view(np.uint64), wx.view(np.uint64)) and np.array_equal(dcy.view(np.uint64), wy.view(np.uint64))


@pytest.mark.parametrize("extra", [0, 1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_host_counts_equal_the_integer_restatement(B, name, extra):
    o, centre, M = make(B, name)
    with o:
        px = lattice(12)
        dcx, dcy, e = o.exact_pixel_offsets(W, H, px)
        got = o.exact_counts(M, dcx, dcy, e, extra_limbs=extra)
        want = X.counts(centre, o.bits, dcx, dcy, e, M, extra_limbs=extra)
        assert got.tolist() == want
        if name == "k4_1e-8":
            assert len(set(want)) > 3   # a spread of counts, not one value


@pytest.mark.parametrize("name", list(CASES))
def test_centre_pixel_count_is_the_constructors(B, name):
    """dc = 0 exactly at (W / 2, H / 2): the loop is the constructor's own, so n = L - 1 where its orbit escaped."""
    o, centre, M = make(B, name)
    with o:
        dcx, dcy, e = o.exact_pixel_offsets(W, H, lattice(1))
        assert dcx[0] == 0.0 and dcy[0] == 0.0
        n = int(o.exact_counts(o.max_iter, dcx, dcy, e)[0])
        want = X.counts(centre, o.bits, dcx, dcy, e, o.max_iter)[0]
        if o.length < o.max_iter:
            assert n == want == o.length - 1
        else:
            # L = max_iter whether Z_M escapes or not; the reference says which: it escapes (n = L - 1) or runs out (n = M)
            z_m_escapes = want == o.max_iter - 1
            assert want in (o.max_iter - 1, o.max_iter)
            assert n == (o.length - 1 if z_m_escapes else o.max_iter)


def test_hair_reference_centre_count_is_L_minus_1(B):
    """The documented failure's view (test_reference_on_the_hair_is_the_documented_failure): L = M, and the exact count is M - 1."""
    M = 4000
    c = R.mp_hair_point(("-0.5", "0"), ("-0.5", "1"), M, 220, 284)
    with B.Orbit(c[0], c[1], 1e-30, 1e-30, M) as o:
        assert o.length == M
        assert int(o.exact_counts(M, [0.0], [0.0])[0]) == M - 1


def test_a_rescaled_orbit_counts_from_its_sources_centre(B):
    centre = mis_centre(D.M33, -140)
    with B.Orbit(centre[0], centre[1], 1.0, 1.0, 300, -140) as src, src.rescale(1.0, 1.0, -100) as r:
        assert r.bits == src.bits
        px = lattice(8)
        dcx, dcy, e = r.exact_pixel_offsets(W, H, px)
        assert np.array_equal(dcx, R.dc_axis(W, r.scale[0], idx=px[:, 0]))
        assert r.exact_counts(300, dcx, dcy, e).tolist() == X.counts(centre, src.bits, dcx, dcy, e, 300)


def status_of(fn):
    with pytest.raises(Exception) as ei:
        fn()
    return ei.value.status, str(ei.value)


def test_refusals(B):
    with B.Orbit(*R.DEEP_CENTRE, 1e-8, 1e-8, 100) as o:
        one = np.array([0.0, 1.0])
        # an offset with a bit below the last fractional bit: 2^-2000 on 3 limbs, at pixel index 1
        st, text = status_of(lambda: o.exact_counts(10, one, [0.0, 0.0], dc_exp2=-2000))
        assert st == UNSUPPORTED and "pixel 1" in text
        with pytest.raises(X.Unsupported):
            X.counts(R.DEEP_CENTRE, o.bits, one, [0.0, 0.0], -2000, 10)
        # 2^-129 needs a bit of the fourth limb: refused on three, accepted with one extra
        st, text = status_of(lambda: o.exact_counts(10, [0.0], [1.0], dc_exp2=-129))
        assert st == UNSUPPORTED and "pixel 0" in text
        assert o.exact_counts(10, [0.0], [1.0], dc_exp2=-129, extra_limbs=1).tolist() == \
            X.counts(R.DEEP_CENTRE, o.bits, [0.0], [1.0], -129, 10, extra_limbs=1)
        assert o.exact_counts(10, [0.0], [1.0], dc_exp2=-128).tolist() == X.counts(R.DEEP_CENTRE, o.bits, [0.0], [1.0], -128, 10)
        # |c| above 4
        st, text = status_of(lambda: o.exact_counts(10, [0.0, 0.0, 5.0], [0.0, 0.0, 0.0]))
        assert st == UNSUPPORTED and "pixel 2" in text
        assert status_of(lambda: o.exact_counts(10, [1.0], [0.0], dc_exp2=400))[0] == UNSUPPORTED
        assert status_of(lambda: o.exact_counts(10, [0.0], [-4.5]))[0] == UNSUPPORTED
        # more than 131 limbs
        assert status_of(lambda: o.exact_counts(10, [0.0], [0.0], extra_limbs=129))[0] == UNSUPPORTED
        assert o.exact_counts(3, [0.0], [0.0], extra_limbs=128).tolist() == [3]
        # zero pixels, M = 0, not finite, NULLs
        assert status_of(lambda: o.exact_counts(10, [], []))[0] == INVALID
        assert status_of(lambda: o.exact_counts(0, [0.0], [0.0]))[0] == INVALID
        assert status_of(lambda: o.exact_counts(10, [float("nan")], [0.0]))[0] == INVALID
        assert status_of(lambda: o.exact_counts(10, [0.0], [float("inf")]))[0] == INVALID
        L = B.lib()
        d = np.zeros(1)
        n = np.zeros(1, np.uint32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert L.mc_mandelbrot_exact_counts(None, 10, 0, 1, p(d), p(d), 0, p(n)) == INVALID
        assert L.mc_mandelbrot_exact_counts(o._h, 10, 0, 1, None, p(d), 0, p(n)) == INVALID
        assert L.mc_mandelbrot_exact_counts(o._h, 10, 0, 1, p(d), None, 0, p(n)) == INVALID
        assert L.mc_mandelbrot_exact_counts(o._h, 10, 0, 1, p(d), p(d), 0, None) == INVALID
        assert L.mc_mandelbrot_exact_counts(o._h, 10, 0, (1 << 20) + 1, p(d), p(d), 0, p(n)) == INVALID
        # the offsets' own
        assert status_of(lambda: o.exact_pixel_offsets(W, H, [(W, 0)]))[0] == INVALID
        assert status_of(lambda: o.exact_pixel_offsets(W, H, [(0, H)]))[0] == INVALID
        assert status_of(lambda: o.exact_pixel_offsets((1 << 20) + 1, H, [(0, 0)]))[0] == INVALID
        assert status_of(lambda: o.exact_pixel_offsets(W, (1 << 20) + 1, [(0, 0)]))[0] == INVALID
        assert status_of(lambda: o.exact_pixel_offsets(W, 0, [(0, 0)]))[0] == INVALID
        g = np.zeros(1, np.uint32)
        e = C.c_int32(0)
        assert L.mc_mandelbrot_exact_pixel_offsets(o._h, W, H, 1, p(g), p(g), p(d), p(d), None) == INVALID
        assert L.mc_mandelbrot_exact_pixel_offsets(None, W, H, 1, p(g), p(g), p(d), p(d), C.byref(e)) == INVALID
        assert L.mc_mandelbrot_exact_pixel_offsets(o._h, W, H, 0, p(g), p(g), p(d), p(d), C.byref(e)) == INVALID


def test_largest_view_converts_exactly(B):
    """W = H = 2^20, the bound of mc_mandelbrot_exact_pixel_offsets: every offset converts with no extra limb (the 96 guard bits)."""
    with B.Orbit(*R.DEEP_CENTRE, 1e-8, 3e-9, 10) as o:
        n = 1 << 20
        px = [(1, 1), (n - 1, n - 1), (n // 2 + 1, n // 2 - 1), (n // 3, 2 * n // 3), (0, 0), (12345, 987653)]
        dcx, dcy, e = o.exact_pixel_offsets(n, n, px)
        assert o.exact_counts(10, dcx, dcy, e).tolist() == X.counts(R.DEEP_CENTRE, o.bits, dcx, dcy, e, 10)
