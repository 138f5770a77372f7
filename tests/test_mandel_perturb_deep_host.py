"""mc_mandelbrot_orbit_create_deep without a GPU: bits and refusals, identity with mc_mandelbrot_orbit_create above 2^-960, the table
against mpmath at 1e-1000, the tiny-entry refusal, the numpy restatement of the rescaled loop against the scalar one
(tests/mandel_perturb_deep_ref.py) and both against direct high-precision iteration, and the scale helper of the binding."""
import fractions
import math

import numpy as np
import pytest

import mandel_perturb_deep_ref as D
import mandel_perturb_ref as R


@pytest.mark.parametrize("m,E,bits", [
    (0.5, -960, 1057),                       # 2^-961: the first deep scale
    (*math.frexp(1e-300), 1093),             # 1e-300 as (mantissa, exponent)
    (0.5255518873824417, -3321, 3418),       # 1e-1000
    (0.5, -8191, 8288),                      # 2^-8192: the floor
    (1.0, -8192, 8288),                      # the floor again, another mantissa
])
def test_bits(B, m, E, bits):
    with B.Orbit("-0.75", "0.1", m, m * 3, 3, E) as o:
        assert o.bits == bits and o.deep and o.scale_exp2 == E


@pytest.mark.parametrize("sx,sy,E,status", [
    (0.5, 1.0, -8192, 5), (0.999, 0.999, -8192, 5), (1.0, 1.0, -2 ** 31, 5),     # below 2^-8192
    (0.0, 1.0, -3000, 1), (1.0, -0.0, -3000, 1), (math.inf, 1.0, -3000, 1), (1.0, math.nan, -3000, 1),
    (1.0, 1.0, 1100, 5),                                                         # above the double range, not deep
])
def test_refusals(B, sx, sy, E, status):
    with pytest.raises(B.McError) as e:
        B.Orbit("-0.75", "0.1", sx, sy, 10, E)
    assert e.value.status == status


def test_bad_centre_is_still_invalid(B):
    with pytest.raises(B.McError) as e:
        B.Orbit("-0.75x", "0.1", 1.0, 1.0, 10, -3000)
    assert e.value.status == 1


@pytest.mark.parametrize("centre,scale,M", [
    (R.DEEP_CENTRE, (1e-20, 1e-20 * 2 / 3), 3000),
    (("-0.445", "0"), (2.34, 2.34), 500),
    (("-1.25", "0.001"), (2.0 ** -960, 2.0 ** -950), 300),
    (("-0.75", "0.1"), (-1e-100, 3e-100), 300),
])
def test_same_as_the_old_constructor(B, centre, scale, M):
    with B.Orbit(centre[0], centre[1], scale[0], scale[1], M) as old:
        want = (old.table(), old.length, old.bits)
    pairs = [(scale[0], scale[1], 0)]
    for k in (-7, 100, 900):
        pairs.append((math.ldexp(scale[0], k), math.ldexp(scale[1], k), -k))
    for sx, sy, E in pairs:
        with B.Orbit(centre[0], centre[1], sx, sy, M, E) as o:
            assert not o.deep and o.scale == scale and o.scale_exp2 == 0
            assert o.length == want[1] and o.bits == want[2]
            assert np.array_equal(o.table(), want[0])


def test_old_constructor_keeps_refusing_below_2_960(B):
    with pytest.raises(B.McError) as e:
        B.Orbit("-0.75", "0.1", 2.0 ** -961, 1e-10, 10)
    assert e.value.status == 5


def test_table_is_correctly_rounded_at_1e_1000(B):
    M = 4000   # the reference orbit is repelling: its fixed-point error stays far below a double's ulp up to here
    c, m, E = D.view(D.M33, "1e-1000")
    with B.Orbit(c[0], c[1], *m, M, E) as o:
        Z, L, bits = o.table(), o.length, o.bits
    assert bits == 3418 and L == M
    Lm, ref = R.mp_orbit(c[0], c[1], M, bits + 64)
    assert Lm == L
    want = np.array([[float(a), float(b)] for a, b in ref], np.float64)
    assert np.array_equal(Z, want)


def test_tiny_entry_refusal(B):
    """A period-3 nucleus written to 400 digits: Z_3 is about 1e-400, nonzero and far below 2^-960."""
    c = D.nucleus(3, D.NUCLEUS3, 1500, 400)
    _, z = R.mp_orbit(c[0], c[1], 3, 4000)
    mag = max(abs(z[3][0]), abs(z[3][1]))
    assert 0 < mag < 2.0 ** -960 and mag > 1e-420
    m, E = B.scale_from_text("1e-1000")
    with pytest.raises(B.McError) as e:
        B.Orbit(c[0], c[1], m, m, 100, E)
    assert e.value.status == 5 and "Z_3" in str(e.value)
    with B.Orbit(c[0], c[1], 1e-200, 1e-200, 100) as o:   # the same centre at a shallow scale: today's orbit, accepted
        assert o.length == 100


@pytest.mark.parametrize("centre", [("0", "0"), ("-1", "0")])
def test_exact_zero_entries_are_accepted(B, centre):
    m, E = B.scale_from_text("1e-1000")
    with B.Orbit(centre[0], centre[1], m, m, 50, E) as o:
        Z, L = o.table(), o.length
        assert o.deep and L == 50
    assert (Z[2] == 0).all()
    pl = D.plane(Z, L, 8, 6, 50, o.scale, E)
    assert (pl == 50).all()   # interior


def test_numpy_restatement_equals_scalar(B):
    W, H = 24, 16
    for point, depth, M in ((D.M33, "1e-300", 2000), (D.M41, "1e-1000", 9000), (D.M33, "1e-2000", 10000)):
        c, m, E = D.view(point, depth)
        mant = (m[0], -m[1] * 0.75)
        with B.Orbit(c[0], c[1], *mant, M, E) as o:
            Z, L = o.table(), o.length
        pl = D.plane(Z, L, W, H, M, mant, E)
        Zl = Z.tolist()
        ux, uy = D.u_axis(W, mant[0]), D.u_axis(H, mant[1])
        for y in range(0, H, 3):
            for x in range(0, W, 5):
                assert pl[y, x] == D.scalar_iters(Zl, L, float(ux[x]), float(uy[y]), E, M), (depth, x, y)
    Z = np.array([[0.0, 0.0], [-1.0, 0.0], [0.0, 0.0], [-1.0, 0.0]])   # zero entries: the fresh-exponent step after m = 0
    for ux, uy in ((0.3, -0.2), (0.0, 0.0), (-0.5, 0.5)):
        assert D.iterate(Z, 3, [ux], [uy], -3000, 40)[0] == D.scalar_iters(Z.tolist(), 3, ux, uy, -3000, 40)


@pytest.mark.parametrize("point,depth,M", [(D.M33, "1e-300", 2000), (D.M33, "1e-1000", 6000), (D.M41, "1e-1000", 10000)])
def test_accuracy_against_direct_iteration(B, point, depth, M):
    """24 sampled pixels per view against direct fixed-point iteration at bits + 64: measured here, all 24 equal in each view."""
    W, H = 64, 48
    c, m, E = D.view(point, depth)
    with B.Orbit(c[0], c[1], *m, M, E) as o:
        pl = D.plane(o.table(), o.length, W, H, M, o.scale, E)
        bits = o.bits
    rng = np.random.default_rng(11)
    gx, gy = rng.integers(0, W, 24), rng.integers(0, H, 24)
    got = pl[gy, gx]
    truth = np.array([D.mp_iters_deep(c, o.scale, E, W, H, x, y, M, bits + 64) for x, y in zip(gx, gy)])
    assert (got == truth).sum() >= 22, (depth, got.tolist(), truth.tolist())
    assert len(np.unique(truth)) >= 5 and truth.max() < M


@pytest.mark.parametrize("text", ["1e-1000", "6.7e-1001", "-2.5e-3000", "1", "0.75", "3", "1e300", "7e-2466", "123456789e-10"])
def test_scale_from_text(B, text):
    m, e = B.scale_from_text(text)
    assert 0.5 <= abs(m) <= 1.0
    v = fractions.Fraction(text)
    exact = v / fractions.Fraction(2) ** e
    assert m == float(exact)   # the correctly rounded mantissa
    with pytest.raises(ValueError):
        B.scale_from_text("0e5")
