"""MC_PRECISION_PERTURB without a GPU: the host reference orbit against mpmath, the refusals of mc_mandelbrot_orbit_create, the numpy
restatement against the scalar one and against direct high-precision iteration (tests/mandel_perturb_ref.py), the gap to F64 it closes,
and the app's option handling."""
import os
import subprocess

import numpy as np
import pytest

import mandel_f64_ref as F
import mandel_perturb_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K4 = R.DEEP_CENTRE


@pytest.fixture(scope="module")
def boundary_views():
    """Boundary points by bisection (their own orbits escape, L < M) and the scales that show a spread of counts around them."""
    return [
        (R.mp_boundary_point(("-0.5", "0"), ("-0.5", "1"), 4000, 70, 134), 1e-20, 4000),
        (R.mp_boundary_point(("0.3", "0"), ("0.3", "1"), 3000, 103, 167), 1e-30, 3000),
        (R.mp_boundary_point(("-0.5", "0"), ("-0.5", "1"), 10000, 190, 254), 1e-50, 10000),
    ]


def test_enum_value(B):
    assert B.PRECISION_PERTURB == 3


@pytest.mark.parametrize("centre,scale,M", [
    (K4, 1e-20, 20000),
    (("-0.75", "0.1"), 1e-20, 20000),                            # the orbit escapes early (L < M)
    (("-0.445", "0"), 2.34, 5000),
])
def test_orbit_against_mpmath(B, centre, scale, M):
    with B.Orbit(centre[0], centre[1], scale, scale, M) as o:
        assert o.bits == R.orbit_bits(scale, scale) and o.max_iter == M
        Z = o.table()
        L, ref = R.mp_orbit(centre[0], centre[1], M, 2 * o.bits)
        assert o.length == L and Z.shape == (L + 1, 2)
    want = np.array([[float(a), float(b)] for a, b in ref], np.float64)
    # within 1 ulp; an entry that cancels to (nearly) 0 carries the fixed point's absolute error instead, a few units of 2^-bits
    assert np.all(np.abs(Z - want) <= np.maximum(np.spacing(np.abs(want)), 2.0 ** (4 - o.bits)))
    assert (Z == want).all(axis=1).mean() >= 0.999
    if centre == ("-0.75", "0.1"):
        assert o.length < 100


@pytest.mark.parametrize("s", ["-0.74364388703715870475219150611477403", "+1.999999999999999999999999999999999e0", "3.9999999999999999999",
                               "-.1234567890123456789012345678901234567890e-3", "0.100000000000000005551115123125782702118158340454101562",
                               "0.1000000000000000055511151231257827021181583404541015625", "-4", "4.", "4e0", "0.000001234567890123e+2",
                               "1234567890123456789e-18", "7e-5", "-0.0", "0"])
def test_z1_is_the_correctly_rounded_double(B, s):
    with B.Orbit(s, "0.25", 1e-12, 1e-12, 1) as o:
        Z = o.table()
    assert Z[1, 0] == float(s) and Z[1, 1] == 0.25


@pytest.mark.parametrize("scale,bits", [(2.34, 95), (1.0, 96), (1e-20, 163), (2.0 ** -950, 1046), (2.0 ** -960, 1056), (1e10, 64)])
def test_bits_follow_the_formula(B, scale, bits):
    with B.Orbit("-0.5", "0", scale, scale * 3, 2) as o:
        assert o.bits == bits == R.orbit_bits(scale, scale * 3)


@pytest.mark.parametrize("s", ["", " 0.5", "0.5 ", "0x1p-2", "inf", "-inf", "nan", "1e", "1e+", ".", "-", "+.", "1.2.3", "e5", "1,5",
                               "4.0000000000000000000000000000001", "-4.000000000000000000000000000000000000000001", "5", "1e1",
                               "0.5" + "0" * 4094])
def test_malformed_or_large_centre_is_refused(B, s):
    with pytest.raises(B.McError) as e:
        B.Orbit(s, "0", 1e-10, 1e-10, 100)
    assert e.value.status == 1
    with pytest.raises(B.McError) as e:
        B.Orbit("0", s, 1e-10, 1e-10, 100)
    assert e.value.status == 1


def test_longest_accepted_centre(B):
    with B.Orbit("0.5" + "0" * 4093, "0", 1e-10, 1e-10, 3) as o:
        assert o.table()[1, 0] == 0.5


@pytest.mark.parametrize("sx,sy,status", [(0.0, 1e-10, 1), (1e-10, -0.0, 1), (float("inf"), 1e-10, 1), (1e-10, float("nan"), 1),
                                          (2.0 ** -961, 1e-10, 5), (1e-10, -(2.0 ** -1000), 5), (1e-300, 1e-300, 5)])
def test_bad_scales_are_refused(B, sx, sy, status):
    with pytest.raises(B.McError) as e:
        B.Orbit("-0.5", "0", sx, sy, 100)
    assert e.value.status == status


def test_zero_max_iter_is_refused(B):
    with pytest.raises(B.McError) as e:
        B.Orbit("-0.5", "0", 1e-10, 1e-10, 0)
    assert e.value.status == 1


def test_numpy_restatement_equals_scalar(B):
    W, H, M = 24, 16, 3000
    for centre, scale in ((K4, 1e-10), (("-0.445", "0"), 2.34), (("-0.5", "0.601612404061598243828492"), 1e-20)):
        with B.Orbit(centre[0], centre[1], scale, scale, M) as o:
            Z, L = o.table(), o.length
        pl = R.plane(Z, L, W, H, M, (scale, scale))
        Zl = Z.tolist()
        dx, dy = R.dc_axis(W, scale), R.dc_axis(H, scale)
        for y in range(0, H, 3):
            for x in range(0, W, 5):
                assert pl[y, x] == R.scalar_iters(Zl, L, float(dx[x]), float(dy[y]), M), (centre, x, y)


def sampled_quality(B, centre, scale, M, n=160, W=64, H=48):
    with B.Orbit(centre[0], centre[1], scale, scale, M) as o:
        Z, L, bits = o.table(), o.length, o.bits
    pl = R.plane(Z, L, W, H, M, (scale, scale))
    rng = np.random.default_rng(7)
    gx, gy = rng.integers(0, W, n), rng.integers(0, H, n)
    got = pl[gy, gx]
    truth = np.array([R.mp_iters(*R.pixel_c(centre, (scale, scale), W, H, x, y, 2 * bits), M, 2 * bits) for x, y in zip(gx, gy)])
    return L, got, truth


def test_quality_against_direct_high_precision(B, boundary_views):
    views = [(K4, 1e-10, 3000)] + boundary_views
    escaping = 0
    for centre, scale, M in views:
        L, got, truth = sampled_quality(B, centre, scale, M)
        escaping += L < M
        assert (got == truth).mean() >= 0.99, (centre, scale, int((got != truth).sum()))
        assert len(np.unique(truth)) >= (10 if scale <= 1e-50 else 20), (scale, len(np.unique(truth)))
    assert escaping >= 1


def test_the_gap_it_closes(B, boundary_views):
    """At 1e-20, F64's per-column c (its view words are doubles) takes at most two values across 64 columns; perturbation resolves the view."""
    centre, scale, M = boundary_views[0]
    cxv, cyv, sxv, syv = F.view_words((float(centre[0]), float(centre[1])), (scale, scale))
    assert len(np.unique(F.c_axis(64, cxv, sxv))) <= 2 and len(np.unique(F.c_axis(48, cyv, syv))) <= 2
    with B.Orbit(centre[0], centre[1], scale, scale, M) as o:
        pl = R.plane(o.table(), o.length, 64, 48, M, (scale, scale))
    assert len(np.unique(pl)) >= 20


def app(*args, cwd):
    return subprocess.run([os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "mandelbrot")] + list(args), capture_output=True,
                          text=True, cwd=cwd, timeout=60)


def test_app_accepts_perturb(B, tmp_path):
    """Parsed and run up to the device: without a GPU init() fails with the device message, with one the image is written."""
    r = app("--precision", "perturb", "--centre", "-0.7436438870371587047521915", "0.13182590420531197049", "--scale", "1e-30", "1e-30",
            "--width", "64", "--height", "48", "--max-iter", "100", "--quiet", cwd=tmp_path)
    assert "not one of" not in r.stdout
    assert (r.returncode == 0 and (tmp_path / "mandelbrot.png").exists()) or (r.returncode == 1 and "could not find a device" in r.stdout)


def test_app_refuses_a_malformed_centre_before_the_device(B, tmp_path):
    r = app("--precision", "perturb", "--centre", "-0.74x", "0.1", "--scale", "1e-30", "1e-30", cwd=tmp_path)
    assert r.returncode == 1 and "--centre -0.74x 0.1" in r.stdout and "could not find a device" not in r.stdout
    assert "using device" not in r.stdout and not list(tmp_path.iterdir())


def test_boundary_views_clear_the_escape_threshold(boundary_views):
    """The views above are chosen off the method's known failure: each centre's own escape clears |z|^2 = 2 by at least 1e-6."""
    for centre, scale, M in boundary_views:
        n, margin = R.escape_margin(centre[0], centre[1], M, 2 * R.orbit_bits(scale, scale))
        assert n < M and margin >= 1e-6, (scale, n, margin)


def test_reference_on_the_hair_is_the_documented_failure(B):
    """include/mc_compute.h: a reference orbit whose escape is within double rounding of |z|^2 = 2 has that comparison decided in
    double for every pixel that follows it.  Here |Z_L|^2 - 2 is about 4e-31: the centre pixel (dc = 0) runs to M instead of escaping
    at L - 1 as direct iteration does."""
    M = 4000
    c = R.mp_hair_point(("-0.5", "0"), ("-0.5", "1"), M, 220, 284)
    with B.Orbit(c[0], c[1], 1e-30, 1e-30, M) as o:
        Z, L, bits = o.table(), o.length, o.bits
    n, margin = R.escape_margin(c[0], c[1], M, 2 * bits)
    assert L == M and n == M - 1 and 0 < margin < 1e-20
    assert R.scalar_iters(Z.tolist(), L, 0.0, 0.0, M) == M
