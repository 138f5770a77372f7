"""Atom domains without a GPU (include/mc_compute.h: "atom domains"): mc_mandelbrot_atom_scan (the update the kernels compile) and the host
domains against tests/mandel_atom_ref.py; mc_mandelbrot_nucleus_refine bit for bit against the Python-float restatement and, for accuracy,
against mpmath's nuclei; mc_mandelbrot_orbit_offset_text against Python Fractions and round its trip through the orbit constructor; every
refusal with its status and text."""
import math
import struct

import mpmath
import numpy as np
import pytest

import mandel_atom_ref as A
from mandel_atom_cases import SYNTHETIC, nucleus3, refused
import mandel_f64_ref as F

INVALID, UNSUPPORTED = 1, 5
REF_VIEW = ((-0.5, 0.0), (3.0, 2.25))   # the reference view
W, H, M = 64, 48, 200


def bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


# ---- the scan ---------------------------------------------------------------------------------------------------------------------------
def orbit_of(cx, cy, n):
    z, out = (0.0, 0.0), []
    for _ in range(n):
        z = ((z[0] * z[0] - z[1] * z[1]) + cx, ((2.0 * z[0]) * z[1]) + cy)
        out.append(z)
    return out


nan, inf = math.nan, math.inf
CRAFTED = {
    "empty": [],
    "one": [(0.25, -0.5)],
    "ties keep the first": [(0.5, 0.1), (0.1, -0.5), (-0.5, 0.5), (0.5, 0.5)],
    "tie after a smaller": [(0.5, 0.0), (0.25, 0.25), (0.25, 0.0), (0.0, 0.25)],
    "c = 0: zero at m = 1": orbit_of(0.0, 0.0, 8),
    "c = -1: zero at m = 2, not 4": orbit_of(-1.0, 0.0, 8),
    "nan never updates": [(nan, 0.0), (0.0, nan), (nan, nan), (0.75, 0.5)],
    "only nans": [(nan, 1.0), (1.0, nan)],
    "inf entries": [(inf, 0.0), (-inf, 0.5), (0.5, -inf), (3.0, -4.0), (inf, inf)],
    "only inf": [(inf, -inf)],
    "minus zero": [(1.0, 1.0), (-0.0, -0.0), (0.0, 0.0)],
    "minus zero part": [(-0.0, 0.5), (0.5, -0.0)],
    "subnormal": [(5e-324, -5e-324), (0.0, 5e-324), (0.0, 0.0)],
}


@pytest.mark.parametrize("name", list(CRAFTED))
def test_scan_on_crafted_sequences(B, name):
    z = CRAFTED[name]
    per, best = B.atom_scan(np.array(z, np.float64).reshape(-1, 2))
    rper, rbest = A.scan(z)
    assert per == rper and bits(best) == bits(rbest), (per, best, rper, rbest)
    if name == "c = 0: zero at m = 1":
        assert (per, best) == (1, 0.0)
    if name == "c = -1: zero at m = 2, not 4":
        assert (per, best) == (2, 0.0)
    if name in ("empty", "only nans", "only inf"):
        assert (per, best) == (0, inf)
    if name == "minus zero":
        assert per == 2 and bits(best) == 0   # |-0| = +0


def test_scan_on_random_sequences(B):
    rng = np.random.default_rng(20250)
    for trial in range(200):
        n = int(rng.integers(0, 40))
        z = rng.standard_normal((n, 2)) * 10.0 ** rng.integers(-300, 300, (n, 1)).astype(np.float64)
        if n and trial % 3 == 0:
            z[rng.integers(0, n)] = z[rng.integers(0, n)]                  # a tie
        if n and trial % 5 == 0:
            z[rng.integers(0, n), rng.integers(0, 2)] = rng.choice([nan, inf, -inf, -0.0, 0.0])
        per, best = B.atom_scan(z)
        rper, rbest = A.scan(z.tolist())
        assert per == rper and bits(best) == bits(rbest), (trial, per, best, rper, rbest)


def test_scan_refuses_null_outputs(B):
    import ctypes as C
    z = np.zeros((1, 2))
    per, best = C.c_uint32(0), C.c_double(0)
    assert B.lib().mc_mandelbrot_atom_scan(z.ctypes.data, 1, None, C.byref(best)) == INVALID
    assert B.lib().mc_mandelbrot_atom_scan(z.ctypes.data, 1, C.byref(per), None) == INVALID
    assert B.lib().mc_mandelbrot_atom_scan(None, 1, C.byref(per), C.byref(best)) == INVALID
    assert B.lib().mc_mandelbrot_atom_scan(None, 0, C.byref(per), C.byref(best)) == 0


# ---- the host domains -------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(SYNTHETIC))
def test_host_domains_against_numpy(B, name):
    per, am, mi = SYNTHETIC[name]
    count, tab, pixel = B.atom_domains(per, am, mi)
    rc, rt, rp = A.domains(per, am, mi)
    assert np.array_equal(count, rc)
    assert np.array_equal(tab.view(np.uint64), rt.view(np.uint64))
    assert np.array_equal(pixel, rp)
    assert int(count.sum()) == per.size
    if name == "equal minima":
        for v in range(1, 6):
            assert pixel[v] == np.nonzero((per == v) & (am == tab[v]))[0][0]
    if name == "all +inf":
        assert pixel[2] == 0 and tab[2] == np.inf and pixel[1] == A.NO_PIXEL and count[1] == 0


def test_host_domains_refusals(B):
    per, am = np.array([1, 9, 2], np.uint32), np.zeros(3)
    with refused(B, INVALID, "pixel 1", "period 9", "above max_iter"):
        B.atom_domains(per, am, 8)
    import ctypes as C
    out = np.zeros(4, np.uint32)
    assert B.lib().mc_mandelbrot_atom_domains(None, am.ctypes.data, 3, 8, out.ctypes.data, am.ctypes.data, out.ctypes.data) == INVALID
    assert B.lib().mc_mandelbrot_atom_domains(per.ctypes.data, am.ctypes.data, 1 << 32, 8, out.ctypes.data, am.ctypes.data, out.ctypes.data) == INVALID
    count, tab, pixel = B.atom_domains(np.zeros(0, np.uint32), np.zeros(0), 2)     # no pixel: the empty tables
    assert count.tolist() == [0, 0, 0] and np.all(tab == np.inf) and pixel.tolist() == [A.NO_PIXEL] * 3


# ---- Newton ---------------------------------------------------------------------------------------------------------------------------
def mp_newton(p, cx, cy, dps):
    """The zero of z_p nearest (cx, cy) (mpf or text), by mpmath's own Newton iteration at `dps` digits."""
    with mpmath.workdps(dps):
        c = mpmath.mpc(mpmath.mpf(cx), mpmath.mpf(cy))
        for _ in range(200):
            z, d = mpmath.mpc(0), mpmath.mpc(0)
            for _ in range(p):
                d = 2 * z * d + 1
                z = z * z + c
            step = z / d
            c = c - step
            if abs(step) < mpmath.mpf(10) ** -(dps - 10):
                break
        return c


@pytest.fixture(scope="module")
def ref_view_starts():
    """The reference view's F64 atom planes by the restatement, their domains, and the best pixel's c for periods 1, 2, 3, 5."""
    cxv, cyv, sxv, syv = F.view_words(*REF_VIEW)
    cx, cy = F.c_axis(W, cxv, sxv), F.c_axis(H, cyv, syv)
    CX, CY = np.broadcast_to(cx[None, :], (H, W)), np.broadcast_to(cy[:, None], (H, W))
    n, period, amin = A.direct_planes(CX, CY, M, np.float64)
    count, tab, pixel = A.domains(period, amin, M)
    starts = {}
    for p in (1, 2, 3, 5):
        assert count[p] > 0
        gy, gx = divmod(int(pixel[p]), W)
        starts[p] = (float(cx[gx]), float(cy[gy]))
    return starts


@pytest.fixture(scope="module")
def zero_orbit(B):
    with B.Orbit("0", "0", REF_VIEW[1][0], REF_VIEW[1][1], M) as o:
        yield o, o.table()


def deep_cases(B):
    """(orbit, table, scale, [(start offsets)]) at mpmath's period-3 nucleus, scales 1e-30 and 1e-250: Smith's branch matters there (|D|^2
    of the naive form overflows at 1e-250)."""
    for scale, digits in ((1e-30, 80), (1e-250, 330)):
        centre = nucleus3(digits)
        o = B.Orbit(centre[0], centre[1], scale, scale * 0.75, 300)
        px = scale / 48.0
        starts = [(3.0 * px, -2.0 * px), (-5.0 * px, 1.0 * px), (0.5 * px, 7.0 * px), (0.0, 0.0)]
        yield o, o.table(), scale, centre, starts


def test_refine_bit_for_bit_on_the_zero_centre_orbit(B, zero_orbit, ref_view_starts):
    o, Z = zero_orbit
    for p, start in ref_view_starts.items():
        got = o.nucleus_refine(p, start, 64)
        want = A.refine(Z, o.length, p, start, 64)
        assert want is not None
        assert [bits(v) for v in got[0]] == [bits(v) for v in want[0]], (p, got, want)
        assert got[1] == want[1] and [bits(v) for v in got[2]] == [bits(v) for v in want[2]], (p, got, want)
        assert got[1] < 64                                                       # converged, not stopped
        # one step at a time is the same sequence
        one = o.nucleus_refine(p, start, 1)
        assert one[1] == 1 and [bits(v) for v in one[0]] == [bits(v) for v in A.refine(Z, o.length, p, start, 1)[0]]


def test_refine_bit_for_bit_at_the_period_3_nucleus(B):
    for o, Z, scale, centre, starts in deep_cases(B):
        with o:
            for p in (3, 6):
                for start in starts:
                    want = A.refine(Z, o.length, p, start, 40)
                    if want is None:
                        with refused(B, UNSUPPORTED, "step"):
                            o.nucleus_refine(p, start, 40)
                        continue
                    got = o.nucleus_refine(p, start, 40)
                    assert [bits(v) for v in got[0]] == [bits(v) for v in want[0]], (scale, p, start, got, want)
                    assert got[1] == want[1] and [bits(v) for v in got[2]] == [bits(v) for v in want[2]]


# |refined - true| / scale, measured on the CPU over the cases of the test below (DESIGN.md section 3.33 lists them): the largest is
# 5.52e-18 (period 5 of the reference view, scale 2.25; periods 1 and 2 land on 0 and -1 exactly, period 3 measures 1.73e-18, the 1e-30
# cases 1.42e-47 and the 1e-250 cases 1.7e-39).  The arithmetic is fixed, so the figure does not move with the platform; the factor 16 is
# room for start pixels a later test adds, not for noise.
ERR_MEASURED = 5.52e-18
ERR_BOUND = 16 * ERR_MEASURED


def test_refine_reaches_mpmaths_nucleus(B, zero_orbit, ref_view_starts):
    o, _ = zero_orbit
    worst = 0.0
    for p, start in ref_view_starts.items():
        (ox, oy), steps, _ = o.nucleus_refine(p, start, 64)
        true = mp_newton(p, ox, oy, 60)
        with mpmath.workdps(60):
            err = float(max(abs(mpmath.mpf(ox) - true.real), abs(mpmath.mpf(oy) - true.imag)) / min(REF_VIEW[1]))
        print(f"reference view, period {p}: start {start} -> ({ox!r}, {oy!r}) in {steps} steps, |refined - true| / scale = {err:.3g}")
        worst = max(worst, err)
        assert err <= ERR_BOUND
    assert abs(o.nucleus_refine(1, ref_view_starts[1])[0][0]) <= ERR_BOUND * 2.25
    (x2, y2), _, _ = o.nucleus_refine(2, ref_view_starts[2])
    assert abs(x2 + 1.0) <= ERR_BOUND * 2.25 and abs(y2) <= ERR_BOUND * 2.25
    (x3, y3), _, _ = o.nucleus_refine(3, ref_view_starts[3])
    assert abs(x3 - -0.12256116687665362) < 1e-15 and abs(abs(y3) - 0.7448617666197442) < 1e-15
    for orb, Z, scale, centre, starts in deep_cases(B):
        with orb:
            dps = 400
            true = mp_newton(3, centre[0], centre[1], dps)
            for start in starts:
                (ox, oy), steps, _ = orb.nucleus_refine(3, start, 40)
                with mpmath.workdps(dps):
                    tx, ty = true.real - mpmath.mpf(centre[0]), true.imag - mpmath.mpf(centre[1])
                    err = float(max(abs(mpmath.mpf(ox) - tx), abs(mpmath.mpf(oy) - ty)) / mpmath.mpf(scale * 0.75))
                print(f"period-3 nucleus at {scale:g}: start {start} -> ({ox!r}, {oy!r}) in {steps} steps, |refined - true| / scale = {err:.3g}")
                worst = max(worst, err)
                assert steps < 40 and err <= ERR_BOUND
    print(f"largest |refined - true| / scale: {worst:.3g}")


def test_refine_refusals(B, zero_orbit):
    o, _ = zero_orbit
    with refused(B, INVALID, "mc_mandelbrot_nucleus_refine", "period must be at least 1"):
        o.nucleus_refine(0, (0.1, 0.1))
    with refused(B, INVALID, "period above the orbit's max_iter"):
        o.nucleus_refine(M + 1, (0.1, 0.1))
    with refused(B, INVALID, "max_steps must be at least 1"):
        o.nucleus_refine(2, (0.1, 0.1), max_steps=0)
    with refused(B, INVALID, "not finite"):
        o.nucleus_refine(2, (math.inf, 0.1))
    with refused(B, UNSUPPORTED, "step 1", "not finite"):     # period 1 from c = 0 exactly: z_1 = c, D = 1: fine; period 2 from -0.5: D = 2c + 1 = 0
        o.nucleus_refine(2, (-0.5, 0.0))
    with B.Orbit("-0.75", "0.1", 1.0, 1.0, 50, -1100) as deep:
        assert deep.deep
        with refused(B, INVALID, "deep orbit"):
            deep.nucleus_refine(2, (0.0, 0.0))
    import ctypes as C
    off, last, steps = np.zeros(2), np.zeros(2), C.c_uint32(0)
    L = B.lib()
    assert L.mc_mandelbrot_nucleus_refine(None, 1, 1, off.ctypes.data, C.byref(steps), last.ctypes.data) == INVALID
    assert L.mc_mandelbrot_nucleus_refine(o._h, 1, 1, None, C.byref(steps), last.ctypes.data) == INVALID
    assert L.mc_mandelbrot_nucleus_refine(o._h, 1, 1, off.ctypes.data, None, last.ctypes.data) == INVALID
    assert L.mc_mandelbrot_nucleus_refine(o._h, 1, 1, off.ctypes.data, C.byref(steps), None) == INVALID


# ---- the centre as text -------------------------------------------------------------------------------------------------------------
TEXT_CASES = [
    # (centre, scale, exp2 or None, M, (ox, oy), frac_digits)
    (("-0.7436438870371587", "0.13182590420531198"), (1e-8, 1e-8), None, 50, (1.25e-9, -3.5e-9), 60),
    (("-0.7436438870371587", "0.13182590420531198"), (1e-8, 1e-8), None, 50, (2.0 ** -300, -(2.0 ** -400) * 3), 140),   # bits below the stored limbs
    (("0.1", "-0.1"), (1e-3, 1e-3), None, 20, (-0.25, 0.35), 30),                                                         # the signs flip
    (("0.9999999999", "-0.9999999999"), (1e-3, 1e-3), None, 20, (1e-9, -1e-9), 40),                                       # a carry into the integer limb
    (("0", "0"), (3.0, 2.25), None, 20, (-0.12256116687665362, -0.7448617666197442), 25),
    (("0", "0"), (3.0, 2.25), None, 20, (0.0, -0.0), 5),
    (("0.25", "-0.5"), (1.0, 1.0), None, 20, (1.5, -1.25), 0),                                                            # no fractional digit
    (("-0.75", "0.1"), (1.0, 0.75), -1100, 20, (0.375, -0.4375), 400),                                                    # a deep orbit: units of 2^E
    (("-0.75", "0.1"), (1.0, 0.75), -1100, 20, (2.0 ** -60, 1.0 + 2.0 ** -52), 40),                                       # ... truncated far above the offset
]


@pytest.mark.parametrize("case", range(len(TEXT_CASES)))
def test_offset_text_against_fractions(B, case):
    centre, scale, E, mi, (ox, oy), digits = TEXT_CASES[case]
    with B.Orbit(centre[0], centre[1], scale[0], scale[1], mi, E) as o:
        got = o.offset_text(ox, oy, digits)
        want = A.offset_text(centre, o.bits, ox, oy, digits, o.scale_exp2 if o.deep else 0)
        assert got == want
        need = max(len(want[0]), len(want[1])) + 1
        assert o.offset_text(ox, oy, digits, capacity=need) == want                 # exactly enough
        with refused(B, INVALID, "mc_mandelbrot_orbit_offset_text", f"{need} bytes needed"):
            o.offset_text(ox, oy, digits, capacity=need - 1)                         # one byte short


def test_offset_text_refusals(B):
    with B.Orbit("0.1", "0.2", 1e-3, 1e-3, 10) as o:
        with refused(B, INVALID, "not finite"):
            o.offset_text(math.nan, 0.0, 10)
        with refused(B, INVALID, "frac_digits"):
            o.offset_text(0.0, 0.0, 1000001)
        buf = bytearray(8)
        import ctypes as C
        assert B.lib().mc_mandelbrot_orbit_offset_text(None, 0.0, 0.0, 3, C.create_string_buffer(8), C.create_string_buffer(8), 8) == INVALID
        assert B.lib().mc_mandelbrot_orbit_offset_text(o._h, 0.0, 0.0, 3, None, C.create_string_buffer(8), 8) == INVALID


def test_offset_text_round_trip_through_the_constructor(B):
    """Refine at 1e-30, write the centre, make an orbit there at a scale 2^40 smaller: Newton from offset 0 stays within that view."""
    scale = 1e-30
    centre = nucleus3(80)
    with B.Orbit(centre[0], centre[1], scale, scale, 300) as o:
        start = (3.0 * scale / 48.0, -2.0 * scale / 48.0)
        (ox, oy), steps, _ = o.nucleus_refine(3, start, 40)
        digits = math.ceil(-math.log10(scale)) + 20 + 13                           # the new scale's depth and 20 more
        tx, ty = o.offset_text(ox, oy, digits)
    small = math.ldexp(scale, -40)
    with B.Orbit(tx, ty, small, small, 300) as o2:
        (rx, ry), steps2, _ = o2.nucleus_refine(3, (0.0, 0.0), 40)
        assert steps2 < 40
        assert abs(rx) <= small / 2 and abs(ry) <= small / 2, (rx, ry, small)
