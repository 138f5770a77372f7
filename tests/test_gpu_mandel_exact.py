"""mc_mandelbrot_exact_counts_device on the GPU (include/mc_compute.h: "exact counts").  Bit equality only:
device == host == the Python-integer restatement (tests/mandel_exact_ref.py), for both kernels, at every limb count where the code
takes another path, at the ends of the loop, across slice boundaries and batch sizes.  The agreement of the renders with the exact
counts is printed, not asserted."""
import os
import re
import subprocess

import numpy as np
import pytest

import mandel_exact_ref as X
import mandel_perturb_deep_ref as D
import mandel_perturb_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "mandelbrot")
W, H = 24, 16
ZERO = dict(centre=(0.0, 0.0), scale=(0.0, 0.0))
WAVE, GROUP = 1, 2


def lattice(count, w=W, h=H):
    """`count` pixels of the w x h view on a fixed lattice, the centre pixel first."""
    px = [(w // 2, h // 2)]
    for i in range(count - 1):
        px.append(((5 * i + 1) % w, (7 * i + 3) % h))
    return np.array(px, np.uint32)


def m33(exp2):
    """The Misiurewicz point M33 as text, accurate beyond the bits of a view of scale 2^exp2."""
    return D.misiurewicz(D.M33[0], D.M33[1], D.M33[2], 96 - exp2 + 64)


def three_ways(ctx, o, centre, M, dcx, dcy, e, extra=0):
    """device == host == Python reference; returns the counts."""
    dev = o.exact_counts(M, dcx, dcy, e, extra_limbs=extra, device=ctx)
    host = o.exact_counts(M, dcx, dcy, e, extra_limbs=extra)
    want = X.counts(centre, o.bits, dcx, dcy, e, M, extra_limbs=extra)
    assert dev.tolist() == host.tolist() == want, (dev.tolist(), want)
    return dev


def native_exp2(n):
    """A scale 2^E whose orbit has n limbs: bits = 96 - E."""
    return {131: -8192, 16: -850, 17: -900}.get(n, 96 - 64 * (n - 1) + 10)


@pytest.mark.parametrize("n", [2, 3, 8, 15, 16, 17, 18, 55, 131])
def test_limb_counts(ctx, B, n):
    """Each n two ways.  A spread of counts: the 24 x 16 view of scale 2^-100 around M33 (5 limbs; counts from 138 up) raised to n limbs
    by extra_limbs, so every product runs at full length on numbers whose low limbs are full; n = 3: the same point at 2^-20; n = 2: a
    grid over the whole set from an orbit at centre 0 of scale 2^33.  And the native depth: the view of the scale that gives n limbs
    around 1 + i, where |c|^2 = 2 exactly at the centre pixel and the offsets' lowest bits decide between n = 0 and n = 1."""
    M = 200 if n == 131 else 500
    kind = WAVE if n <= 16 else GROUP
    if n == 2:
        o = B.Orbit("0", "0", 1.0, 1.0, M, 33)
        centre = ("0", "0")
        g = np.arange(48)
        dcx, dcy, e, extra = -2.0 + (g % 8) * (2.5 / 8), -1.0 + (g // 8) * (2.0 / 6) + 1.0 / 64, 0, 0
    elif n == 3:
        centre = m33(-20)
        o = B.Orbit(centre[0], centre[1], 1.0, 1.0, M, -20)
        dcx, dcy, e = o.exact_pixel_offsets(W, H, lattice(48))
        extra = 0
    else:
        centre = m33(-100)
        o = B.Orbit(centre[0], centre[1], 1.0, 1.0, M, -100)
        dcx, dcy, e = o.exact_pixel_offsets(W, H, lattice(48))
        extra = n - 5
    with o:
        assert X.limbs_of(o.bits, extra) == n
        got = three_ways(ctx, o, centre, M, dcx, dcy, e, extra)
        assert len(set(got.tolist())) >= 8
        _, _, limbs, _, k = ctx.last_exact_timing()
        assert (limbs, k) == (n, kind)
    if n == 2:
        return
    E = native_exp2(n)
    with B.Orbit("1", "1", 1.0, 1.0, M, E) as o:
        assert X.limbs_of(o.bits) == n
        dcx, dcy, e = o.exact_pixel_offsets(W, H, lattice(48))
        got = three_ways(ctx, o, ("1", "1"), M, dcx, dcy, e)
        assert set(got.tolist()) == {0, 1} and got[0] == 1
        _, _, limbs, _, k = ctx.last_exact_timing()
        assert (limbs, k) == (n, kind)


def test_extra_limb_crosses_from_the_wave_kernel_to_the_workgroup_kernel(ctx, B):
    centre = m33(-850)
    with B.Orbit(centre[0], centre[1], 1.0, 1.0, 500, -850) as o:
        dcx, dcy, e = o.exact_pixel_offsets(W, H, lattice(48))
        a = three_ways(ctx, o, centre, 500, dcx, dcy, e)
        assert ctx.last_exact_timing()[2:] == (16, ctx.last_exact_timing()[3], WAVE)
        b = three_ways(ctx, o, centre, 500, dcx, dcy, e, extra=1)
        assert ctx.last_exact_timing()[2] == 17 and ctx.last_exact_timing()[4] == GROUP
        print(f"\n2^-850 view, 16 against 17 limbs: {int((a != b).sum())} of 48 counts differ")


@pytest.mark.parametrize("extra", [0, 14], ids=["wave", "workgroup"])
def test_ends(ctx, B, extra):
    """|c|^2 > 2 (n = 0), n = 1, interior pixels (n = M), and M = 1, on 3 and on 17 limbs."""
    with B.Orbit("0", "0", 1e-8, 1e-8, 10) as o:
        dcx = np.array([1.5, 1.0, 0.0, -1.0, -0.125, 1.0, -2.0, 0.25])
        dcy = np.array([0.0, 1.0, 0.0, 0.0, 0.0, 1.0 + 2.0 ** -50, 0.0, 0.5])
        for M in (1, 2, 300):
            got = three_ways(ctx, o, ("0", "0"), M, dcx, dcy, 0, extra)
            assert got[0] == 0 and got[1] == min(M, 1) and got[2] == got[3] == got[4] == M and got[5] == 0
        assert ctx.last_exact_timing()[2] == 3 + extra


def real_axis_c_with_count(bits, extra, target):
    """delta (a double) with the exact count of c = 0.25 + delta equal to `target`: the count falls as delta grows (about pi / sqrt(delta)),
    so bisection on the double finds every value."""
    rx, F = X.parse_centre("0.25", bits), 64 * (X.limbs_of(bits, extra) - 1)
    n_of = lambda d: X.count(X.pixel_c(rx, bits, extra, d, 0), 0, F, target + 2)
    f32 = lambda v: float(np.float32(v))       # few mantissa bits: exact on any limb count used here
    guess = (np.pi / (target + 1.0)) ** 2
    lo, hi = f32(guess / 2.0), f32(guess * 2.0)   # n_of(lo) > target >= n_of(hi)
    if target < 16 or not n_of(lo) > target >= n_of(hi):
        lo, hi = 2.0 ** -40, 1.0
        assert n_of(lo) > target >= n_of(hi)
    for _ in range(200):
        mid = f32((lo + hi) / 2)
        if mid in (lo, hi):
            break
        v = n_of(mid)
        if v == target:
            return mid
        if v > target:
            lo = mid
        else:
            hi = mid
    raise AssertionError(f"no real-axis c with count {target}")


@pytest.mark.parametrize("extra", [0, 128], ids=["wave 3 limbs", "workgroup 131 limbs"])
def test_slices(ctx, B, extra):
    """M = I, I + 1 and 2 I + 1 for the slice length I the call reports, and escapes placed on the boundary between the first launch and
    the second.  The wave kernel tests z_(j+1) at the end of iteration j: n = I - 1 is found in the last iteration of the first launch,
    n = I in the first of the second.  The workgroup kernel tests z_j at the start of iteration j: n = I - 2 is found in the last
    iteration of the first launch, n = I - 1 in the first of the second.  Both kernels get I - 2, I - 1 and I, beside an immediate escape
    and an interior point, so the pixels of one call finish in different launches."""
    with B.Orbit("0.25", "0", 1e-8, 1e-8, 10) as o:
        n = 3 + extra
        probe = o.exact_counts(1, [0.0] * 5, [0.0] * 5, extra_limbs=extra, device=ctx)
        assert probe.tolist() == [1] * 5
        _, launches, limbs, I, kind = ctx.last_exact_timing()
        assert (limbs, kind) == (n, WAVE if n <= 16 else GROUP) and I >= 3
        edge = [real_axis_c_with_count(o.bits, extra, t) for t in (I - 2, I - 1, I)]
        dcx = np.array(edge + [1.5, -0.25])   # ... an immediate escape (c = 1.75) and an interior point (c = 0)
        dcy = np.zeros(5)
        for M in (I, I + 1, 2 * I + 1):
            dev = o.exact_counts(M, dcx, dcy, extra_limbs=extra, device=ctx)
            assert dev.tolist() == [I - 2, I - 1, I, 0, M]
            assert dev.tolist() == o.exact_counts(M, dcx, dcy, extra_limbs=extra).tolist()
            _, launches, _, I2, _ = ctx.last_exact_timing()
            # the interior pixel runs M iterations; the workgroup kernel then needs the start of one more for the test of z_M
            assert I2 == I and launches == ((M + I - 1) // I if kind == WAVE else M // I + 1)


@pytest.mark.parametrize("count", [1, 63, 64, 65])
def test_wave_kernel_batches(ctx, B, count):
    centre = m33(-20)
    with B.Orbit(centre[0], centre[1], 1.0, 1.0, 300, -20) as o:
        px = lattice(count)[::-1].copy()                        # unordered ...
        px[count // 2] = px[0]                                  # ... and with a duplicate
        px[count // 3] = px[count - 1]
        dcx, dcy, e = o.exact_pixel_offsets(W, H, px)
        three_ways(ctx, o, centre, 300, dcx, dcy, e)
        assert ctx.last_exact_timing()[4] == WAVE


def test_workgroup_kernel_batches(ctx, B):
    """1, CUs, CUs + 1 and 2 CUs + 1 pixels at 17 limbs: the slice shortens with the rounds the grid needs."""
    cus = ctx.device_info()[1]
    centre = m33(-100)
    with B.Orbit(centre[0], centre[1], 1.0, 1.0, 300, -100) as o:
        big = lattice(2 * cus + 1, 48, 32)[::-1]
        dcx, dcy, e = o.exact_pixel_offsets(48, 32, big)
        want = np.array(X.counts(centre, o.bits, dcx, dcy, e, 300, extra_limbs=12), np.uint32)
        assert np.array_equal(o.exact_counts(300, dcx, dcy, e, extra_limbs=12), want)
        slices = []
        for count in (1, cus, cus + 1, 2 * cus + 1):
            dev = o.exact_counts(300, dcx[:count], dcy[:count], e, extra_limbs=12, device=ctx)
            assert np.array_equal(dev, want[:count]), count
            _, _, limbs, I, kind = ctx.last_exact_timing()
            assert (limbs, kind) == (17, GROUP)
            slices.append(I)
        # kOrbitLaunchWork / 17^2 (csrc/mandel_perturb.h) over the rounds at one workgroup per CU, clamped to [1, 65536]
        assert slices == [min(65536, max(1, 32_000_000 // 289 // r)) for r in (1, 1, 2, 3)]


def test_timing_is_refused_before_the_first_call(B):
    with B.Context(0) as c:
        with pytest.raises(B.McError) as ei:
            c.last_exact_timing()
        assert ei.value.status == 1
        with B.Orbit("0", "0", 1e-8, 1e-8, 10) as o:
            with pytest.raises(B.McError):                      # a refused call leaves it refused
                o.exact_counts(0, [0.0], [0.0], device=c)
            with pytest.raises(B.McError):
                c.last_exact_timing()
            assert o.exact_counts(7, [0.0], [0.0], device=c).tolist() == [7]
            ms, launches, limbs, I, kind = c.last_exact_timing()
            assert ms >= 0.0 and launches == 1 and limbs == 3 and I >= 7 and kind == WAVE


def test_reference_on_the_hair_is_caught(B):
    """The view of test_reference_on_the_hair_is_the_documented_failure: the PERTURB render says M at the centre pixel, whose exact count
    is L - 1."""
    M, w, h = 4000, 24, 16
    c = R.mp_hair_point(("-0.5", "0"), ("-0.5", "1"), M, 220, 284)
    with B.Context(0) as cx, B.Orbit(c[0], c[1], 1e-30, 1e-30, M) as o:
        assert o.length == M
        cx.bind_mandelbrot_orbit(o)
        _, it = cx.mandelbrot(B.mandelbrot_params(w, h, max_iter=M, precision=B.PRECISION_PERTURB, **ZERO), want_rgba=False)
        exact = cx.exact_counts(o, w, h, [(w // 2, h // 2)], M)
        assert exact.tolist() == [o.length - 1] == cx.exact_counts(o, w, h, [(w // 2, h // 2)], M, device=False).tolist()
        assert int(it[h // 2, w // 2]) == M


def test_agreement_of_the_renders_is_printed(B, capsys):
    """All 1536 pixels of the 48 x 32 view of test_rescaled_orbit_renders_the_restatement (M33, (1, 0.75) * 2^-100, M = 2000) under
    PERTURB and PERTURB_BLA against their exact counts, and extra_limbs 0 against 2.  Printed, not asserted."""
    w, h, M = 48, 32, 2000
    c, _, _ = D.view(D.M33, "1e-60")
    px = np.array([(x, y) for y in range(h) for x in range(w)], np.uint32)
    lines = []
    with B.Context(0) as cx, B.Orbit(c[0], c[1], 1.0, 0.75, M, -100) as o:
        e0 = cx.exact_counts(o, w, h, px, M).reshape(h, w)
        e2 = cx.exact_counts(o, w, h, px, M, extra_limbs=2).reshape(h, w)
        lines.append(f"extra_limbs 0 against 2: {int((e0 == e2).sum())} of {w * h} equal")
        for name, precision, tables in (("PERTURB", B.PRECISION_PERTURB, 0), ("PERTURB_BLA", B.PRECISION_PERTURB_BLA, B.ORBIT_TABLE_BLA)):
            cx.bind_mandelbrot_orbit(o, device_tables=tables)
            _, it = cx.mandelbrot(B.mandelbrot_params(w, h, max_iter=M, precision=precision, **ZERO), want_rgba=False)
            lines.append(f"{name}: {int((it == e0).sum())} of {w * h} pixels equal their exact count "
                         f"(largest difference {int(np.abs(it.astype(np.int64) - e0).max())})")
        assert e0.shape == e2.shape == it.shape
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_app_exact_check(tmp_path):
    c = R.mp_boundary_point(("-0.5", "0"), ("-0.5", "1"), 4000, 70, 134)
    cmd = [APP, "--width", "64", "--height", "48", "--max-iter", "4000", "--precision", "perturb", "--centre", c[0], c[1], "--scale", "1e-20",
           "1e-20", "--quiet", "--exact-check", "64", "--out", str(tmp_path / "a.png")]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    at = [i for i, s in enumerate(out) if s.startswith("exact check: ")]
    assert len(at) == 1, r.stdout
    m = re.fullmatch(r"exact check: (\d+) of 64 equal \(limbs (\d+), [0-9.]+ ms\)", out[at[0]])
    assert m and int(m.group(2)) == 4, out[at[0]]
    shown = [s for s in out[at[0] + 1:] if re.fullmatch(r"  pixel \(\d+, \d+\): render \d+, exact \d+", s)]
    assert len(shown) == min(64 - int(m.group(1)), 8), r.stdout   # the first few mismatches: at most 8 lines
    r2 = subprocess.run(cmd + ["--exact-extra-limbs", "13"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r2.returncode == 0 and "(limbs 17," in r2.stdout, r2.stdout + r2.stderr
