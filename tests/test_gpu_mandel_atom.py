"""Atom domains on the GPU (include/mc_compute.h: "atom domains"): the period plane of F32, F64 and PERTURB against the restatements of
tests/mandel_atom_ref.py bit for bit (which iterate every pixel to max_iter with no cycle exit), its count plane against the plain
render's, the device domains against the host's and numpy's, every refusal with its text, and the chain from a view to a dive's centre."""
import math
import os
import re
import subprocess

import mpmath
import numpy as np
import pytest

import mandel_atom_ref as A
import mandel_f64_ref as F
import mandel_perturb_deep_ref as D
import mandel_perturb_ref as R
from conftest import ROOT
from mandel_atom_cases import SYNTHETIC, nucleus3, refused

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 5
REF_VIEW = ((-0.5, 0.0), (3.0, 2.25))
K4_VIEW = ((-0.7436438870371587, 0.13182590420531198), (1e-8, 1e-8 * 2.0 / 3.0))
K4_TEXT = ("-0.7436438870371587", "0.13182590420531198")


@pytest.fixture(scope="module")
def actx(B):
    """A context of this module's own: the tests bind orbits to it."""
    c = B.Context(0)
    yield c
    c.close()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def direct_ref(view, W, H, M, f32):
    """The restated planes of an F32 / F64 view."""
    if f32:
        words = [F.split_double(v)[0] for v in (view[0][0], view[0][1], view[1][0], view[1][1])]
        cx, cy = A.f32_axis(W, words[0], words[2]), A.f32_axis(H, words[1], words[3])
        dt = np.float32
    else:
        cxv, cyv, sxv, syv = F.view_words(*view)
        cx, cy = F.c_axis(W, cxv, sxv), F.c_axis(H, cyv, syv)
        dt = np.float64
    return A.direct_planes(np.broadcast_to(cx[None, :], (H, W)), np.broadcast_to(cy[:, None], (H, W)), M, dt)


def perturb_p(B, W, H, M):
    return B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_PERTURB, centre=(0.0, 0.0), scale=(0.0, 0.0))


def check_planes(got, want, what):
    n, per, am = got
    rn, rper, ram = want
    assert np.array_equal(n, rn), f"{what}: n differs at {np.argwhere(n != rn)[:4].tolist()}"
    bad = np.argwhere(per != rper)
    assert bad.size == 0, f"{what}: period differs at {bad[:4].tolist()}: {per[tuple(bad[0])]} vs {rper[tuple(bad[0])]}"
    assert same_bits(am, ram), f"{what}: amin differs"


# ---- out_iters is the plain render's ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(67, 37), (1, 1)])
@pytest.mark.parametrize("prec", ["f32", "f64", "perturb"])
def test_count_plane_is_the_plain_renders(B, actx, prec, size):
    W, H = size
    for M in (1, 7, 8, 9, 17, 100):
        if prec == "perturb":
            with B.Orbit(K4_TEXT[0], K4_TEXT[1], 3.0, 2.25, M) as o:      # a wide view around K4's centre: a spread of counts
                actx.bind_mandelbrot_orbit(o)
            p = perturb_p(B, W, H, M)
        else:
            p = B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_F32 if prec == "f32" else B.PRECISION_F64, centre=REF_VIEW[0],
                                    scale=REF_VIEW[1])
        _, plain = actx.mandelbrot(p, want_rgba=False)
        n, per, am = actx.mandelbrot_atom(p)
        assert np.array_equal(n, plain), (prec, size, M)
        assert np.all(per <= n) and np.all((per == 0) == np.isinf(am)) and np.all(per[n == 0] == 0)
        only_n, none_p, none_a = actx.mandelbrot_atom(p, want_period=False, want_amin=False)     # any subset of the planes
        assert np.array_equal(only_n, plain) and none_p is None and none_a is None
        _, only_p, _ = actx.mandelbrot_atom(p, want_iters=False, want_amin=False)
        assert np.array_equal(only_p, per)
    actx.bind_mandelbrot_orbit(None)


# ---- period and amin, bit for bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["f32 reference view", "f64 reference view", "f64 k4", "f32 interior", "f64 interior", "f32 |c| to 8",
                                  "f64 |c| to 8"])
def test_direct_planes_equal_the_restatement(B, actx, case):
    f32 = case.startswith("f32")
    view, W, H, M = {"reference view": (REF_VIEW, 64, 48, 200), "k4": (K4_VIEW, 64, 48, 3000),
                     "interior": (((-0.1, 0.2), (0.01, 0.01)), 64, 48, 1000),          # every wave leaves by the cycle exit
                     "|c| to 8": (((0.0, 0.0), (16.0, 16.0)), 64, 48, 500)}[case[4:]]     # escaped lanes run on into inf and NaN
    p = B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_F32 if f32 else B.PRECISION_F64, centre=view[0], scale=view[1])
    got = actx.mandelbrot_atom(p)
    want = direct_ref(view, W, H, M, f32)
    check_planes(got, want, case)
    n, per, am = got
    if "interior" in case:
        assert np.all(n == M) and np.all(per >= 1)
    if "to 8" in case:
        assert (n == 0).any() and np.all(per[n == 0] == 0) and np.all(np.isinf(am[n == 0]))
    if case == "f64 reference view":
        assert len(np.unique(per)) > 20
    print(f"{case}: {len(np.unique(per))} distinct periods")


def perturb_case(B, name):
    W, H, M = 48, 32, 300
    if name == "nucleus3 1e-30":
        cx, cy = nucleus3(80)
        # a few pixels off the nucleus: the centre's text moved by 3 and 2 pixel pitches
        with mpmath.workdps(100):
            cx = mpmath.nstr(mpmath.mpf(cx) + mpmath.mpf(3e-30) / 48, 90, min_fixed=-math.inf, max_fixed=math.inf)
            cy = mpmath.nstr(mpmath.mpf(cy) - mpmath.mpf(2e-30) / 32, 90, min_fixed=-math.inf, max_fixed=math.inf)
        return (cx, cy), (1e-30, 1e-30 * 2 / 3), W, H, M
    centre = D.misiurewicz(D.M33[0], D.M33[1], D.M33[2], 100)      # 100 bits of a repelling orbit: it ends before M, the m == L rebase
    return centre, (1e-20, 1e-20 * 2 / 3), W, H, M


@pytest.mark.parametrize("name", ["nucleus3 1e-30", "misiurewicz 1e-20"])
def test_perturb_planes_equal_the_restatement(B, actx, name):
    centre, scale, W, H, M = perturb_case(B, name)
    with B.Orbit(centre[0], centre[1], scale[0], scale[1], M) as o:
        Z, L = o.table(), o.length
        actx.bind_mandelbrot_orbit(o)
    if name.startswith("misiurewicz"):
        assert L < M
    dcx, dcy = R.dc_axis(W, scale[0]), R.dc_axis(H, scale[1])
    want = A.perturb_planes(Z, L, np.broadcast_to(dcx[None, :], (H, W)), np.broadcast_to(dcy[:, None], (H, W)), M)
    got = actx.mandelbrot_atom(perturb_p(B, W, H, M))
    actx.bind_mandelbrot_orbit(None)
    check_planes(got, want, name)
    print(f"{name}: L = {L}, {len(np.unique(got[1]))} distinct periods, {int((got[0] == M).sum())} interior pixels")


# ---- the domains ----------------------------------------------------------------------------------------------------------------------
def device_domains(ctx, per, am, mi, guard=3):
    """The device tables of host planes, with `guard` words on either side of each table that must stay untouched."""
    import torch
    d_per = torch.from_numpy(np.ascontiguousarray(per, np.uint32).ravel().view(np.int32).copy()).cuda()
    d_am = torch.from_numpy(np.ascontiguousarray(am, np.float64).ravel().copy()).cuda()
    n = mi + 1
    count = torch.full((n + 2 * guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    tab = torch.full((n + 2 * guard,), -7.25, dtype=torch.float64, device="cuda")
    pixel = torch.full((n + 2 * guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.mandelbrot_atom_domains_device(d_per.data_ptr(), d_am.data_ptr(), d_per.numel(), mi, count[guard:].data_ptr(), tab[guard:].data_ptr(),
                                       pixel[guard:].data_ptr())
    ctx.synchronize()
    count, tab, pixel = count.cpu().numpy().view(np.uint32), tab.cpu().numpy(), pixel.cpu().numpy().view(np.uint32)
    for t, g in ((count, 0x5A5A5A5A), (tab, -7.25), (pixel, 0x5A5A5A5A)):
        assert np.all(t[:guard] == g) and np.all(t[-guard:] == g), "a table was written outside [0, max_iter]"
    return count[guard:-guard], tab[guard:-guard], pixel[guard:-guard]


def check_domains(B, ctx, per, am, mi, what):
    got = device_domains(ctx, per, am, mi)
    host = B.atom_domains(per, am, mi)
    ref = A.domains(per, am, mi)
    for g, h, r, name in zip(got, host, ref, ("count", "amin", "pixel")):
        if name == "amin":
            assert same_bits(g, h) and same_bits(g, r), f"{what}: {name}"
        else:
            assert np.array_equal(g, h) and np.array_equal(g, r), f"{what}: {name}"


@pytest.mark.parametrize("name", list(SYNTHETIC))
def test_device_domains_on_the_synthetic_planes(B, actx, name):
    per, am, mi = SYNTHETIC[name]
    check_domains(B, actx, per, am, mi, name)


def test_device_domains_on_rendered_and_large_planes(B, actx):
    for view, M in ((REF_VIEW, 200), (K4_VIEW, 3000)):
        p = B.mandelbrot_params(64, 48, max_iter=M, precision=B.PRECISION_F64, centre=view[0], scale=view[1])
        _, per, am = actx.mandelbrot_atom(p)
        check_domains(B, actx, per, am, M, f"rendered M = {M}")
    rng = np.random.default_rng(11)
    n = 257 * 130
    check_domains(B, actx, np.full(n, 17, np.uint32), rng.random(n), 40, "one period, 257 x 130")
    # past the grid cap (8 blocks of 256 lanes per CU): the kernels' loops repeat
    cus = actx.device_info()[1]
    n = cus * 8 * 256 + 70001
    per = rng.integers(0, 6, n).astype(np.uint32)
    per[n // 3: n // 3 + 100000] = 4                           # a flat stretch and a spread one
    am = rng.integers(1, 1 << 20, n).astype(np.float64) * 2.0 ** -20
    check_domains(B, actx, per, am, 5, f"past the cap: {n} pixels")
    # the device form ignores a period above max_iter (the host form refuses it); count[max_iter] takes the histogram's clamp
    per = np.array([1, 9, 2, 9, 3], np.uint32)
    am = np.array([0.5, 0.001, 0.25, 0.002, 0.125])
    count, tab, pixel = device_domains(actx, per, am, 3)
    assert count.tolist() == [0, 1, 1, 3] and pixel.tolist() == [A.NO_PIXEL, 0, 2, 4] and tab.tolist() == [np.inf, 0.5, 0.25, 0.125]


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(B, actx):
    W, H, M = 16, 8, 20
    ok = dict(max_iter=M, centre=REF_VIEW[0], scale=REF_VIEW[1])
    with refused(B, UNSUPPORTED, "mc_mandelbrot_render_atom", "MC_PRECISION_DS"):
        actx.mandelbrot_atom(B.mandelbrot_params(W, H, precision=B.PRECISION_DS, **ok))
    actx.bind_mandelbrot_orbit(None)
    with refused(B, INVALID, "MC_PRECISION_PERTURB", "no orbit bound"):
        actx.mandelbrot_atom(perturb_p(B, W, H, M))
    with B.Orbit(K4_TEXT[0], K4_TEXT[1], 1e-8, 1e-8, M) as o:
        o.bla()
        o.bla_deep()
        actx.bind_mandelbrot_orbit(o)
    for prec, name in ((B.PRECISION_PERTURB_BLA, "MC_PRECISION_PERTURB_BLA"), (B.PRECISION_PERTURB_BLA_DEEP, "MC_PRECISION_PERTURB_BLA_DEEP")):
        p = perturb_p(B, W, H, M)
        p.precision = prec
        with refused(B, UNSUPPORTED, name, "a skip does not visit its iterations"):
            actx.mandelbrot_atom(p)
    with refused(B, INVALID, "max_iter above the bound orbit's"):
        actx.mandelbrot_atom(perturb_p(B, W, H, M + 1))
    with B.Orbit(K4_TEXT[0], K4_TEXT[1], 1.0, 1.0, M, -1100) as o:
        assert o.deep
        actx.bind_mandelbrot_orbit(o)
    with refused(B, UNSUPPORTED, "the bound orbit is deep", "floatexp"):
        actx.mandelbrot_atom(perturb_p(B, W, H, M))
    actx.bind_mandelbrot_orbit(None)
    with refused(B, INVALID, "flags must be 0"):
        actx.mandelbrot_atom(B.mandelbrot_params(W, H, flags=B.MANDEL_ITERS_U16, **ok))
    with refused(B, INVALID, "flags must be 0"):
        actx.mandelbrot_atom(B.mandelbrot_params(W, H, flags=B.MANDEL_COLOUR_SMOOTH, **ok))
    with refused(B, INVALID, "the whole image only"):
        actx.mandelbrot_atom(B.mandelbrot_params(W, H, row_begin=0, row_end=4, **ok))
    with refused(B, INVALID, "the whole image only"):
        actx.mandelbrot_atom(B.mandelbrot_params(W, H, row_block=2, row_stride=4, **ok))
    with refused(B, INVALID, "all three outputs are NULL"):
        actx.mandelbrot_atom(B.mandelbrot_params(W, H, **ok), want_iters=False, want_period=False, want_amin=False)
    with refused(B, INVALID, "all three outputs are NULL"):
        actx.mandelbrot_atom_device(B.mandelbrot_params(W, H, **ok))
    with refused(B, INVALID, "max_iter must be nonzero"):
        actx.mandelbrot_atom(B.mandelbrot_params(W, H, max_iter=0))
    p = B.mandelbrot_params(W, H, **ok)                                       # and the context still renders
    n, per, am = actx.mandelbrot_atom(p)
    assert np.array_equal(n, actx.mandelbrot(p, want_rgba=False)[1])


# ---- the chain: from a view to a dive's centre ----------------------------------------------------------------------------------------
APP = os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "mandelbrot")
LINE = re.compile(r"  period (\d+): (\d+) pixels, best pixel \((\d+), (\d+)\) amin (\S+), Newton (\d+) steps( \(not converged\))? to pixel "
                  r"\((-?[0-9.e+]+), (-?[0-9.e+]+)\), (inside|outside view)(, = period (\d+))?: --centre (-?\d+\.\d+) (-?\d+\.\d+)")


def locate(tmp_path, *args):
    cmd = [APP, "--width", "64", "--height", "48", "--quiet", "--out", str(tmp_path / "a.png")] + list(args)
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    head = [s for s in out if s.startswith("locate: atom plane 64 x 48, ")]
    assert len(head) == 1, r.stdout
    rows = [s for s in out if s.startswith("  period ")]
    print("\n".join(head + rows))
    parsed = [LINE.fullmatch(s) for s in rows]
    assert rows and all(m or ", Newton failed: " in s for m, s in zip(parsed, rows)), r.stdout   # (a refused Newton run is reported, not fatal)
    return [m for m in parsed if m]


def test_locate_finds_a_nucleus_inside_k4s_view_and_the_dive_lands_on_it(B, actx, tmp_path):
    M = 3000
    rows = locate(tmp_path, "--precision", "f64", "--max-iter", str(M), "--centre", repr(K4_VIEW[0][0]), repr(K4_VIEW[0][1]), "--scale",
                  repr(K4_VIEW[1][0]), repr(K4_VIEW[1][1]), "--locate")
    assert len(rows) <= 8
    counts = [int(m.group(2)) for m in rows]
    assert counts == sorted(counts, reverse=True)                                   # the largest domains first
    inside = [m for m in rows if m.group(10) == "inside" and not m.group(7)]
    assert inside, "no line says inside"
    m = inside[0]
    p, amin1, cx, cy = int(m.group(1)), float(m.group(5)), m.group(13), m.group(14)
    # ceil(-log10(min scale)) + 20 fractional digits: the smaller scale is the vertical one, 6.67e-9
    assert len(cx.split(".")[1]) == len(cy.split(".")[1]) == math.ceil(-math.log10(min(K4_VIEW[1]))) + 20 == 29
    print(f"the dive: period {p} (printed, not pinned), amin {amin1}, centre {cx} {cy}")
    # a PERTURB render recentred on the printed centre at a scale 2^20 smaller: that period at the centre pixel, a smaller amin.
    # max_iter stays below 2 p: at a nucleus z_2p, z_3p, ... are as close to 0 as z_p is, and which of them is smallest in double is
    # rounding; the contract's period is the index of the minimum, so the multiples are kept out of the loop.
    W, H, M2 = 48, 32, min(M, 2 * p - 1)
    sx, sy = math.ldexp(K4_VIEW[1][0], -20), math.ldexp(K4_VIEW[1][1], -20)
    with B.Orbit(cx, cy, sx, sy, M2) as o:
        actx.bind_mandelbrot_orbit(o)
    n, per, am = actx.mandelbrot_atom(perturb_p(B, W, H, M2))
    actx.bind_mandelbrot_orbit(None)
    print(f"recentred: centre pixel n {n[H // 2, W // 2]}, period {per[H // 2, W // 2]}, amin {am[H // 2, W // 2]}")
    assert per[H // 2, W // 2] == p and n[H // 2, W // 2] == M2
    assert am[H // 2, W // 2] < amin1


def test_locate_on_the_reference_view_and_its_refusals(tmp_path):
    for prec in ("f32", "f64"):
        rows = locate(tmp_path, "--precision", prec, "--max-iter", "200", "--centre", "-0.5", "0", "--scale", "3", "2.25", "--locate=5")
        assert len(rows) == 5 and int(rows[0].group(1)) == 1                        # the main cardioid's domain is the largest
        assert abs(float(rows[0].group(13))) < 1e-15 and abs(float(rows[0].group(14))) < 1e-15 and rows[0].group(10) == "inside"
        assert len(rows[0].group(13).split(".")[1]) == 20
    rows = locate(tmp_path, "--precision", "perturb", "--max-iter", "200", "--centre", "-0.5", "0", "--scale", "3", "2.25", "--locate", "3")
    assert len(rows) == 3 and int(rows[0].group(1)) == 1
    assert abs(float(rows[0].group(13))) < 1e-15 and abs(float(rows[0].group(14))) < 1e-15
    for bad, word in ((["--precision", "ds"], "--locate: needs --precision f32 | f64 | perturb"), (["--zoom", "1", "1"], "not with --zoom"),
                      (["--locate=0"], "1 .. 64")):
        r = subprocess.run([APP, "--width", "64", "--height", "48", "--quiet", "--locate"] + bad, capture_output=True, text=True, cwd=tmp_path,
                           timeout=120)
        assert r.returncode != 0 and word in r.stdout, r.stdout + r.stderr
