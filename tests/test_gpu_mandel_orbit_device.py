"""mc_mandelbrot_orbit_create_device on the MI355X: the kernel's product against Python integers; the device orbit against the host
constructor's, field by field and bit by bit (pure integer arithmetic: no tolerance), over the limb counts at which the code changes
path, escapes, exact zeros, a subnormal entry, every refusal, the launch boundaries; everything downstream of an orbit; the app."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mandel_orbit_device_cases as K
import mandel_perturb_deep_ref as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "mandelbrot")
LAUNCH_WORK = 32_000_000   # kOrbitLaunchWork (csrc/mandel_perturb.h): a launch runs at most LAUNCH_WORK / (k + 1)^2 iterations, in [1, 65536]


def launch_iters(k):
    return min(65536, max(1, LAUNCH_WORK // ((k + 1) ** 2)))


@pytest.fixture(scope="module")
def xctx(B):
    c = B.Context(0)
    yield c
    c.close()


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def both(B, xctx, cx, cy, M, k=None, scale=None):
    """(host orbit, device orbit) for k fractional limbs (mantissas 1.0) or for scale = (mx, my, E)."""
    mx, my, E = scale if scale else (1.0, 1.0, K.exp2_for(k))
    h = B.Orbit(cx, cy, mx, my, M, E)
    d = B.Orbit(cx, cy, mx, my, M, E, device=xctx)
    if k is not None:
        assert (h.bits + 63) // 64 == k
    return h, d


def assert_same(h, d, what=None):
    assert (d.length, d.max_iter, d.bits, d.deep, d.scale, d.scale_exp2) == (h.length, h.max_iter, h.bits, h.deep, h.scale, h.scale_exp2), what
    assert np.array_equal(u64(d.table()), u64(h.table())), what


def test_timing_needs_a_device_orbit_first(B):
    with B.Context(0) as c:
        with pytest.raises(B.McError) as e:
            c.last_orbit_timing()
        assert e.value.status == 1


@pytest.mark.parametrize("k", (1, 2, 3, 17, 64, 65, 130))
def test_device_product(B, xctx, k):
    T = B.test_lib()
    for name, a, b in K.crafted_operands(k):
        A, Bv, out = K.limbs(a, k), K.limbs(b, k), np.zeros(k + 1, np.uint64)
        assert T.mc_hook_orbit_mul_device(xctx._h, k, A.ctypes.data, Bv.ctypes.data, out.ctypes.data) == 0
        assert K.value(out) == K.rounded_product(a, b, k), (k, name)


def mirror(c, sx, sy):
    flip = lambda t, s: t if s > 0 else (t[1:] if t.startswith("-") else "-" + t)
    return flip(c[0], sx), flip(c[1], sy)


@pytest.mark.parametrize("k", (2, 3, 4, 17, 18, 31, 32, 33, 54, 63, 64, 65, 127, 128, 129, 130))
def test_table_equals_the_host_orbit(B, xctx, k):
    M = 1500
    prec = 64 * k + 64
    m33 = D.misiurewicz(*D.M33, prec)
    centres = [m33, D.misiurewicz(*D.M41, prec), ("-0.1", "0.2")]
    if k in (54, 130):   # every sign path of add and sub
        centres += [mirror(m33, -1, 1), mirror(m33, 1, -1), mirror(m33, -1, -1)]
    for c in centres:
        h, d = both(B, xctx, c[0], c[1], M, k)
        with h, d:
            assert h.deep == (k >= 18)   # (at few limbs the Misiurewicz orbits, which repel, leave their point and escape before M)
            assert h.length == M or c[0] != "-0.1"
            assert_same(h, d, (k, c[0][:12], c[1][:12]))
            assert xctx.last_orbit_timing()[2] == k + 1


@pytest.mark.parametrize("k", (2, 17, 54, 130))
def test_escape(B, xctx, k):
    with B.Orbit("-0.75", "0.01", 1.0, 1.0, 5000, K.exp2_for(k)) as o:
        L = o.length
    assert 100 < L < 1000
    for M in (L - 1, L, L + 1, 2 * L):
        h, d = both(B, xctx, "-0.75", "0.01", M, k)
        with h, d:
            assert h.length == min(L, M)
            assert_same(h, d, (k, M))
    h, d = both(B, xctx, "-2", "0", 50, k)
    with h, d:
        assert h.length == 1
        assert_same(h, d)


@pytest.mark.parametrize("centre", [("0", "0"), ("-1", "0"), ("0", "1")])
def test_exact_zeros(B, xctx, centre):
    for k in (2, 18, 130):
        h, d = both(B, xctx, centre[0], centre[1], 60, k)
        with h, d:
            Z = d.table()
            assert_same(h, d, (centre, k))
            assert (Z[1:] == 0).any()
            assert not (np.signbit(Z) & (Z == 0) & ~np.signbit(h.table())).any()   # no negative zero where the host has none


def test_subnormal_entry(B, xctx):
    m, E = B.scale_from_text("1e-300")
    h, d = both(B, xctx, "-0.75", "3e-320", 200, scale=(m, m, E))
    with h, d:
        assert h.bits == 1093 and h.deep
        y1 = h.table()[1, 1]
        assert 0 < y1 < 2.0 ** -1022 and y1 == 3e-320   # the correctly rounded subnormal
        assert_same(h, d)


def detail_after_name(B, name):
    text = B.lib().mc_last_error_detail().decode()
    assert text.startswith(name + ": "), text
    return text[len(name) + 2:]


def refusal(B, xctx, args, device):
    with pytest.raises(B.McError) as e:
        B.Orbit(*args, device=xctx if device else None)
    return e.value.status


def test_tiny_entry_refusal(B, xctx):
    c = D.nucleus(3, D.NUCLEUS3, 1500, 400)
    m, E = B.scale_from_text("1e-1000")
    args = (c[0], c[1], m, m, 100, E)
    assert refusal(B, xctx, args, False) == 5
    host = detail_after_name(B, "mc_mandelbrot_orbit_create_deep")
    assert refusal(B, xctx, args, True) == 5
    dev = detail_after_name(B, "mc_mandelbrot_orbit_create_device")
    assert dev == host and "Z_3 " in dev


REFUSALS = [   # tests/test_mandel_perturb_deep_host.py: test_refusals and test_bad_centre_is_still_invalid
    ("-0.75", "0.1", 0.5, 1.0, 10, -8192), ("-0.75", "0.1", 0.999, 0.999, 10, -8192), ("-0.75", "0.1", 1.0, 1.0, 10, -2 ** 31),
    ("-0.75", "0.1", 0.0, 1.0, 10, -3000), ("-0.75", "0.1", 1.0, -0.0, 10, -3000), ("-0.75", "0.1", float("inf"), 1.0, 10, -3000),
    ("-0.75", "0.1", 1.0, float("nan"), 10, -3000), ("-0.75", "0.1", 1.0, 1.0, 10, 1100), ("-0.75x", "0.1", 1.0, 1.0, 10, -3000),
    ("-0.75", "0.1", 1.0, 1.0, 0, -3000), ("-0.75x", "0.1", 1.0, 1.0, 10, -30), ("4.5", "0", 1.0, 1.0, 10, -30),
]


@pytest.mark.parametrize("args", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_every_other_refusal(B, xctx, args):
    want = refusal(B, xctx, args, False)
    text = B.lib().mc_last_error_detail().decode()
    host = text.split(": ", 1)[1]   # (create_deep names mc_mandelbrot_orbit_create where it forwards to it)
    assert refusal(B, xctx, args, True) == want
    assert detail_after_name(B, "mc_mandelbrot_orbit_create_device") == host


def test_null_out_pointer(B, xctx):
    assert B.lib().mc_mandelbrot_orbit_create_device(xctx._h, b"0", b"0", 1.0, 1.0, 0, 10, None) == 1


def test_launch_boundaries_deep(B, xctx):
    k = 130
    chunk = launch_iters(k)
    assert 1 < chunk < 20000
    for M, launches in ((chunk, 1), (chunk + 1, 2), (2 * chunk + 1, 3)):   # an orbit that ends on the last iteration of a launch, on
        h, d = both(B, xctx, "-0.1", "0.2", M, k)                          # the first of the next, and one of three launches
        with h, d:
            assert_same(h, d, M)
            ms, n, limbs = xctx.last_orbit_timing()
            assert (n, limbs) == (launches, k + 1) and ms > 0


def test_launch_boundaries_shallow(B, xctx):
    assert launch_iters(2) == 65536
    h, d = both(B, xctx, "-0.1", "0.2", 65536 + 3, 2)
    with h, d:
        assert_same(h, d)
        assert xctx.last_orbit_timing()[1] >= 2


def escape_centre(B, k, target):
    """A real centre 0.25 + eps, just past the cusp, whose orbit escapes at exactly L = target (L is about pi / sqrt(eps), in steps of
    one): bisection on eps with shallow host orbits, which cost a microsecond per iteration."""
    lo, hi = (3.0 / target) ** 2, (3.3 / target) ** 2   # L(lo) > target > L(hi)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        with B.Orbit(repr(0.25 + mid), "0", 1.0, 1.0, 2 * target, K.exp2_for(2)) as o:
            L = o.length
        if L == target:
            return repr(0.25 + mid)
        lo, hi = (mid, hi) if L > target else (lo, mid)
    raise AssertionError("no centre found")


def test_escape_at_a_launch_boundary(B, xctx):
    """The escape that ends the orbit is found on the last iteration of the first launch, and on the first iteration of the second."""
    k = 130
    chunk = launch_iters(k)
    for L in (chunk, chunk + 1):
        cx = escape_centre(B, k, L)
        h, d = both(B, xctx, cx, "0", 2 * chunk, k)
        with h, d:
            assert h.length == L   # (the construction: the same escape at 130 limbs as at 2)
            assert_same(h, d, L)
            assert xctx.last_orbit_timing()[1] == 2


def pp(B, W, H, M):
    return B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_PERTURB_BLA_DEEP, centre=(0.0, 0.0), scale=(0.0, 0.0))


def test_downstream(B, xctx):
    W, H, M = 96, 64, 6000
    c, m, E = D.view(D.M33, "1e-1000")
    with B.Context(0) as other, B.Orbit(c[0], c[1], *m, M, E) as h:
        h.bla_deep()
        xctx.bind_mandelbrot_orbit(h)
        _, want = xctx.mandelbrot(pp(B, W, H, M), want_rgba=False)
        assert len(np.unique(want)) >= 10
        with B.Orbit(c[0], c[1], *m, M, E, device=xctx) as d:
            _, still = xctx.mandelbrot(pp(B, W, H, M), want_rgba=False)   # the host orbit is still the bound one
            assert np.array_equal(still, want)
            assert_same(h, d)
            assert d.bla_deep() == (h.bla_deep_levels, h.bla_deep_entries)
            for a, b in zip(d.bla_deep_table(), h.bla_deep_table()):
                assert np.array_equal(a, b)
            for ctx in (xctx, other):                                     # bound on the context that made it, and on another
                ctx.bind_mandelbrot_orbit(d)
                _, got = ctx.mandelbrot(pp(B, W, H, M), want_rgba=False)
                assert np.array_equal(got, want)
    with B.Orbit("-0.1", "0.2", 1e-20, 1e-20, 800, 0) as h, B.Orbit("-0.1", "0.2", 1e-20, 1e-20, 800, 0, device=xctx) as d:
        assert not d.deep and d.scale == (1e-20, 1e-20)                   # where create_deep forwards to the plain constructor
        assert_same(h, d)
        assert d.bla() == h.bla() and np.array_equal(d.bla_table(), h.bla_table())
    xctx.bind_mandelbrot_orbit(None)


def test_app_orbit_option(B, tmp_path):
    W, H, M = 96, 64, 6000
    c, _, _ = D.view(D.M33, "1e-1000")
    base = [APP, "--precision", "perturb-bla-deep", "--width", str(W), "--height", str(H), "--max-iter", str(M), "--centre", c[0], c[1],
            "--scale", "1e-1000", "1e-1000", "--quiet"]
    png = {}
    for where in ("host", "device", "auto"):
        out = tmp_path / f"{where}.png"
        r = subprocess.run(base + ["--orbit", where, "--out", str(out)], capture_output=True, text=True, cwd=tmp_path, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        line = [s for s in r.stdout.splitlines() if s.startswith("orbit: ")]
        assert len(line) == 1 and "3418 bits" in line[0], r.stdout
        if where != "auto":   # (auto: whichever side DESIGN.md section 3.13 measured faster at this limb count)
            assert f"({where}," in line[0], r.stdout
        png[where] = out.read_bytes()
    assert png["device"] == png["host"] == png["auto"]
    r = subprocess.run(base + ["--out", str(tmp_path / "plain.png")], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0 and "orbit: " not in r.stdout and (tmp_path / "plain.png").read_bytes() == png["host"]
    r = subprocess.run(base + ["--orbit", "bogus"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 1 and "--orbit bogus: not one of host | device | auto" in r.stdout
    bad = [a if a != c[0] else c[0] + "x" for a in base]
    msgs = []
    for where in ("host", "device"):
        r = subprocess.run(bad + ["--orbit", where], capture_output=True, text=True, cwd=tmp_path, timeout=120)
        assert r.returncode == 1
        msgs.append([s for s in r.stdout.splitlines() if s.startswith("--centre ")][0])
    assert msgs[0].replace("mc_mandelbrot_orbit_create_deep", "mc_mandelbrot_orbit_create_device") == msgs[1]
