"""BLA tables built on the MI355X (mc_context_bind_mandelbrot_orbit_tables) and dives on one shared orbit (mc_mandelbrot_orbit_rescale).

The device's tables against the host builders', field by field, read back through mc_context_bound_bla_copy / _bla_deep_copy: every
value the same bits, except that where the host holds a NaN the device holds a NaN too, of any sign and payload (include/mc_compute.h);
the radius R is never a NaN and is compared exactly.  (None of the orbits below makes the host produce a NaN: the bounded orbit's
products underflow to zero and none overflows, 0 NaN entries measured; the rule stays in the comparison.)  The shapes sit where the level
layout can go wrong: the first lengths, and L - 2 in {2^k - 1, 2^k, 2^k + 1} on either side of the single-workgroup threshold MC_BLA_TABLE_GROUP_ENTRIES (the second launch starts one
level above it).  Renders after the new bind equal the renders after the plain bind of a host-built table and the numpy restatements;
rebinding; rescaled orbits; the app with both switches against the app with neither.

The existing deep host test (tests/test_mandel_bla_deep_host.py) has no case that reaches the +-2^20 exponent bound (it asserts the bound
on every table, and its deepest exponents stay near 2^13), so none is repeated here."""
import os
import subprocess

import numpy as np
import pytest

import mandel_bla_deep_ref as BD
import mandel_bla_ref as BR
import mandel_perturb_deep_ref as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "mandelbrot")
K4 = ("-0.74364388703715870000000000000000", "0.13182590420531198000000000000000")   # K4's centre written to 32 digits
INTERIOR = ("-0.1", "0.2")
ZERO = dict(centre=(0.0, 0.0), scale=(0.0, 0.0))
U64 = np.uint64


@pytest.fixture(scope="module")
def xctx(B):
    c = B.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_under_the_nan_rule(dev, host, what):
    """Every field the same bits; a host NaN is any NaN on the device.  Column 4 (R) holds no NaN and is compared exactly."""
    assert dev.shape == host.shape, (what, dev.shape, host.shape)
    hn, dn = np.isnan(host), np.isnan(dev)
    assert not hn[:, 4].any() and not dn[:, 4].any(), what
    assert np.array_equal(hn, dn), (what, int((hn != dn).sum()))
    bad = (dev.view(U64) != host.view(U64)) & ~hn
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def check_device_tables(xctx, B, o, plain=True, deep=True):
    """Bind o with the named tables built on the device and compare them with the host builders' (which fill o afterwards)."""
    which = (B.ORBIT_TABLE_BLA if plain else 0) | (B.ORBIT_TABLE_BLA_DEEP if deep else 0)
    xctx.bind_mandelbrot_orbit(o, device_tables=which)
    ms, launches = xctx.last_table_timing()
    counts = BR.level_counts(o.length)
    span = B.bla_table_group_entries().bit_length()            # log2(group) + 1 levels a launch: eleven
    per_table = -(-len(counts) // span) if counts else 0
    assert launches == per_table * (int(plain) + int(deep)) and ms >= 0.0, (launches, len(counts))
    nan_entries = 0
    if plain:
        T, levels = xctx.bound_bla_table()
        assert levels == len(counts) and T.shape == (sum(counts), 5)
        o.bla()
        host = o.bla_table()
        same_under_the_nan_rule(T, host, ("bla", o.length))
        nan_entries = int(np.isnan(host).any(axis=1).sum())
        assert (host[np.isnan(host).any(axis=1), 4] == 0).all()   # a NaN entry has R = 0: the kernels never read its A or B
    if deep:
        mant, exps, levels = xctx.bound_bla_deep_table()
        assert levels == len(counts) and mant.shape == (sum(counts), 5) and exps.shape == (sum(counts), 3)
        o.bla_deep()
        hm, he = o.bla_deep_table()
        assert not np.isnan(hm).any()
        same_under_the_nan_rule(mant, hm, ("bla_deep mantissas", o.length))
        assert np.array_equal(exps, he), ("bla_deep exponents", o.length, int((exps != he).sum()))
    return nan_entries


def test_level_shapes(xctx, B):
    g = B.bla_table_group_entries()
    lengths = [2, 3, 4, 5, 6] + [n + 2 for p in (g // 2, g, 2 * g) for n in (p - 1, p, p + 1)]
    for L in lengths:                                            # a bounded orbit: L = max_iter
        with B.Orbit(*INTERIOR, 1e-14, 1e-14, L) as o:
            assert o.length == L
            check_device_tables(xctx, B, o)
    # 2 g + 1 level-0 entries: three workgroups in the first launch, and a second launch of one workgroup for the level above its span
    assert len(BR.level_counts(2 * g + 3)) == g.bit_length() + 1


def test_no_host_table_is_made(xctx, B):
    with B.Orbit(*INTERIOR, 1e-14, 1e-14, 300) as o:
        xctx.bind_mandelbrot_orbit(o, device_tables=B.ORBIT_TABLE_BLA | B.ORBIT_TABLE_BLA_DEEP)
        L = B.lib()
        buf, ebuf = np.zeros(5 * 600), np.zeros(3 * 600, np.int32)
        assert L.mc_mandelbrot_orbit_bla_copy(o._h, buf.ctypes.data) == 1          # MC_ERR_INVALID_ARGUMENT: the orbit holds no table
        assert L.mc_mandelbrot_orbit_bla_deep_copy(o._h, buf.ctypes.data, ebuf.ctypes.data) == 1
        T, _ = xctx.bound_bla_table()
        assert T.shape[0] == sum(BR.level_counts(300))


ORBITS = [("escaping", K4, (2.0 ** -100, 0.75 * 2.0 ** -100), 20000), ("bounded", INTERIOR, (1e-200, 1e-200), 5000),
          ("centre 0", ("0", "0"), (1e-10, 1e-10), 1000), ("centre -1", ("-1", "0"), (1e-10, 1e-10), 1000)]


@pytest.mark.parametrize("name,centre,scale,M", ORBITS, ids=[v[0] for v in ORBITS])
def test_orbits(xctx, B, name, centre, scale, M):
    with B.Orbit(centre[0], centre[1], scale[0], scale[1], M) as o:
        nan_entries = check_device_tables(xctx, B, o)
        if name.startswith("escaping"):
            assert 3000 < o.length < M
        if name.startswith("bounded"):
            assert o.length == M
            print(f"bounded orbit: {nan_entries} NaN entries in the host's plain table")   # (0 measured: its products underflow, none overflows)
        if name.startswith("centre"):                            # zero entries: A = 0 and R = 0
            T, _ = xctx.bound_bla_table()
            zero = (o.table()[1:o.length - 1] == 0).all(axis=1)
            assert zero.any() and (T[:o.length - 2][zero][:, [0, 1, 4]] == 0).all() and (T[o.length - 2:, 4] == 0).all()


@pytest.mark.parametrize("E", [-1100, -8000])
def test_floatexp_table_below_the_double_range(xctx, B, E):
    with B.Orbit(*INTERIOR, 0.75, 0.5, 1500, E) as o:
        assert o.deep and o.length == 1500
        check_device_tables(xctx, B, o, plain=False)
        mant, exps, _ = xctx.bound_bla_deep_table()
        assert (mant[o.length - 2:, 4] > 0).sum() > 1000         # the merges keep positive radii: their arithmetic is what was compared
        assert exps[:, 0].min() < -1074                          # and |A| shrinks below the double range at the top levels


def test_refusals_come_before_the_binding_is_touched(xctx, B):
    W, H, M = 32, 24, 400
    P = B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_PERTURB_BLA, **ZERO)
    with B.Orbit(*INTERIOR, 1e-14, 1e-14, M) as o, B.Orbit(*INTERIOR, 0.75, 0.5, M, -1100) as deep:
        xctx.bind_mandelbrot_orbit(o, device_tables=B.ORBIT_TABLE_BLA)
        _, want = xctx.mandelbrot(P, want_rgba=False)
        with pytest.raises(B.McError) as e:
            xctx.bind_mandelbrot_orbit(deep, device_tables=B.ORBIT_TABLE_BLA)
        assert e.value.status == 5 and "a deep orbit (min |scale| < 2^-960) renders by the rescaled loop, which has no BLA" in str(e.value)
        with pytest.raises(B.McError) as e:
            xctx.bind_mandelbrot_orbit(deep, device_tables=B.ORBIT_TABLE_BLA | B.ORBIT_TABLE_BLA_DEEP)
        assert e.value.status == 5
        for unknown in (4, 1 << 31, 7):
            with pytest.raises(B.McError) as e:
                xctx.bind_mandelbrot_orbit(o, device_tables=unknown)
            assert e.value.status == 1
        _, got = xctx.mandelbrot(P, want_rgba=False)             # the binding is the one from before the refusals
        assert np.array_equal(got, want)
        xctx.bind_mandelbrot_orbit(None)
        with pytest.raises(B.McError) as e:
            xctx.bound_bla_table()
        assert e.value.status == 1
        with pytest.raises(B.McError) as e:
            xctx.bound_bla_deep_table()
        assert e.value.status == 1
    with B.Context(0) as fresh:
        with pytest.raises(B.McError) as e:
            fresh.last_table_timing()                            # before the first such bind
        assert e.value.status == 1


# ---- renders -------------------------------------------------------------------------------------------------------------------------------
def planes(xctx, B, precision, W, H, M):
    return xctx.mandelbrot(B.mandelbrot_params(W, H, max_iter=M, precision=precision, **ZERO))


def restated(B, o, precision, W, H, M):
    """The numpy restatement's plane, fed the orbit's table and scale (the host builders fill o)."""
    if precision == B.PRECISION_PERTURB_BLA:
        o.bla()
        return BR.plane(o.table(), o.length, o.bla_table(), W, H, M, o.scale)
    o.bla_deep()
    return BD.orbit_plane(o, W, H, M)


def view_orbit(B, name, M):
    if name == "shallow":
        return B.Orbit(*K4, 1e-8, 1e-8 * 2 / 3, M)
    if name == "interior":
        return B.Orbit(*INTERIOR, 1e-14, 1e-14, M)
    c, m, E = D.view(D.M33, "1e-300")
    return B.Orbit(c[0], c[1], *m, M, E)


@pytest.mark.parametrize("view,precision", [("shallow", 4), ("shallow", 5), ("interior", 4), ("interior", 5), ("deep", 5)])
def test_renders_equal_the_host_table_bind_and_the_restatement(xctx, B, O, view, precision):
    W, H, M = 64, 48, 2000
    which = B.ORBIT_TABLE_BLA if precision == 4 else B.ORBIT_TABLE_BLA_DEEP
    with view_orbit(B, view, M) as o:
        xctx.bind_mandelbrot_orbit(o, device_tables=which)       # before the orbit holds any table
        rgba, it = planes(xctx, B, precision, W, H, M)
        ref = restated(B, o, precision, W, H, M)                 # (builds the host table into o)
        xctx.bind_mandelbrot_orbit(o)                            # the plain bind of the host-built table
        rgba_h, it_h = planes(xctx, B, precision, W, H, M)
    assert np.array_equal(it, it_h) and np.array_equal(bits(rgba), bits(rgba_h)), (view, precision, int((it != it_h).sum()))
    assert np.array_equal(it, ref), (view, precision, int((it != ref).sum()))
    lut, _ = O.mandel_lut(M)
    assert np.array_equal(bits(rgba), bits(lut[ref]))
    if view != "interior":
        assert len(np.unique(ref)) >= 10
    else:
        assert (ref == M).mean() > 0.5


def test_rebinding(xctx, B):
    W, H, M = 40, 32, 1500
    P4, P5 = B.PRECISION_PERTURB_BLA, B.PRECISION_PERTURB_BLA_DEEP
    with B.Orbit(*K4, 1e-8, 1e-8, M) as a, B.Orbit(*INTERIOR, 1e-14, 1e-14, M) as b:
        ra4, ra5 = restated(B, a, P4, W, H, M), restated(B, a, P5, W, H, M)     # (a and b hold both host tables from here on)
        rb4, rb5 = restated(B, b, P4, W, H, M), restated(B, b, P5, W, H, M)
        assert not np.array_equal(ra4, rb4)
        xctx.bind_mandelbrot_orbit(a, device_tables=B.ORBIT_TABLE_BLA | B.ORBIT_TABLE_BLA_DEEP)
        assert np.array_equal(planes(xctx, B, P4, W, H, M)[1], ra4) and np.array_equal(planes(xctx, B, P5, W, H, M)[1], ra5)
        xctx.bind_mandelbrot_orbit(b, device_tables=B.ORBIT_TABLE_BLA)          # another orbit, other tables: the deep one comes from b
        assert np.array_equal(planes(xctx, B, P4, W, H, M)[1], rb4) and np.array_equal(planes(xctx, B, P5, W, H, M)[1], rb5)
        same_under_the_nan_rule(xctx.bound_bla_table()[0], b.bla_table(), "rebind")
        assert np.array_equal(xctx.bound_bla_deep_table()[0].view(U64), b.bla_deep_table()[0].view(U64))   # the uploaded one, read back
        xctx.bind_mandelbrot_orbit(a)                                            # plain bind after a device bind
        assert np.array_equal(planes(xctx, B, P4, W, H, M)[1], ra4) and np.array_equal(planes(xctx, B, P5, W, H, M)[1], ra5)
        xctx.bind_mandelbrot_orbit(b, device_tables=B.ORBIT_TABLE_BLA_DEEP)     # and the reverse
        assert np.array_equal(planes(xctx, B, P4, W, H, M)[1], rb4) and np.array_equal(planes(xctx, B, P5, W, H, M)[1], rb5)
        xctx.bind_mandelbrot_orbit(a, device_tables=0)                          # 0: the plain bind
        assert np.array_equal(planes(xctx, B, P4, W, H, M)[1], ra4)
        with B.Orbit(*K4, 1e-8, 1e-8, M) as bare:                                # a table not named and not held: released
            xctx.bind_mandelbrot_orbit(bare, device_tables=B.ORBIT_TABLE_BLA)
            assert np.array_equal(planes(xctx, B, P4, W, H, M)[1], ra4)
            with pytest.raises(B.McError) as e:
                planes(xctx, B, P5, W, H, M)
            assert e.value.status == 1 and "no deep BLA table" in str(e.value)
        xctx.bind_mandelbrot_orbit(None, device_tables=B.ORBIT_TABLE_BLA)       # NULL unbinds
        with pytest.raises(B.McError) as e:
            planes(xctx, B, P4, W, H, M)
        assert e.value.status == 1 and "no orbit bound" in str(e.value)


# ---- rescaled orbits -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst,mant", [(-140, -100, (1.0, 0.75)), (-162, -160, (1.0, 1.0))], ids=["same limbs", "across a limb boundary"])
def test_rescaled_orbit_renders_the_restatement(xctx, B, src, dst, mant):
    W, H, M = 48, 32, 2000
    c, _, _ = D.view(D.M33, "1e-60")                              # a Misiurewicz point, written far more closely than these scales need
    with B.Orbit(c[0], c[1], *mant, M, src) as deepest, deepest.rescale(*mant, dst) as r:
        assert ((deepest.bits + 63) // 64 == (r.bits + 63) // 64) and r.scale == (np.ldexp(mant[0], dst), np.ldexp(mant[1], dst))
        for precision, which in ((4, B.ORBIT_TABLE_BLA), (5, B.ORBIT_TABLE_BLA_DEEP)):
            xctx.bind_mandelbrot_orbit(r, device_tables=which)
            _, it = planes(xctx, B, precision, W, H, M)
            ref = restated(B, r, precision, W, H, M)             # that orbit's table (the source's) and the new scale
            assert np.array_equal(it, ref), (precision, int((it != ref).sum()))
            assert len(np.unique(ref)) >= 10


def test_three_pushes_of_rescaled_orbits(xctx, B):
    W, H, M, K = 48, 32, 1000, 2
    mant, E = (1.0, 0.75), -100
    P = B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_PERTURB_BLA, **ZERO)
    with B.Orbit(*K4, *mant, M, E) as deepest, xctx.zoom(W, H) as z:
        first = None
        for j in range(K + 1):
            with deepest.rescale(*mant, E + (K - j)) as r:
                xctx.bind_mandelbrot_orbit(r, device_tables=B.ORBIT_TABLE_BLA)
                z.push(P)                                        # the "scale exactly halves" check accepts the sequence
                if j == 0:
                    first = planes(xctx, B, B.PRECISION_PERTURB_BLA, W, H, M)[0]
                    assert np.array_equal(bits(z.frame(1.0)[0]), bits(first))   # frame 0 is the keyframe
        with B.Orbit(*K4, *mant, M, E) as fresh:                 # the last keyframe is the deepest orbit's own render
            fresh.bla()
            xctx.bind_mandelbrot_orbit(fresh)
            assert np.array_equal(bits(z.frame(0.5)[0]), bits(planes(xctx, B, B.PRECISION_PERTURB_BLA, W, H, M)[0]))
    xctx.bind_mandelbrot_orbit(None)


# ---- the app -------------------------------------------------------------------------------------------------------------------------------
def run_dive(tmp_path, name, args):
    d = tmp_path / name
    d.mkdir()
    r = subprocess.run([APP, "--quiet", "--width", "96", "--height", "64", "--zoom", "2", "1", "--max-iter", "2000"] + args,
                       capture_output=True, text=True, cwd=d, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    files = sorted(p.name for p in d.glob("mandelbrot_*.png"))
    assert files == [f"mandelbrot_{i:05d}.png" for i in range(3)], files
    return r.stdout, [(d / f).read_bytes() for f in files]


def dive_views():
    c30, _, _ = D.view(D.M33, "1e-30")
    c300, _, _ = D.view(D.M33, "1e-300")
    scale = ["--scale", "1e-30", "6.7e-31"]                      # keyframes of 195, 196, 197 bits: 4 limbs
    return {"K4": ("perturb-bla", 4, ["--centre", K4[0], K4[1]] + scale),
            "M33": ("perturb-bla", 4, ["--centre", c30[0], c30[1]] + scale),
            "M33 below 2^-960": ("perturb-bla-deep", 18, ["--centre", c300[0], c300[1], "--scale", "1e-300", "1e-300"])}   # 1091 .. 1093 bits


@pytest.mark.parametrize("which", ["K4", "M33", "M33 below 2^-960"])
def test_app_dive_with_both_switches_writes_the_defaults_files(B, tmp_path, which):
    precision, limbs, where = dive_views()[which]
    view = ["--precision", precision] + where
    out0, plain = run_dive(tmp_path, "defaults", view)
    out1, both = run_dive(tmp_path, "both", view + ["--zoom-orbit", "shared", "--bla-table", "device"])
    assert plain == both
    if which != "K4":                                            # (K4 at this depth and M = 2000 is all interior: three equal images)
        assert len(set(plain)) == 3
    assert "orbit:" not in out0 and "table:" not in out0         # the defaults print what they printed
    assert out1.count("orbit:") == 1 and "shared by 3 keyframes" in out1 and f"{limbs} fractional limbs" in out1, out1
    assert out1.count("table:") == 3 and out1.count("(device, 1 launches; built by the bind)") == 3, out1
    out2, shared = run_dive(tmp_path, "shared", view + ["--zoom-orbit", "shared"])
    out3, device = run_dive(tmp_path, "device", view + ["--bla-table", "device"])
    assert shared == plain and device == plain
    assert out2.count("orbit:") == 1 and out2.count("table:") == 3 and "(host; uploaded by the bind)" in out2
    assert "orbit:" not in out3 and out3.count("table:") == 3


def test_app_still_with_the_device_table(B, tmp_path):
    args = ["--quiet", "--width", "96", "--height", "64", "--max-iter", "2000", "--precision", "perturb-bla", "--centre", K4[0], K4[1],
            "--scale", "1e-30", "6.7e-31"]
    imgs = []
    for extra in ([], ["--bla-table", "device"]):
        out = tmp_path / f"still{len(imgs)}.png"
        r = subprocess.run([APP] + args + ["--out", str(out)] + extra, capture_output=True, text=True, cwd=tmp_path, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("table:" in r.stdout) == bool(extra)
        imgs.append(out.read_bytes())
    assert imgs[0] == imgs[1]
