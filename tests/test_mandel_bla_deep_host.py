"""MC_PRECISION_PERTURB_BLA_DEEP without a GPU: the library's floatexp table against the numpy restatement bit for bit, and against
precision 4's table on shallow orbits; the numpy loop against the scalar one (tests/mandel_bla_deep_ref.py); the parity with precision 4
on shallow views; accuracy against the rescaled loop's plane and direct fixed-point iteration on deep views; that the loop skips; the
refusals; the app's option handling."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mandel_bla_deep_ref as BD
import mandel_bla_ref as BR
import mandel_perturb_deep_ref as D
import mandel_perturb_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K4 = R.DEEP_CENTRE
REF = ("-0.445", "0")


def test_enum_value(B):
    assert B.PRECISION_PERTURB_BLA_DEEP == 5 and B.MANDEL_BLA_COUNT_TRIPS == 8


def deep(B, point, depth, M, mantissa=None):
    c, m, E = D.view(point, depth)
    o = B.Orbit(c[0], c[1], *(mantissa or m), M, E)
    assert o.deep
    return o


def check_table(o):
    levels, entries = o.bla_deep()
    assert o.bla_deep() == (levels, entries)                # built once, the same shape on a second call
    counts = BR.level_counts(o.length)
    assert levels == len(counts) and entries == sum(counts)
    mant, exps = o.bla_deep_table()
    assert mant.shape == (entries, 5) and exps.shape == (entries, 3) and exps.dtype == np.int32
    wm, we = BD.table(o.table(), o.length, o.scale, BD.orbit_E(o))
    assert np.array_equal(mant.view(np.uint64), wm.view(np.uint64)), int((mant.view(np.uint64) != wm.view(np.uint64)).sum())
    assert np.array_equal(exps, we), int((exps != we).sum())
    a = np.fmax(np.abs(mant[:, [0, 2]]), np.abs(mant[:, [1, 3]]))
    assert (((a >= 0.5) & (a < 1.0)) | (a == 0.0)).all()   # normalised mantissas
    assert ((mant[:, 4] == 0.0) | ((mant[:, 4] >= 0.5) & (mant[:, 4] < 1.0))).all()
    assert (np.abs(exps) <= BD.BOUND).all()
    return mant, exps


@pytest.mark.parametrize("point,depth,M", [(D.M33, "1e-300", 3000), (D.M41, "1e-300", 3000), (D.M33, "1e-1000", 6000),
                                           (D.M41, "1e-1000", 6000), (D.M33, "1e-2400", 12000)])
def test_deep_table_is_the_restatement(B, point, depth, M):
    with deep(B, point, depth, M) as o:
        mant, exps = check_table(o)
    assert (mant[:, 4] > 0).mean() > 0.99                   # these orbits stay away from 0: nearly every radius is positive
    if D.view(point, depth)[2] < -3000:                     # below 1e-1000 B leaves the double range (|B| ~ 2^-E at the top levels)
        assert exps[:, 1].max() > 1024


SHALLOW = [
    ("reference view", REF, (2.34, 2.34), 256),
    ("K4 1e-20", K4, (1e-20, 1e-20 * 2 / 3), 20000),
    ("escaping orbit", ("-0.75", "0.1"), (1e-20, 1e-20), 20000),
    ("interior", ("-0.1", "0.2"), (1e-200, 1e-200), 20000),
    ("centre -1 (exact zeros)", ("-1", "0"), (1e-10, 1e-10), 1000),
    ("L = 2", ("1", "0"), (1e-3, 1e-3), 100),
]


@pytest.mark.parametrize("name,centre,scale,M", SHALLOW, ids=[v[0] for v in SHALLOW])
def test_shallow_table_is_the_restatement_and_precision_4s(B, name, centre, scale, M):
    with B.Orbit(centre[0], centre[1], scale[0], scale[1], M) as o:
        mant, exps = check_table(o)
        o.bla()
        T = o.bla_table()
    back = np.ldexp(mant, np.repeat(exps, [2, 2, 1], axis=1))
    normal = (T == 0.0) | (np.abs(T) >= np.finfo(np.float64).tiny)
    sel = (T[:, 4] > 0) & normal.all(axis=1) & np.isfinite(T).all(axis=1)
    assert np.array_equal(back[sel].view(np.uint64), T[sel].view(np.uint64)), (name, int(sel.sum()))
    assert (mant[sel, 4] > 0).all()
    if name == "centre -1 (exact zeros)":
        assert (mant[BR.level_counts(o.length)[0]:, 4] == 0).all()


def test_radius_never_grows_with_the_level(B):
    with deep(B, D.M33, "1e-1000", 6000) as o:
        o.bla_deep()
        mant, exps = o.bla_deep_table()
        L, levels = o.length, o.bla_deep_levels
    off = BR.level_offsets(L)
    for k in range(1, levels):
        m = 1 + (np.arange(off[k + 1] - off[k]) << k)
        par = off[k - 1] + ((m - 1) >> (k - 1))
        cur = slice(off[k], off[k + 1])
        assert not BD.less((mant[par, 4], exps[par, 2].astype(np.int64)), (mant[cur, 4], exps[cur, 2].astype(np.int64))).any(), k


@pytest.mark.parametrize("centre", [("-1", "0"), ("0", "0")])
def test_orbits_through_zero_never_skip(B, centre):
    W, H, M = 24, 16, 1000
    with B.Orbit(centre[0], centre[1], 1e-10, 1e-10, M) as o:
        o.bla_deep()
        n = BD.orbit_plane(o, W, H, M)
        tr = BD.orbit_plane(o, W, H, M, trips=True)
        mant, _ = o.bla_deep_table()
    assert (mant[BR.level_counts(M)[0]:, 4] == 0).all() if len(BR.level_counts(M)) > 1 else True
    assert np.array_equal(tr.astype(np.int64), np.minimum(n.astype(np.int64) + 1, M))   # one iteration per trip


def test_numpy_loop_equals_scalar(B):
    cases = [(deep(B, D.M33, "1e-1000", 6000), 24, 16, 6000),
             (deep(B, D.M41, "1e-900", 4000, (-0.7, 0.45)), 20, 12, 4000),
             (B.Orbit(*K4, 1e-10, 1e-10, 3000), 24, 16, 3000),
             (B.Orbit("-0.1", "0.2", 1e-200, 1e-200, 3000), 24, 16, 3000),
             (B.Orbit("-1", "0", 1e-10, 1e-10, 500), 12, 8, 500)]
    for o, W, H, M in cases:
        with o:
            o.bla_deep()
            pl = BD.orbit_plane(o, W, H, M)
            tr = BD.orbit_plane(o, W, H, M, trips=True)
            Zl = o.table().tolist()
            mant, exps = o.bla_deep_table()
            tab = (mant.tolist(), exps.astype(np.int64).tolist())
            E = BD.orbit_E(o)
            ux, uy = D.u_axis(W, o.scale[0]), D.u_axis(H, o.scale[1])
            for y in range(0, H, 3):
                for x in range(0, W, 5):
                    assert pl[y, x] == BD.scalar_iters(Zl, o.length, tab, float(ux[x]), float(uy[y]), E, M), (o.scale, x, y)
                    assert tr[y, x] == BD.scalar_iters(Zl, o.length, tab, float(ux[x]), float(uy[y]), E, M, trips=True), (o.scale, x, y)


PARITY = [   # the views of tests/test_gpu_mandel_bla.py
    ("reference view", 96, 64, 256, REF, (2.34, 2.34)),
    ("K4 1e-8", 64, 48, 20000, K4, (1e-8, 1e-8 * 2 / 3)),
    ("K4 1e-20", 64, 48, 20000, K4, (1e-20, 1e-20)),
    ("interior-heavy 1e-14", 64, 48, 5000, ("-0.1", "0.2"), (1e-14, 1e-14)),
    ("interior 1e-200", 64, 48, 20000, ("-0.1", "0.2"), (1e-200, 1e-200)),
    ("1e-100", 40, 24, 3000, ("-0.75", "0.1"), (1e-100, 1e-100)),
    ("2^-950", 24, 16, 2000, ("-1.25", "0.001"), (2.0 ** -950, 2.0 ** -950)),
    ("centre -1 (zeros in the orbit)", 40, 24, 1000, ("-1", "0"), (1e-10, 1e-10)),
    ("odd sizes, M % 8 != 0", 77, 45, 1003, ("-0.75", "0.1"), (0.05, 0.03)),
    ("M < 8", 13, 5, 7, REF, (2.34, 2.34)),
]


@pytest.mark.parametrize("name,W,H,M,centre,scale", PARITY, ids=[v[0] for v in PARITY])
def test_parity_with_precision_4_on_shallow_views(B, name, W, H, M, centre, scale):
    """include/mc_compute.h: where no floatexp operation goes subnormal or overflows, precision 5 computes precision 4's values.  The
    iteration planes are equal on every view; so are the trip planes, except where precision 4's table lost entries to the double range
    (a product in its chain underflowed or overflowed: interior 1e-200) and precision 5 skips where precision 4 could not."""
    with B.Orbit(centre[0], centre[1], scale[0], scale[1], M) as o:
        o.bla()
        o.bla_deep()
        Z, L, T = o.table(), o.length, o.bla_table()
        n5 = BD.orbit_plane(o, W, H, M)
        t5 = BD.orbit_plane(o, W, H, M, trips=True)
        mant, _ = o.bla_deep_table()
    n4 = BR.plane(Z, L, T, W, H, M, scale)
    t4 = BR.plane(Z, L, T, W, H, M, scale, trips=True)
    assert np.array_equal(n5, n4), (name, int((n5 != n4).sum()))
    if ((mant[:, 4] > 0) == (T[:, 4] > 0)).all():
        assert np.array_equal(t5, t4), (name, int((t5 != t4).sum()))
    else:
        assert name == "interior 1e-200" and (t5 <= t4).all()


def test_accuracy_on_deep_views(B):
    """24 sampled pixels against direct fixed-point iteration at bits + 64, and whole CPU-sized planes against the rescaled loop's."""
    W, H = 64, 48
    rng = np.random.default_rng(5)
    for point, depth, M in ((D.M33, "1e-1000", 6000), (D.M41, "1e-300", 3000)):
        c, m, E = D.view(point, depth)
        with B.Orbit(c[0], c[1], *m, M, E) as o:
            o.bla_deep()
            p5 = BD.orbit_plane(o, W, H, M)
            pd = D.orbit_plane(o, W, H, M)
            bits = o.bits
        assert (p5 == pd).mean() >= 0.99, (depth, int((p5 != pd).sum()))
        gx, gy = rng.integers(0, W, 24), rng.integers(0, H, 24)
        truth = np.array([D.mp_iters_deep(c, m, E, W, H, int(x), int(y), M, bits + 64) for x, y in zip(gx, gy)])
        assert (p5[gy, gx] == truth).sum() >= 22, (depth, p5[gy, gx], truth)
        assert len(np.unique(truth)) >= 5, depth


def test_skipping_happens_on_a_deep_view(B):
    W, H, M = 64, 48, 6000
    with deep(B, D.M33, "1e-1000", M) as o:
        o.bla_deep()
        n = BD.orbit_plane(o, W, H, M)
        tr = BD.orbit_plane(o, W, H, M, trips=True)
    count = np.minimum(n.astype(np.int64) + 1, M).mean()
    assert tr.astype(np.float64).mean() * 10 <= count, (tr.mean(), count)


def test_refusals(B):
    L = B.lib()
    lv, ne = C.c_uint32(0), C.c_uint64(0)
    assert L.mc_mandelbrot_orbit_bla_deep(None, C.byref(lv), C.byref(ne)) == 1
    mant = np.zeros(5, np.float64)
    exps = np.zeros(3, np.int32)
    assert L.mc_mandelbrot_orbit_bla_deep_copy(None, mant.ctypes.data_as(C.c_void_p), exps.ctypes.data_as(C.c_void_p)) == 1
    with B.Orbit(*K4, 1e-10, 1e-10, 100) as o:
        assert L.mc_mandelbrot_orbit_bla_deep_copy(o._h, mant.ctypes.data_as(C.c_void_p), exps.ctypes.data_as(C.c_void_p)) == 1
        with pytest.raises(ValueError):
            o.bla_deep_table()                              # before bla_deep()
        assert L.mc_mandelbrot_orbit_bla_deep(o._h, None, None) == 0   # shape pointers may be NULL
        assert L.mc_mandelbrot_orbit_bla_deep_copy(o._h, None, exps.ctypes.data_as(C.c_void_p)) == 1
    with B.Orbit("-0.75", "0.1", 0.75, 0.5, 200, scale_exp2=-1000) as d:   # deep orbits: accepted here, still refused by bla()
        assert d.deep
        assert d.bla_deep()[1] == sum(BR.level_counts(d.length))
        with pytest.raises(B.McError) as e:
            d.bla()
        assert e.value.status == 5


def app(*args, cwd):
    return subprocess.run([os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "mandelbrot")] + list(args), capture_output=True,
                          text=True, cwd=cwd, timeout=120)


def test_app_accepts_perturb_bla_deep_with_a_deep_scale(B, tmp_path):
    """Parsed and run up to the device: without a GPU init() fails with the device message, with one the image is written."""
    c, _, _ = D.view(D.M33, "1e-1000")
    r = app("--precision", "perturb-bla-deep", "--centre", c[0], c[1], "--scale", "1e-1000", "1e-1000", "--width", "64", "--height", "48",
            "--max-iter", "500", "--quiet", cwd=tmp_path)
    assert "not one of" not in r.stdout and "below 2^-960" not in r.stdout
    assert (r.returncode == 0 and (tmp_path / "mandelbrot.png").exists()) or (r.returncode == 1 and "could not find a device" in r.stdout)


def test_app_points_perturb_bla_at_the_deep_precision(B, tmp_path):
    r = app("--precision", "perturb-bla", "--centre", "-0.75", "0.1", "--scale", "1e-300", "1e-300", cwd=tmp_path)
    assert r.returncode == 1 and "below 2^-960" in r.stdout and "perturb-bla-deep" in r.stdout
