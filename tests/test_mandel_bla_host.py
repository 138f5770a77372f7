"""MC_PRECISION_PERTURB_BLA without a GPU: the library's BLA table against the numpy restatement bit for bit, the numpy loop against the
scalar one (tests/mandel_bla_ref.py), the refusals, accuracy against PERTURB's restated plane and against direct high-precision
iteration, that the loop does skip, and the app's option handling."""
import os
import subprocess

import numpy as np
import pytest

import mandel_bla_ref as BR
import mandel_perturb_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K4 = R.DEEP_CENTRE


@pytest.fixture(scope="module")
def boundary_views():
    """test_mandel_perturb_host.py's boundary points (their own orbits escape, L < M) and scales."""
    return [
        (R.mp_boundary_point(("-0.5", "0"), ("-0.5", "1"), 4000, 70, 134), 1e-20, 4000),
        (R.mp_boundary_point(("0.3", "0"), ("0.3", "1"), 3000, 103, 167), 1e-30, 3000),
        (R.mp_boundary_point(("-0.5", "0"), ("-0.5", "1"), 10000, 190, 254), 1e-50, 10000),
    ]


def test_enum_value(B):
    assert B.PRECISION_PERTURB_BLA == 4 and B.MANDEL_BLA_COUNT_TRIPS == 8


def tables(B, centre, scale, M):
    with B.Orbit(centre[0], centre[1], scale[0], scale[1], M) as o:
        levels, entries = o.bla()
        assert o.bla() == (levels, entries)                 # built once, the same shape on a second call
        return o.table(), o.length, o.bla_table(), levels, entries


@pytest.mark.parametrize("name,centre,scale,M", [
    ("reference view", ("-0.445", "0"), (2.34, 2.34), 256),
    ("K4 1e-20", K4, (1e-20, 1e-20 * 2 / 3), 20000),
    ("escaping orbit", ("-0.75", "0.1"), (1e-20, 1e-20), 20000),
    ("interior", ("-0.1", "0.2"), (1e-200, 1e-200), 20000),
    ("centre -1 (exact zeros)", ("-1", "0"), (1e-10, 1e-10), 1000),
    ("L = 2", ("1", "0"), (1e-3, 1e-3), 100),
])
def test_table_is_the_restatement(B, name, centre, scale, M):
    Z, L, T, levels, entries = tables(B, centre, scale, M)
    counts = BR.level_counts(L)
    assert levels == len(counts) and entries == sum(counts) and T.shape == (entries, 5)
    want = BR.table(Z, L, scale)
    assert np.array_equal(T.view(np.uint64), want.view(np.uint64)), (name, int((T != want).sum()))
    assert (T[:, 4] >= 0).all() and np.isfinite(T[:, 4]).all()
    if name == "escaping orbit":
        assert L < M
    if name == "centre -1 (exact zeros)":                   # Z_j = 0 at every even j: every level >= 1 has R = 0
        assert levels >= 2 and (T[counts[0]:, 4] == 0).all()


def test_radius_never_grows_with_the_level(B):
    Z, L, T, levels, _ = tables(B, K4, (1e-20, 1e-20), 20000)
    off = BR.level_offsets(L)
    for k in range(1, levels):
        m = 1 + (np.arange(off[k + 1] - off[k]) << k)
        assert (T[off[k]:off[k + 1], 4] <= T[off[k - 1] + ((m - 1) >> (k - 1)), 4]).all(), k


def test_numpy_loop_equals_scalar(B):
    W, H, M = 24, 16, 3000
    for centre, scale in ((K4, 1e-10), (("-0.445", "0"), 2.34), (("-0.1", "0.2"), 1e-200), (("-0.5", "0.601612404061598243828492"), 1e-20)):
        Z, L, T, _, _ = tables(B, centre, (scale, scale), M)
        pl = BR.plane(Z, L, T, W, H, M, (scale, scale))
        tr = BR.plane(Z, L, T, W, H, M, (scale, scale), trips=True)
        Zl, Tl = Z.tolist(), T.tolist()
        dx, dy = R.dc_axis(W, scale), R.dc_axis(H, scale)
        for y in range(0, H, 3):
            for x in range(0, W, 5):
                assert pl[y, x] == BR.scalar_iters(Zl, L, Tl, float(dx[x]), float(dy[y]), M), (centre, x, y)
                assert tr[y, x] == BR.scalar_iters(Zl, L, Tl, float(dx[x]), float(dy[y]), M, trips=True), (centre, x, y)


def test_deep_orbit_is_refused(B):
    with B.Orbit("-0.75", "0.1", 0.75, 0.5, 200, scale_exp2=-1000) as o:
        assert o.deep
        with pytest.raises(B.McError) as e:
            o.bla()
        assert e.value.status == 5 and "deep" in str(e.value)


def test_null_and_missing_table_are_refused(B):
    import ctypes as C
    L = B.lib()
    assert L.mc_mandelbrot_orbit_bla(None, None, None) == 1
    out = np.zeros(5, np.float64)
    assert L.mc_mandelbrot_orbit_bla_copy(None, out.ctypes.data_as(C.c_void_p)) == 1
    with B.Orbit(*K4, 1e-10, 1e-10, 100) as o:
        assert L.mc_mandelbrot_orbit_bla_copy(o._h, out.ctypes.data_as(C.c_void_p)) == 1   # before mc_mandelbrot_orbit_bla
        with pytest.raises(ValueError):
            o.bla_table()
        assert L.mc_mandelbrot_orbit_bla(o._h, None, None) == 0                          # shape pointers may be NULL


def sampled_truth(centre, scale, M, bits, W, H, gx, gy):
    return np.array([R.mp_iters(*R.pixel_c(centre, (scale, scale), W, H, x, y, 2 * bits), M, 2 * bits) for x, y in zip(gx, gy)])


def test_accuracy_against_perturb_and_direct_iteration(B, boundary_views):
    W, H, n = 64, 48, 160
    for centre, scale, M in boundary_views:
        with B.Orbit(centre[0], centre[1], scale, scale, M) as o:
            o.bla()
            Z, L, T, bits = o.table(), o.length, o.bla_table(), o.bits
        assert L < M
        bla = BR.plane(Z, L, T, W, H, M, (scale, scale))
        per = R.plane(Z, L, W, H, M, (scale, scale))
        assert (bla == per).mean() >= 0.99, (scale, int((bla != per).sum()))
        rng = np.random.default_rng(7)
        gx, gy = rng.integers(0, W, n), rng.integers(0, H, n)
        truth = sampled_truth(centre, scale, M, bits, W, H, gx, gy)
        assert (bla[gy, gx] == truth).sum() >= (per[gy, gx] == truth).sum() - 1, scale
        assert len(np.unique(truth)) >= (10 if scale <= 1e-50 else 20)


def test_skipping_happens_on_the_interior_view(B):
    W, H, M = 64, 48, 20000
    Z, L, T, _, _ = tables(B, ("-0.1", "0.2"), (1e-200, 1e-200), M)
    assert L == M
    tr = BR.plane(Z, L, T, W, H, M, (1e-200, 1e-200), trips=True)
    assert tr.astype(np.float64).mean() <= M / 20, tr.mean()
    assert (BR.plane(Z, L, T, W, H, M, (1e-200, 1e-200)) == M).all()


def app(*args, cwd):
    return subprocess.run([os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "mandelbrot")] + list(args), capture_output=True,
                          text=True, cwd=cwd, timeout=60)


def test_app_accepts_perturb_bla(B, tmp_path):
    """Parsed and run up to the device: without a GPU init() fails with the device message, with one the image is written."""
    r = app("--precision", "perturb-bla", "--centre", "-0.7436438870371587047521915", "0.13182590420531197049", "--scale", "1e-30",
            "1e-30", "--width", "64", "--height", "48", "--max-iter", "100", "--quiet", cwd=tmp_path)
    assert "not one of" not in r.stdout
    assert (r.returncode == 0 and (tmp_path / "mandelbrot.png").exists()) or (r.returncode == 1 and "could not find a device" in r.stdout)


def test_app_refuses_a_deep_scale_before_the_device(B, tmp_path):
    r = app("--precision", "perturb-bla", "--centre", "-0.75", "0.1", "--scale", "1e-300", "1e-300", cwd=tmp_path)
    assert r.returncode == 1 and "below 2^-960" in r.stdout and "could not find a device" not in r.stdout
    assert "using device" not in r.stdout and not list(tmp_path.iterdir())
