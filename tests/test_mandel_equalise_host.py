"""MC_MANDEL_COLOUR_EQUALISED without a GPU: mc_mandelbrot_equalise_map against the restatement bit for bit (tests/mandel_equalise_ref.py),
its properties and refusals, the motivating fact (a deep view's counts sit in a sliver of [0, M]; their ranks do not), the argument checks
of the device-level calls that need no device, the app's option handling, the exports."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mandel_equalise_ref as E
import mandel_perturb_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1


def check_map(B, hist, M):
    hist = np.asarray(hist, np.uint32)
    got = B.equalise_map(M, hist)
    want = E.rank_map(hist, M)
    assert got.dtype == np.uint32 and got.shape == (M + 1,)
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(want, E.rank_map_scalar(hist, M))
    assert (np.diff(got.astype(np.int64)) >= 0).all()          # non-decreasing
    assert got[M] == M
    occurs = hist[:M] > 0
    assert (got[:M][occurs] < M).all()                         # a count that occurs maps below M
    return got


def test_enum_value(B):
    assert B.MANDEL_COLOUR_EQUALISED == 16
    text = open(B.HEADER_PATH).read()
    assert "MC_MANDEL_COLOUR_EQUALISED = 1u << 4" in text


def test_symbols_declared_and_exported(B):
    names = B.declared_symbols()
    for s in ("mc_mandelbrot_histogram_device_async", "mc_mandelbrot_equalise_map", "mc_mandelbrot_recolour_device_async"):
        assert s in names and hasattr(B.lib(), s)


@pytest.fixture(scope="module")
def k4_plane():
    """K4's view (scale 1e-8 by 2/3 of it, M = 50 000) restated on the CPU at 96 x 64."""
    M, W, H = 50000, 96, 64
    scale = (1e-8, 1e-8 * 2.0 / 3.0)
    L, z = R.mp_orbit(R.DEEP_CENTRE[0], R.DEEP_CENTRE[1], M, R.orbit_bits(*scale))
    Z = np.array([[float(a), float(b)] for a, b in z], np.float64)
    return R.plane(Z, L, W, H, M, scale), M


def test_map_of_a_restated_plane(B, k4_plane):
    n, M = k4_plane
    hist = E.histogram(n, M)
    assert np.array_equal(hist, E.histogram_scalar(n, M)) and int(hist.sum()) == n.size
    check_map(B, hist, M)


def test_motivating_fact(B, k4_plane):
    """The plain palette position n / M of 98 % of the pixels spans less than 0.02 of [0, 1]; the equalised one more than 0.9."""
    n, M = k4_plane
    m = B.equalise_map(M, E.histogram(n, M))
    plain = E.percentile_span(n.astype(np.float64) / M)
    equalised = E.percentile_span(m[n].astype(np.float64) / M)
    print(f"1st..99th percentile span: n / M {plain:.4f}, map[n] / M {equalised:.4f}; distinct counts {np.unique(n).size}, "
          f"distinct map values {np.unique(m[n]).size}")
    assert plain < 0.02
    assert equalised > 0.9
    assert np.unique(m[n]).size == np.unique(n).size            # the same number of distinct colours


def test_map_edge_cases(B):
    M = 100
    h = np.zeros(M + 1, np.uint32)
    h[M] = 6144                                                  # all interior: E = 0
    got = check_map(B, h, M)
    assert (got[:M] == 0).all()
    h = np.zeros(M + 1, np.uint32)
    h[37] = 6144                                                 # one escaped bin
    got = check_map(B, h, M)
    assert (got[:38] == 0).all() and (got[38:M] == M).all()
    got = check_map(B, [3, 5], 1)                                # M = 1
    assert list(got) == [0, 1]
    check_map(B, [0, 5], 1)
    got = check_map(B, np.ones(M + 1, np.uint32), M)             # every bin 1: the identity
    assert np.array_equal(got, np.arange(M + 1))
    for j in (0, 50, M - 1, M):                                  # a single pixel
        h = np.zeros(M + 1, np.uint32)
        h[j] = 1
        check_map(B, h, M)
    check_map(B, np.zeros(M + 1, np.uint32), M)                  # an empty histogram


def test_map_product_beyond_2_53(B):
    """M = 2^22, 2^32 - 2 pixels in bin 0 and one in bin M - 1: M * C(M - 1) is about 2^54, and the quotient's exactness decides
    map[M - 1] (an implementation that goes through a double misses it)."""
    M = 1 << 22
    h = np.zeros(M + 1, np.uint32)
    h[0] = 2 ** 32 - 2
    h[M - 1] = 1
    got = B.equalise_map(M, h)
    escaped = 2 ** 32 - 1
    assert int(got[0]) == 0 and int(got[M]) == M
    assert int(got[1]) == (M * (2 ** 32 - 2)) // escaped == int(got[M - 1])
    assert int(got[M - 1]) == M - 1
    want = np.full(M + 1, (M * (2 ** 32 - 2)) // escaped, np.uint32)
    want[0], want[M] = 0, M
    assert np.array_equal(got, want)
    h[3] = 1 << 20                                               # the total is 2^32 - 1 + 2^20: refused
    with pytest.raises(B.McError) as e:
        B.equalise_map(M, h)
    assert e.value.status == INVALID


def test_map_random(B):
    rng = np.random.default_rng(5)
    for M in (2, 3, 17, 1000, 65535, 200000):
        for _ in range(3):
            h = rng.integers(0, 1 << int(rng.integers(1, 14)), M + 1).astype(np.uint32)
            h[rng.random(M + 1) < rng.random()] = 0               # a skewed table: many empty bins
            check_map(B, h, M)
    h = rng.integers(0, 2 ** 32 // 1001, 1001).astype(np.uint32)   # a total just below 2^32
    check_map(B, h, 1000)


def test_map_refusals(B):
    L = B.lib()
    h = (C.c_uint32 * 4)(1, 2, 3, 4)
    m = (C.c_uint32 * 4)()
    assert L.mc_mandelbrot_equalise_map(3, None, m) == INVALID
    assert L.mc_mandelbrot_equalise_map(3, h, None) == INVALID
    assert L.mc_mandelbrot_equalise_map(0, h, m) == INVALID
    big = np.zeros(4, np.uint32)
    big[0] = big[1] = 2 ** 31                                     # the total is exactly 2^32
    with pytest.raises(B.McError) as e:
        B.equalise_map(3, big)
    assert e.value.status == INVALID and "2^32" in str(e.value)
    big[1] -= 1                                                   # 2^32 - 1 is accepted
    check_map(B, big, 3)
    big = np.zeros(4, np.uint32)
    big[3] = 2 ** 32 - 1
    big[0] = 1                                                    # interior pixels count towards the total too
    with pytest.raises(B.McError):
        B.equalise_map(3, big)


def test_device_calls_refuse_bad_arguments_without_a_device(B):
    L = B.lib()
    p = B.mandelbrot_params(8, 8, max_iter=10)
    buf = (C.c_uint32 * 64)()
    one = C.cast(buf, C.c_void_p)
    m = (C.c_uint32 * 11)()
    hist, rec = L.mc_mandelbrot_histogram_device_async, L.mc_mandelbrot_recolour_device_async
    assert hist(None, one, 4, 64, 10, one, None) == INVALID       # no context
    assert rec(None, C.byref(p), one, 4, m, one, None) == INVALID
    fake = C.c_void_p(1)   # never dereferenced: the argument checks come first
    assert hist(fake, None, 4, 64, 10, one, None) == INVALID
    assert hist(fake, one, 4, 64, 10, None, None) == INVALID
    assert hist(fake, one, 3, 64, 10, one, None) == INVALID
    assert hist(fake, one, 8, 64, 10, one, None) == INVALID
    assert hist(fake, one, 4, 64, 0, one, None) == INVALID
    assert rec(fake, None, one, 4, m, one, None) == INVALID
    assert rec(fake, C.byref(p), None, 4, m, one, None) == INVALID
    assert rec(fake, C.byref(p), one, 4, None, one, None) == INVALID
    assert rec(fake, C.byref(p), one, 4, m, None, None) == INVALID
    assert rec(fake, C.byref(p), one, 1, m, one, None) == INVALID
    p.max_iter = 0
    assert rec(fake, C.byref(p), one, 4, m, one, None) == INVALID


def app(name, *args, cwd):
    return subprocess.run([os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", name)] + list(args), capture_output=True, text=True,
                          cwd=cwd, timeout=60)


def test_app_colour_option(B, tmp_path):
    r = app("mandelbrot", "--colour", "rainbow", cwd=tmp_path)
    assert r.returncode == 1 and "--colour rainbow: not one of reference | equalised" in r.stdout
    assert "using device" not in r.stdout and not list(tmp_path.iterdir())
    r = app("mandelbrot", "--colour", cwd=tmp_path)
    assert r.returncode == 1 and "missing value for --colour" in r.stdout
    for word in ("reference", "equalised"):   # parsed and run up to the device: without a GPU init() fails with the device message
        r = app("mandelbrot", "--colour", word, "--width", "64", "--height", "48", "--quiet", cwd=tmp_path)
        assert "not one of" not in r.stdout and "unknown option" not in r.stdout
        assert (r.returncode == 0 and (tmp_path / "mandelbrot.png").exists()) or (r.returncode == 1 and "could not find a device" in r.stdout)
    r = app("pathtracer", "--colour", "equalised", cwd=tmp_path)
    assert r.returncode == 1 and "--colour: a Mandelbrot option" in r.stdout and not (tmp_path / "pathtracer.png").exists()
