"""MC_MANDEL_COLOUR_SMOOTH_EQUALISED without a GPU: mc_mandelbrot_smooth_equalise_map and mc_mandelbrot_smooth_remap against both
restatements bit for bit (tests/mandel_smooth_equalise_ref.py), the contract's four stated consequences, every refusal of the host calls,
the motivating fact on exact restatements of two views (more distinct colours than the integer rank, and the whole palette), the argument
checks of the device-level calls that need no device, the exports."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mandel_equalise_ref as E
import mandel_perturb_ref as R
import mandel_smooth_equalise_ref as Q
import mandel_smooth_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
LIMIT = S.MAX_ITER_LIMIT                                                  # 2^24 - 1


def check_map(B, hist, M, slow=True):
    """The library's knot map of hist against both restatements, and the contract's consequences that concern the map alone."""
    hist = np.asarray(hist, np.uint32)
    got = B.smooth_equalise_map(M, hist)
    want = Q.knot_map(hist, M)
    assert got.dtype == np.uint32 and got.shape == (M + 1,)
    assert np.array_equal(got, want), int((got != want).sum())
    if slow:
        assert np.array_equal(want, Q.knot_map_scalar(hist, M))
    assert (np.diff(got.astype(np.int64)) >= 0).all()                     # non-decreasing
    assert int(got[M]) == 256 * M
    occurs = hist[:M] > 0
    assert (got[:M][occurs] < 256 * M).all()                              # an occupied bin's knot lies below the interior's
    assert np.array_equal(got >> 8, B.equalise_map(M, hist))              # the integer rank map is the knots' integer part
    escaped = int(hist[:M].astype(np.uint64).sum())
    if escaped:                                                           # knot j within 1 / (256 M) of C(j) / E: exact integers
        below = np.concatenate(([0], np.cumsum(hist[:M].astype(object))))[:M]
        for j in np.unique(np.concatenate((np.flatnonzero(occurs)[:50], np.arange(min(M, 50)), [M - 1]))):
            c = int(below[j])
            # 0 <= C/E - qmap/(256 M) < 1/(256 M)  <=>  0 <= 256 M C - qmap E < E
            slack = 256 * M * c - int(got[j]) * escaped
            assert 0 <= slack < escaped, (j, slack)
    return got


def check_remap(B, qmap, M, q):
    """The library's remap of q against both restatements; monotone; escaped stays escaped where the map came from a histogram."""
    q = np.asarray(q, np.uint32)
    got = B.smooth_remap(M, qmap, q)
    assert got.dtype == np.uint32 and got.shape == q.shape
    assert np.array_equal(got, Q.remap(q, qmap, M))
    assert np.array_equal(got, Q.remap_scalar(q, qmap, M))
    order = np.argsort(q.reshape(-1), kind="stable")
    assert (np.diff(got.reshape(-1)[order].astype(np.int64)) >= 0).all()  # q' is non-decreasing in q
    assert (got[q == 256 * M] == 256 * M).all()
    return got


def check_plane(B, q, M):
    """Histogram, map and remap of one plane; an escaped pixel never reaches 256 M."""
    hist = Q.histogram(q, M)
    assert np.array_equal(hist, Q.histogram_scalar(q, M)) and int(hist.sum()) == q.size
    qmap = check_map(B, hist, M)
    inside = np.minimum(q, 256 * M)
    got = check_remap(B, qmap, M, inside)
    assert (got[q < 256 * M] < 256 * M).all()
    assert np.array_equal(got, Q.ranked(q, M))
    return got


def test_enum_value_and_symbols(B):
    assert B.MANDEL_COLOUR_SMOOTH_EQUALISED == 1 << 12
    text = open(B.HEADER_PATH).read()
    assert "MC_MANDEL_COLOUR_SMOOTH_EQUALISED = 1u << 12" in text and "#define MC_ABI_VERSION 3" in text
    names = B.declared_symbols()
    for s in ("mc_mandelbrot_render_smooth_equalised", "mc_mandelbrot_smooth_histogram_device_async", "mc_mandelbrot_smooth_equalise_map",
              "mc_mandelbrot_smooth_remap", "mc_mandelbrot_smooth_remap_device_async"):
        assert s in names and hasattr(B.lib(), s)


@pytest.mark.parametrize("M", [1, 2, 255, 4096])
def test_random_histograms(B, M):
    rng = np.random.default_rng(100 + M)
    for k in range(4):
        h = rng.integers(0, 1 << int(rng.integers(1, 20)), M + 1).astype(np.uint32)
        if k:
            h[rng.random(M + 1) < rng.random()] = 0                       # a skewed table: many empty bins
        qmap = check_map(B, h, M)
        q = rng.integers(0, 256 * M + 1, 3000).astype(np.uint32)
        q[:4] = (0, 255 if M > 0 else 0, 256 * M - 1, 256 * M)
        check_remap(B, qmap, M, q)
        check_remap(B, qmap, M, np.arange(min(256 * M + 1, 70000), dtype=np.uint32))   # every q of the first bins, in order


@pytest.mark.parametrize("M", [1, 2, 255, 4096])
def test_synthetic_planes(B, M):
    for name, q in Q.synthetic_planes(67, 35, M):
        got = check_plane(B, q, M)
        if name in ("interior", "above"):
            assert (got == 256 * M).all()


def test_m_equal_to_one(B):
    got = check_map(B, [3, 5], 1)
    assert list(got) == [0, 256]
    r = check_remap(B, got, 1, np.arange(257, dtype=np.uint32))
    assert np.array_equal(r, np.arange(257))                              # one bin spanning the palette: the identity
    check_map(B, [0, 5], 1)
    check_map(B, [7, 0], 1)


def test_no_escaped_pixel(B):
    M = 100
    h = np.zeros(M + 1, np.uint32)
    h[M] = 6144
    got = check_map(B, h, M)
    assert (got[:M] == 0).all()
    check_map(B, np.zeros(M + 1, np.uint32), M)                           # an empty histogram
    q = np.array([0, 255, 256 * 50 + 3, 256 * M - 256, 256 * M - 1, 256 * M], np.uint32)
    r = check_remap(B, got, M, q)
    # below the last bin every q' is 0; the last bin rises to the interior's knot, which it does not reach
    assert list(r[:3]) == [0, 0, 0] and r[3] == 0 and r[4] == (256 * M * 255) >> 8 and r[5] == 256 * M


def test_one_occupied_bin(B):
    M = 100
    h = np.zeros(M + 1, np.uint32)
    h[37] = 6144
    got = check_map(B, h, M)
    assert (got[:38] == 0).all() and (got[38:] == 256 * M).all()
    q = 256 * 37 + np.arange(256, dtype=np.uint32)
    r = check_remap(B, got, M, q)
    assert np.array_equal(r, (256 * M * np.arange(256)) >> 8)              # the bin's fractions spread over the whole palette
    assert r.max() < 256 * M


def test_more_escaped_pixels_than_palette_positions(B):
    """E > 256 M: neighbouring knots may coincide (a difference rounds to 0) and a bin's pixels then share one q'."""
    M = 4
    h = np.array([1, 5000, 1, 1, 9], np.uint32)
    got = check_map(B, h, M)
    assert int(h[:M].sum()) > 256 * M and got[0] == 0 and got[1] == 0 and got[2] == got[3] == 1023
    q = np.arange(256 * M + 1, dtype=np.uint32)
    r = check_remap(B, got, M, q)
    assert (r[:256] == 0).all() and (r[512:768] == 1023).all() and r[1023] < 1024


def test_total_at_the_limit(B):
    M = 3
    h = np.array([2 ** 31, 2 ** 31 - 1, 0, 0], np.uint32)                 # 2^32 - 1 escaped
    check_map(B, h, M)
    h = np.array([2 ** 32 - 2, 0, 1, 0], np.uint32)
    got = check_map(B, h, M)
    assert int(got[1]) == int(got[2]) == (768 * (2 ** 32 - 2)) // (2 ** 32 - 1) == 767
    h = np.array([1, 0, 0, 2 ** 32 - 2], np.uint32)                       # interior pixels count towards the total
    check_map(B, h, M)
    for bad in ([2 ** 31, 2 ** 31, 0, 0], [1, 0, 0, 2 ** 32 - 1]):
        with pytest.raises(B.McError) as e:
            B.smooth_equalise_map(M, np.array(bad, np.uint32))
        assert e.value.status == INVALID and "2^32" in str(e.value)


def test_largest_max_iter_with_a_sparse_histogram(B):
    """M = 2^24 - 1: 256 M C(j) passes 2^63 (an implementation in signed or floating arithmetic misses the quotient)."""
    M = LIMIT
    h = np.zeros(M + 1, np.uint32)
    h[5] = 2 ** 32 - 4
    h[1 << 20] = 2
    h[M - 1] = 1
    h[M] = 0
    got = B.smooth_equalise_map(M, h)
    E_ = 2 ** 32 - 1
    assert int(got[5]) == 0 and int(got[6]) == (256 * M * (2 ** 32 - 4)) // E_ == int(got[1 << 20])
    assert int(got[(1 << 20) + 1]) == (256 * M * (2 ** 32 - 2)) // E_ == int(got[M - 1]) and int(got[M]) == 256 * M
    assert 256 * M * (2 ** 32 - 2) > 2 ** 63
    assert (np.diff(got.astype(np.int64)) >= 0).all()
    assert np.array_equal(got >> 8, B.equalise_map(M, h))
    q = np.array([0, 256 * 5, 256 * 5 + 255, 256 * 6, 256 * (1 << 20) + 128, 256 * (M - 1) + 255, 256 * M], np.uint32)
    r = B.smooth_remap(M, got, q)
    assert np.array_equal(r, Q.remap_scalar(q, got, M)) and np.array_equal(r, Q.remap(q, got, M))
    assert (r[:-1] < 256 * M).all() and r[-1] == 256 * M


def test_host_refusals(B):
    L = B.lib()
    M = 3
    h = (C.c_uint32 * 4)(1, 2, 3, 4)
    m = (C.c_uint32 * 4)()
    fn = L.mc_mandelbrot_smooth_equalise_map
    assert fn(M, None, m) == INVALID and fn(M, h, None) == INVALID and fn(0, h, m) == INVALID and fn(LIMIT + 1, h, m) == INVALID
    assert fn(M, h, m) == 0 and list(m) == [0, 128, 384, 768]
    rm = L.mc_mandelbrot_smooth_remap
    q = (C.c_uint32 * 2)(5, 768)
    out = (C.c_uint32 * 2)()
    assert rm(M, m, q, 2, out) == 0 and list(out) == [(128 * 5) >> 8, 768]
    assert rm(M, m, None, 0, None) == 0                                   # nothing to do
    assert rm(0, m, q, 2, out) == INVALID and rm(LIMIT + 1, m, q, 2, out) == INVALID
    assert rm(M, None, q, 2, out) == INVALID and rm(M, m, None, 2, out) == INVALID and rm(M, m, q, 2, None) == INVALID
    with pytest.raises(B.McError) as e:
        B.smooth_remap(M, list(m), [0, 769])                              # a q above 256 M
    assert e.value.status == INVALID and "above 256 * max_iter" in str(e.value)
    for bad, word in (([0, 200, 100, 768], "decrease"), ([0, 900, 900, 768], "above 256 * max_iter"), ([0, 128, 384, 767], "qmap[max_iter]"),
                      ([0, 128, 384, 769], "qmap[max_iter]"), ([769, 769, 769, 768], "above 256 * max_iter")):
        with pytest.raises(B.McError) as e:
            B.smooth_remap(M, bad, [0])
        assert e.value.status == INVALID and word in str(e.value), (bad, str(e.value))


def test_device_calls_refuse_bad_arguments_without_a_device(B):
    L = B.lib()
    p = B.mandelbrot_params(8, 8, max_iter=10, flags=B.MANDEL_COLOUR_SMOOTH_EQUALISED)
    buf = (C.c_uint32 * 64)()
    one = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(one.value + 2)
    m = (C.c_uint32 * 11)(*[256 * j for j in range(11)])
    hist, rem, whole = L.mc_mandelbrot_smooth_histogram_device_async, L.mc_mandelbrot_smooth_remap_device_async, L.mc_mandelbrot_render_smooth_equalised
    fake = C.c_void_p(1)   # never dereferenced: the argument checks come first
    assert hist(None, one, 64, 10, one, None) == INVALID
    assert hist(fake, None, 64, 10, one, None) == INVALID and hist(fake, one, 64, 10, None, None) == INVALID
    assert hist(fake, one, 64, 0, one, None) == INVALID and hist(fake, one, 64, LIMIT + 1, one, None) == INVALID
    assert hist(fake, one, 2 ** 32, 10, one, None) == INVALID and "2^32" in L.mc_last_error_detail().decode()
    assert hist(fake, odd, 64, 10, one, None) == INVALID and hist(fake, one, 64, 10, odd, None) == INVALID
    assert rem(None, C.byref(p), one, m, one, one, None) == INVALID
    assert rem(fake, None, one, m, one, one, None) == INVALID and rem(fake, C.byref(p), None, m, one, one, None) == INVALID
    assert rem(fake, C.byref(p), one, None, one, one, None) == INVALID and rem(fake, C.byref(p), one, m, None, None, None) == INVALID
    plain = B.mandelbrot_params(8, 8, max_iter=10)
    assert rem(fake, C.byref(plain), one, m, one, one, None) == INVALID
    assert "must carry MC_MANDEL_COLOUR_SMOOTH_EQUALISED" in L.mc_last_error_detail().decode()
    both = B.mandelbrot_params(8, 8, max_iter=10, flags=B.MANDEL_COLOUR_SMOOTH_EQUALISED | B.MANDEL_COLOUR_SMOOTH)
    assert rem(fake, C.byref(both), one, m, one, one, None) == INVALID and "MC_MANDEL_COLOUR_SMOOTH " in L.mc_last_error_detail().decode()
    assert whole(None, C.byref(p), one, None, None, None) == INVALID and whole(fake, None, one, None, None, None) == INVALID
    assert whole(fake, C.byref(p), None, None, None, None) == INVALID
    assert whole(fake, C.byref(plain), one, None, None, None) == INVALID
    assert "must carry MC_MANDEL_COLOUR_SMOOTH_EQUALISED" in L.mc_last_error_detail().decode()
    # MC_MANDEL_COLOUR_SMOOTH | MC_MANDEL_COLOUR_EQUALISED without the new flag stays refused, and still names the integer flag
    old = B.mandelbrot_params(8, 8, max_iter=10, flags=B.MANDEL_COLOUR_SMOOTH | B.MANDEL_COLOUR_EQUALISED)
    assert L.mc_mandelbrot_render_device_async(fake, C.byref(old), one, None, None) == INVALID
    assert "MC_MANDEL_COLOUR_EQUALISED" in L.mc_last_error_detail().decode()
    assert B.supersample_params(B.mandelbrot_params(8, 8, max_iter=10, flags=B.MANDEL_COLOUR_SMOOTH_EQUALISED, supersample=2)).flags \
        & B.MANDEL_COLOUR_SMOOTH_EQUALISED


# ---- the motivating fact, on exact restatements ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reference_plane(O):
    """(q, n, M): the reference view in MC_PRECISION_F32 at 400 x 400, M = 128."""
    W, H, M = 400, 400, 128
    n, zx, zy, cx, cy = S.f32_capture(W, H, M)
    return S.smooth_count(O, n, M, zx, zy, cx, cy), n, M


@pytest.fixture(scope="module")
def k4_plane(O):
    """(q, n, M): K4's view (scale 1e-8 by 2/3 of it, M = 50 000) in float64 perturbation arithmetic at 96 x 64, the plane
    tests/test_mandel_equalise_host.py restates, with its escape states."""
    M, W, H = 50000, 96, 64
    scale = (1e-8, 1e-8 * 2.0 / 3.0)
    L, z = R.mp_orbit(R.DEEP_CENTRE[0], R.DEEP_CENTRE[1], M, R.orbit_bits(*scale))
    Z = np.array([[float(a), float(b)] for a, b in z], np.float64)
    n, zx, zy, cx, cy = S.perturb_plane_capture(R, Z, L, W, H, M, scale)
    assert np.array_equal(n, R.plane(Z, L, W, H, M, scale))
    return S.smooth_count(O, n, M, zx, zy, cx, cy), n, M


@pytest.mark.parametrize("view", ["reference", "k4"])
def test_motivating_fact(B, view, reference_plane, k4_plane):
    """Smooth equalised colouring draws strictly more distinct palette positions than the integer rank, and its 1st..99th percentile span
    is at least 0.9 of the palette, where plain smooth colouring sits in a sliver on the deep view.  0.9 is a floor under the reference
    restatement (DESIGN.md section 3.21 quotes the values printed here), not under the library."""
    q, n, M = reference_plane if view == "reference" else k4_plane
    want = Q.ranked(q, M)
    got = check_plane(B, q, M)                                           # the library's map and remap are the restatement's
    integer = E.rank_map(E.histogram(n, M), M)[np.minimum(n, M)]
    esc = q < 256 * M                                                     # the spans over the escaped pixels, and over every pixel
    spans = {}
    for name, t in (("smooth equalised", want / (256.0 * M)), ("smooth", q / (256.0 * M)), ("integer equalised", integer / float(M))):
        spans[name] = (E.percentile_span(t[esc]), E.percentile_span(t))
    distinct_eq, distinct_int, distinct_q = np.unique(want).size, np.unique(integer).size, np.unique(q).size
    print(f"{view}: distinct q' {distinct_eq}, distinct q {distinct_q}, distinct integer ranks {distinct_int}; 1st..99th percentile span "
          "(escaped pixels / all pixels): " + ", ".join(f"{k} {a:.4f} / {b:.4f}" for k, (a, b) in spans.items()))
    assert distinct_eq > distinct_int
    assert min(spans["smooth equalised"]) >= 0.9
    assert np.array_equal(got, want)


def app(name, *args, cwd):
    return subprocess.run([os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", name)] + list(args), capture_output=True, text=True,
                          cwd=cwd, timeout=60)


def test_app_colour_option(tmp_path):
    r = app("mandelbrot", "--colour", "smooth-equalized", cwd=tmp_path)   # (the spelling is the library's)
    assert r.returncode == 1 and "not one of reference | equalised" in r.stdout and "smooth-equalised" in r.stdout
    r = app("mandelbrot", "--colour", "smooth-equalised", "--width", "64", "--height", "48", "--quiet", cwd=tmp_path)
    assert "not one of" not in r.stdout and "unknown option" not in r.stdout
    assert (r.returncode == 0 and (tmp_path / "mandelbrot.png").exists()) or (r.returncode == 1 and "could not find a device" in r.stdout)
    r = app("mandelbrot", "--colour", "smooth-equalised", "--supersample", "2", "--width", "64", "--height", "48", cwd=tmp_path)
    assert r.returncode == 1 and "--colour smooth-equalised" in r.stdout
