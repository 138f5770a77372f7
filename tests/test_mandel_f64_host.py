"""MC_PRECISION_F64 on the CPU: the numpy restatement the GPU tests compare against (tests/mandel_f64_ref.py) checked against a scalar
loop on Python floats, the enum value in the header and the bindings, and the proof that the deep view the GPU tests render tells F64
from the two-float variant (so a kernel that rendered F64 as DS could not pass them)."""
import os
import re

import numpy as np

import mandel_f64_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scalar_plane(W, H, M, centre, scale, pixels):
    cxv, cyv, sxv, syv = R.view_words(centre, scale)
    cx, cy = R.c_axis(W, cxv, sxv), R.c_axis(H, cyv, syv)
    return np.array([R.scalar_iters(float(cx[gx]), float(cy[gy]), M) for gx, gy in pixels], np.uint32)


def test_restatement_matches_scalar_loop():
    rng = np.random.default_rng(7)
    # the reference view (escapes, boundary, interior pixels running to M) and K4's centre at a deep scale
    for W, H, M, centre, scale in ((64, 48, 300, (-0.445, 0.0), (2.34, 2.34)),
                                   (40, 30, 3000, R.DEEP_CENTRE, (1e-10, 0.75e-10))):
        plane = R.mandelbrot_iters_f64(W, H, M, centre, scale)
        pixels = [(int(x), int(y)) for x, y in zip(rng.integers(0, W, 24), rng.integers(0, H, 24))]
        inside = np.argwhere(plane == M)
        pixels += [(int(x), int(y)) for y, x in inside[:4]]
        got = plane[[y for _, y in pixels], [x for x, _ in pixels]]
        assert np.array_equal(got, _scalar_plane(W, H, M, centre, scale, pixels)), (centre, scale)
    assert (R.mandelbrot_iters_f64(64, 48, 300, (-0.445, 0.0), (2.34, 2.34)) == 300).any()


def test_magnitude_exactly_two():
    """Even W and H put c = centre at pixel (W/2, H/2).  c = (1, 1): the first |z|^2 is 2.0 exactly, which does not escape, so n = 1.
    c = (0, 1): the orbit i, -1+i, -i, -1+i, ... meets |z|^2 = 2.0 exactly every other iteration and never escapes (n = M) — the
    fp64 fast filter's only false positive, met again in every block."""
    W, H, M = 16, 12, 100
    for centre, want in (((1.0, 1.0), 1), ((0.0, 1.0), M)):
        plane = R.mandelbrot_iters_f64(W, H, M, centre, (1e-3, 1e-3))
        cxv, cyv, sxv, syv = R.view_words(centre, (1e-3, 1e-3))
        assert R.c_axis(W, cxv, sxv)[W // 2] == centre[0] and R.c_axis(H, cyv, syv)[H // 2] == centre[1]
        assert plane[H // 2, W // 2] == want == R.scalar_iters(centre[0], centre[1], M)


def test_view_words_are_exact():
    """hi = (float)d, lo = (float)(d - hi): hi + lo in double is exact, and recovers d to ~48 bits."""
    for d in (R.DEEP_CENTRE + (1e-8, 1e-12, 2.34, -0.445)):
        hi, lo = R.split_double(d)
        s = np.float64(hi) + np.float64(lo)
        assert s - np.float64(hi) == np.float64(lo)
        assert abs(s - d) <= abs(d) * 2.0 ** -47


def test_precision_value_in_bindings_and_header(B):
    assert (B.PRECISION_F32, B.PRECISION_DS, B.PRECISION_F64) == (0, 1, 2)
    with open(os.path.join(ROOT, "include", "mc_compute.h")) as f:
        hdr = f.read()
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(MC_PRECISION_\w+)\s*=\s*(\d+)", hdr))
    assert enum == {"MC_PRECISION_F32": 0, "MC_PRECISION_DS": 1, "MC_PRECISION_F64": 2}


def test_deep_view_tells_f64_from_ds(O):
    """K4's centre at 64 x 48, M = 20 000, scale 1e-12: the two-float plane (the existing oracle) differs from the F64 plane in ~46 % of
    the pixels.  The GPU tests render this view and compare with the F64 plane, so an F64 request served by the DS kernel fails them."""
    W, H, M, scale = 64, 48, 20000, (1e-12, 0.75e-12)
    f64 = R.mandelbrot_iters_f64(W, H, M, R.DEEP_CENTRE, scale)
    ds = O.mandelbrot_iters(W, H, M, view=O.make_view(R.DEEP_CENTRE[0], R.DEEP_CENTRE[1], *scale), precision=1)
    assert (f64 != ds).mean() > 0.3
