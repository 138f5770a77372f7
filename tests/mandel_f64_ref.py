"""Restatement of MC_PRECISION_F64 (include/mc_compute.h) in numpy float64, the reference plane of the fp64 Mandelbrot tests.

Every operation is its own ufunc on float64 arrays: IEEE double, correctly rounded, never contracted into an fma — the contract the
kernel is built to (-ffp-contract=off).  The loop is compacted to the pixels that are still running, so a view whose pixels mostly
escape early costs little; pixels inside the set still cost M iterations each.  Not a conftest: the test files import it."""
import numpy as np

DEEP_CENTRE = (-0.7436438870371587, 0.13182590420531198)   # K4's centre (bench.K4_VIEW)


def split_double(d):
    """The (hi, lo) float words of a view value, as the bindings and the app pack them (hi = (float)d, lo = (float)(d - hi))."""
    hi = np.float32(d)
    lo = np.float32(np.float64(d) - np.float64(hi))
    return hi, lo


def view_words(centre, scale):
    """(centre_x, centre_y, scale_x, scale_y) as the doubles F64 reads: (double)hi + (double)lo of each packed value."""
    out = []
    for d in (centre[0], centre[1], scale[0], scale[1]):
        hi, lo = split_double(d)
        out.append(np.float64(hi) + np.float64(lo))
    return tuple(out)


def c_axis(n, centre, scale, idx=None):
    """c along one axis: x = double(g) / double(n), c = centre + (x - 0.5) * scale."""
    g = np.arange(n, dtype=np.float64) if idx is None else np.asarray(idx, dtype=np.float64)
    x = g / np.float64(n)
    t = x - np.float64(0.5)
    t = t * np.float64(scale)
    return np.float64(centre) + t


def iterate(cx, cy, max_iter):
    """n per pixel for flat float64 arrays cx, cy: the number of iterations that did not escape, in [0, max_iter]."""
    cx = np.ascontiguousarray(cx, np.float64).ravel()
    cy = np.ascontiguousarray(cy, np.float64).ravel()
    n = np.full(cx.shape, max_iter, np.uint32)
    live = np.arange(cx.size)
    zx = np.zeros_like(cx); zy = np.zeros_like(cx); sx = np.zeros_like(cx); sy = np.zeros_like(cx)
    two = np.float64(2.0)
    for i in range(max_iter):
        nzx = sx - sy
        nzx = nzx + cx
        nzy = two * zx
        nzy = nzy * zy
        nzy = nzy + cy
        zx, zy = nzx, nzy
        sx = zx * zx
        sy = zy * zy
        esc = (sx + sy) > two
        if esc.any():
            n[live[esc]] = i
            keep = ~esc
            live, cx, cy, zx, zy, sx, sy = live[keep], cx[keep], cy[keep], zx[keep], zy[keep], sx[keep], sy[keep]
            if live.size == 0:
                break
    return n


def mandelbrot_iters_f64(W, H, max_iter, centre, scale, rows=None):
    """The (len(rows), W) uint32 plane of MC_PRECISION_F64 for the image rows `rows` (default: all H)."""
    cxv, cyv, sxv, syv = view_words(centre, scale)
    rows = np.arange(H) if rows is None else np.asarray(rows)
    cx = c_axis(W, cxv, sxv)
    cy = c_axis(H, cyv, syv, idx=rows)
    CX = np.broadcast_to(cx[None, :], (rows.size, W))
    CY = np.broadcast_to(cy[:, None], (rows.size, W))
    return iterate(CX, CY, max_iter).reshape(rows.size, W)


def scalar_iters(cx, cy, max_iter):
    """The same loop on Python floats (IEEE doubles), one pixel: an independent statement of the contract."""
    zx = zy = sx = sy = 0.0
    for i in range(max_iter):
        nzx = (sx - sy) + cx
        nzy = ((2.0 * zx) * zy) + cy
        zx, zy = nzx, nzy
        sx, sy = zx * zx, zy * zy
        if sx + sy > 2.0:
            return i
    return max_iter
