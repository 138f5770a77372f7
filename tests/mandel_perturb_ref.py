"""Restatements of MC_PRECISION_PERTURB (include/mc_compute.h), the reference planes of the perturbation tests, and mpmath ground truth.

- `iterate` / `plane`: numpy float64, one ufunc per operation (IEEE double, never contracted into an fma: the kernel's contract), compacted
  to the pixels still running, fed an orbit table Z_0 .. Z_L (the library's own Orbit.table(), or `mp_orbit`'s).
- `scalar_iters`: the same loop on Python floats, one pixel: an independent statement of the contract.
- `mp_orbit` / `mp_iters`: mpmath at a given binary precision: the reference orbit, and c = c_ref + dc iterated directly (the truth the
  perturbation has to reproduce).  `mp_boundary_point`: a point of the set's boundary by bisection, for deep views with a spread of counts.
Not a conftest: the test files import it."""
import math

import mpmath
import numpy as np

DEEP_CENTRE = ("-0.7436438870371587", "0.13182590420531198")   # K4's centre (bench.K4_VIEW) as text


def dc_axis(n, scale, idx=None):
    """The pixel offsets along one axis: ((double)g / (double)n - 0.5) * scale."""
    g = np.arange(n, dtype=np.float64) if idx is None else np.asarray(idx, dtype=np.float64)
    t = g / np.float64(n)
    t = t - np.float64(0.5)
    return t * np.float64(scale)


def iterate(Z, L, dcx, dcy, max_iter):
    """n per pixel for flat float64 offset arrays dcx, dcy against the orbit table Z ((L+1, 2) float64)."""
    Zx = np.ascontiguousarray(Z[:, 0], np.float64)
    Zy = np.ascontiguousarray(Z[:, 1], np.float64)
    dcx = np.ascontiguousarray(dcx, np.float64).ravel().copy()
    dcy = np.ascontiguousarray(dcy, np.float64).ravel().copy()
    n = np.full(dcx.shape, max_iter, np.uint32)
    live = np.arange(dcx.size)
    dx = np.zeros_like(dcx); dy = np.zeros_like(dcx); m = np.zeros(dcx.shape, np.int64)
    two = np.float64(2.0)
    for i in range(max_iter):
        zmx = Zx[m]; zmy = Zy[m]
        ax = zmx + zmx
        ax = ax + dx
        ay = zmy + zmy
        ay = ay + dy
        ndx = ax * dx
        t = ay * dy
        ndx = ndx - t
        ndx = ndx + dcx
        ndy = ax * dy
        t = ay * dx
        ndy = ndy + t
        ndy = ndy + dcy
        m = m + 1
        zx = Zx[m] + ndx
        zy = Zy[m] + ndy
        r = zx * zx
        t = zy * zy
        r = r + t
        esc = r > two
        d2 = ndx * ndx
        t = ndy * ndy
        d2 = d2 + t
        reb = (m == L) | (r < d2)
        dx = np.where(reb, zx, ndx)
        dy = np.where(reb, zy, ndy)
        m = np.where(reb, 0, m)
        if esc.any():
            n[live[esc]] = i
            keep = ~esc
            live, dcx, dcy, dx, dy, m = live[keep], dcx[keep], dcy[keep], dx[keep], dy[keep], m[keep]
            if live.size == 0:
                break
    return n


def plane(Z, L, W, H, max_iter, scale, rows=None, cols=None):
    """The (len(rows), len(cols)) uint32 plane of MC_PRECISION_PERTURB for image rows `rows` and columns `cols` (default: all)."""
    rows = np.arange(H) if rows is None else np.asarray(rows)
    cols = np.arange(W) if cols is None else np.asarray(cols)
    dx = dc_axis(W, scale[0], idx=cols)
    dy = dc_axis(H, scale[1], idx=rows)
    DX = np.broadcast_to(dx[None, :], (rows.size, cols.size))
    DY = np.broadcast_to(dy[:, None], (rows.size, cols.size))
    return iterate(Z, L, DX, DY, max_iter).reshape(rows.size, cols.size)


def scalar_iters(Z, L, dcx, dcy, max_iter, stats=None):
    """The loop of include/mc_compute.h on Python floats, one pixel.  stats (a dict), when given, counts the rebases by kind:
    "rebase_end" (the orbit's end, m == L) and "rebase_near" (|z| < |d|)."""
    dx = dy = 0.0
    m = 0
    for i in range(max_iter):
        ax = (Z[m][0] + Z[m][0]) + dx
        ay = (Z[m][1] + Z[m][1]) + dy
        ndx = ((ax * dx) - (ay * dy)) + dcx
        ndy = ((ax * dy) + (ay * dx)) + dcy
        m = m + 1
        zx = Z[m][0] + ndx
        zy = Z[m][1] + ndy
        r = (zx * zx) + (zy * zy)
        if r > 2.0:
            return i
        if m == L or r < ((ndx * ndx) + (ndy * ndy)):
            if stats is not None:
                key = "rebase_end" if m == L else "rebase_near"
                stats[key] = stats.get(key, 0) + 1
            dx, dy, m = zx, zy, 0
        else:
            dx, dy = ndx, ndy
    return max_iter


def orbit_bits(scale_x, scale_y):
    """The fractional bits of the library's orbit arithmetic: max(64, ceil(-log2 min(|sx|, |sy|)) + 96)."""
    _, e = math.frexp(min(abs(scale_x), abs(scale_y)))
    return max(64, 1 - e + 96)


def mp_orbit(cx, cy, max_iter, prec):
    """(L, [(re, im) as mpf, ...] Z_0 .. Z_L) with mpmath at `prec` bits: L = first j >= 1 with |Z_j|^2 > 2, or max_iter."""
    with mpmath.workprec(prec):
        cx, cy = mpmath.mpf(cx), mpmath.mpf(cy)
        zx = zy = mpmath.mpf(0)
        out = [(zx, zy)]
        for j in range(max_iter):
            zx, zy = zx * zx - zy * zy + cx, 2 * zx * zy + cy
            out.append((zx, zy))
            if zx * zx + zy * zy > 2:
                return j + 1, out
        return max_iter, out


def _fixed(v, prec):
    """v (mpf, text or float) as an integer multiple of 2^-prec (nearest)."""
    with mpmath.workprec(prec + 64):
        return int(mpmath.nint(mpmath.mpf(v) * mpmath.mpf(2) ** prec))


def mp_iters(cx, cy, max_iter, prec):
    """n for c = (cx, cy) (mpf, text or float) iterated directly at `prec` fractional bits: the iterations with |z|^2 <= 2, as the kernel
    counts them.  c is rounded once by mpmath; the loop runs on Python integers (fixed point, products truncated: error 2^-prec per
    operation), far faster than mpf arithmetic at the same precision."""
    cx, cy = _fixed(cx, prec), _fixed(cy, prec)
    two = 2 << prec
    zx = zy = 0
    sx = sy = 0
    for i in range(max_iter):
        zx, zy = sx - sy + cx, ((zx * zy) >> (prec - 1)) + cy
        sx, sy = (zx * zx) >> prec, (zy * zy) >> prec
        if sx + sy > two:
            return i
    return max_iter


def pixel_c(centre, scale, W, H, gx, gy, prec):
    """c of pixel (gx, gy) as the kernel defines it: c_ref + dc, where c_ref is the decimal centre (exact here; the library's fixed
    point is within 2^-bits of it) and dc the double offsets of dc_axis."""
    dcx = float(dc_axis(W, scale[0], idx=[gx])[0])
    dcy = float(dc_axis(H, scale[1], idx=[gy])[0])
    with mpmath.workprec(prec):
        return mpmath.mpf(centre[0]) + mpmath.mpf(dcx), mpmath.mpf(centre[1]) + mpmath.mpf(dcy)


def escape_margin(cx, cy, max_iter, prec):
    """(n, |z|^2 - 2 at the escape) for c = (cx, cy) iterated as mp_iters does, or (max_iter, None) when it does not escape."""
    cx, cy = _fixed(cx, prec), _fixed(cy, prec)
    two = 2 << prec
    zx = zy = 0
    sx = sy = 0
    for i in range(max_iter):
        zx, zy = sx - sy + cx, ((zx * zy) >> (prec - 1)) + cy
        sx, sy = (zx * zx) >> prec, (zy * zy) >> prec
        if sx + sy > two:
            return i, math.ldexp(float((sx + sy - two) >> max(prec - 1000, 0)), -min(prec, 1000))
    return max_iter, None


def mp_boundary_point(inside, outside, max_iter, steps, prec, margin=1e-6):
    """Bisection on the segment inside -> outside (pairs of text) between "does not escape within max_iter" and "escapes": after `steps`
    halvings the ends lie within 2^-steps of the boundary of that set, and a view of about that scale around the point returned (some
    such lengths outside) has a spread of counts; its own orbit escapes (L < max_iter).  Returned as exact decimal text (a dyadic rational
    has a finite decimal expansion).
    The ends escape at the last iteration with |z|^2 a hair above 2.  A reference orbit on that hair is the known failure of the method
    (include/mc_compute.h): double precision cannot decide its last comparison, so every pixel that follows the reference gets it wrong.
    The point returned lies 7, 14, 28, ... segment lengths outward, the first whose own escape clears 2 by at least `margin`."""
    with mpmath.workprec(prec):
        a = [mpmath.mpf(v) for v in inside]
        b = [mpmath.mpf(v) for v in outside]
        for _ in range(steps):
            mid = [(a[0] + b[0]) / 2, (a[1] + b[1]) / 2]
            if mp_iters(mid[0], mid[1], max_iter, prec) >= max_iter:
                a = mid
            else:
                b = mid
        k = 7
        while True:
            c = [b[0] + k * (b[0] - a[0]), b[1] + k * (b[1] - a[1])]
            _, m = escape_margin(c[0], c[1], max_iter, prec)
            if m is not None and m >= margin:
                return tuple(mpmath.nstr(v, prec, strip_zeros=True, min_fixed=-math.inf, max_fixed=math.inf) for v in c)
            k *= 2
            if k > 1 << 40:
                raise RuntimeError("mp_boundary_point: no point clear of the escape threshold along the segment")


def mp_hair_point(inside, outside, max_iter, steps, prec):
    """The outside end of the same bisection, unmoved: its orbit escapes at the last iteration with |z|^2 - 2 far below double
    rounding — a reference on the hair (the known failure of the method)."""
    with mpmath.workprec(prec):
        a = [mpmath.mpf(v) for v in inside]
        b = [mpmath.mpf(v) for v in outside]
        for _ in range(steps):
            mid = [(a[0] + b[0]) / 2, (a[1] + b[1]) / 2]
            if mp_iters(mid[0], mid[1], max_iter, prec) >= max_iter:
                a = mid
            else:
                b = mid
        return tuple(mpmath.nstr(v, prec, strip_zeros=True, min_fixed=-math.inf, max_fixed=math.inf) for v in b)
