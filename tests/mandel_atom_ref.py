"""Restatements of the atom-domain calls (include/mc_compute.h, "atom domains"): the reference planes and values of the atom tests.

- `scan`: the update on Python floats over a sequence z_1 .. z_n: best = +inf, period = 0; (a_m, m) is taken when a_m < best, strictly,
  a_m = max(|x_m|, |y_m|); a NaN part never updates.
- `direct_planes`: (n, period, amin) of the F32 / F64 loop in numpy, one ufunc per operation (never contracted), EVERY pixel iterated to
  max_iter with no cycle exit and no compaction: an escaped pixel is frozen, not dropped.  The kernels keep their cycle exit; a test holds
  them to this.
- `perturb_planes`: the same for MC_PRECISION_PERTURB over an orbit table.
- `domains`: the three tables of a period plane and its amin plane, by numpy.
- `refine`: mc_mandelbrot_nucleus_refine on Python floats (IEEE doubles), operation for operation.
- `offset_text`: mc_mandelbrot_orbit_offset_text on Python Fractions.
Not a conftest: the test files import it."""
import math
from fractions import Fraction

import numpy as np

INF_BITS = 0x7FF0000000000000
NO_PIXEL = 0xFFFFFFFF


def scan(z):
    """(period, amin) of z_1 .. z_n, a sequence of (re, im) pairs."""
    best, period = math.inf, 0
    for m, (x, y) in enumerate(z, start=1):
        ax, ay = abs(float(x)), abs(float(y))
        a = ax if ax > ay else ay
        if ax < best and ay < best:
            best, period = a, m
    return period, best


def _update(best, period, m, x, y, live):
    """The vector form of the update: x, y float64 arrays (exact conversions of the state's z), live = not yet escaped."""
    ax, ay = np.abs(x), np.abs(y)
    a = np.where(ax > ay, ax, ay)
    take = live & (ax < best) & (ay < best)
    return np.where(take, a, best), np.where(take, np.uint32(m), period)


def direct_planes(cx, cy, max_iter, dtype):
    """(n uint32, period uint32, amin float64) for arrays cx, cy of `dtype` (np.float32: F32's loop, np.float64: F64's), same shape out."""
    shape = np.shape(cx)
    cx, cy = np.ascontiguousarray(cx, dtype).ravel(), np.ascontiguousarray(cy, dtype).ravel()
    n = np.full(cx.shape, max_iter, np.uint32)
    live = np.ones(cx.shape, bool)
    best, period = np.full(cx.shape, np.inf, np.float64), np.zeros(cx.shape, np.uint32)
    zx = np.zeros_like(cx); zy = np.zeros_like(cx); sx = np.zeros_like(cx); sy = np.zeros_like(cx)
    two = dtype(2.0)
    with np.errstate(all="ignore"):
        for i in range(max_iter):
            nzx = sx - sy
            nzx = nzx + cx
            nzy = two * zx
            nzy = nzy * zy
            nzy = nzy + cy
            zx, zy = nzx, nzy
            sx = zx * zx
            sy = zy * zy
            esc = ((sx + sy) > two) & live
            n[esc] = i
            live = live & ~esc
            best, period = _update(best, period, i + 1, zx.astype(np.float64), zy.astype(np.float64), live)
            if not live.any():
                break
    return n.reshape(shape), period.reshape(shape), best.reshape(shape)


def f32_axis(n, centre_hi, scale_hi, idx=None):
    """F32's c along one axis, in fp32 source order: u = float(g) / float(n); c = centre + (u - 0.5) * scale (the hi words only)."""
    g = np.arange(n, dtype=np.float32) if idx is None else np.asarray(idx, dtype=np.float32)
    u = g / np.float32(n)
    t = u - np.float32(0.5)
    t = t * np.float32(scale_hi)
    return np.float32(centre_hi) + t


def perturb_planes(Z, L, dcx, dcy, max_iter):
    """(n, period, amin) of MC_PRECISION_PERTURB for float64 offset arrays against the orbit table Z ((L + 1, 2) float64).  z_m is the z
    the iteration tested: Z[m] + nd, which after a rebase is the new d itself."""
    shape = np.shape(dcx)
    Zx, Zy = np.ascontiguousarray(Z[:, 0], np.float64), np.ascontiguousarray(Z[:, 1], np.float64)
    dcx, dcy = np.ascontiguousarray(dcx, np.float64).ravel(), np.ascontiguousarray(dcy, np.float64).ravel()
    n = np.full(dcx.shape, max_iter, np.uint32)
    live = np.ones(dcx.shape, bool)
    best, period = np.full(dcx.shape, np.inf, np.float64), np.zeros(dcx.shape, np.uint32)
    dx = np.zeros_like(dcx); dy = np.zeros_like(dcx); m = np.zeros(dcx.shape, np.int64)
    two = np.float64(2.0)
    with np.errstate(all="ignore"):
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
            zx = Zx[np.minimum(m, L)] + ndx
            zy = Zy[np.minimum(m, L)] + ndy
            r = zx * zx
            t = zy * zy
            r = r + t
            esc = (r > two) & live
            d2 = ndx * ndx
            t = ndy * ndy
            d2 = d2 + t
            reb = (m == L) | (r < d2)
            dx = np.where(reb, zx, ndx)
            dy = np.where(reb, zy, ndy)
            m = np.where(reb, 0, m)
            n[esc] = i
            live = live & ~esc
            best, period = _update(best, period, i + 1, zx, zy, live)
            if not live.any():
                break
            m = np.where(live, m, 0)   # (a frozen pixel's index must stay inside the table)
    return n.reshape(shape), period.reshape(shape), best.reshape(shape)


def domains(period, amin, max_iter):
    """(count uint32, amin float64, pixel uint32), max_iter + 1 entries each.  amin values order by their bit patterns as uint64; a
    pattern above +inf's (a negative, a NaN) is counted and takes no further part; a period above max_iter is ignored here."""
    period = np.ascontiguousarray(period, np.uint32).ravel()
    key = np.ascontiguousarray(amin, np.float64).ravel().view(np.uint64)
    n = max_iter + 1
    inside = period <= max_iter
    count = np.bincount(period[inside], minlength=n).astype(np.uint32)
    tab = np.full(n, INF_BITS, np.uint64)
    pixel = np.full(n, NO_PIXEL, np.uint32)
    ok = inside & (key <= np.uint64(INF_BITS))
    idx = np.nonzero(ok)[0]
    if idx.size:
        np.minimum.at(tab, period[idx], key[idx])
        hit = idx[key[idx] == tab[period[idx]]]
        np.minimum.at(pixel, period[hit], hit.astype(np.uint32))
    return count, tab.view(np.float64), pixel


def _iterate_newton(Z, L, p, ox, oy):
    dx = dy = zmx = zmy = Dx = Dy = 0.0
    m = 0
    for _ in range(p):
        zkx = dx if m == 0 else zmx + dx
        zky = dy if m == 0 else zmy + dy
        tx, ty = zkx + zkx, zky + zky
        Dx, Dy = ((tx * Dx) - (ty * Dy)) + 1.0, (tx * Dy) + (ty * Dx)
        m = m + 1
        j = m if m < L else L
        z1x, z1y = float(Z[j][0]), float(Z[j][1])
        ax, ay = (zmx + zmx) + dx, (zmy + zmy) + dy
        ndx = ((ax * dx) - (ay * dy)) + ox
        ndy = ((ax * dy) + (ay * dx)) + oy
        zx, zy = z1x + ndx, z1y + ndy
        r = (zx * zx) + (zy * zy)
        if m == L or r < ((ndx * ndx) + (ndy * ndy)):
            dx, dy, m, zmx, zmy = zx, zy, 0, 0.0, 0.0
        else:
            dx, dy, zmx, zmy = ndx, ndy, z1x, z1y
    zx = dx if m == 0 else zmx + dx
    zy = dy if m == 0 else zmy + dy
    return zx, zy, Dx, Dy


def _div(a, b):
    """IEEE division of Python floats where Python raises: x / 0."""
    try:
        return a / b
    except ZeroDivisionError:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def smith(zx, zy, Dx, Dy):
    if abs(Dx) >= abs(Dy):
        r = _div(Dy, Dx)
        den = Dx + (Dy * r)
        return _div(zx + (zy * r), den), _div(zy - (zx * r), den)
    r = _div(Dx, Dy)
    den = Dy + (Dx * r)
    return _div((zx * r) + zy, den), _div((zy * r) - zx, den)


def refine(Z, L, period, offset, max_steps=64):
    """((ox, oy), steps, (qx, qy)) as mc_mandelbrot_nucleus_refine returns them, or None where it refuses a non-finite value."""
    ox, oy = float(offset[0]), float(offset[1])
    steps, q = 0, (0.0, 0.0)
    eps = math.ldexp(1.0, -52)
    for s in range(1, max_steps + 1):
        zx, zy, Dx, Dy = _iterate_newton(Z, L, period, ox, oy)
        if not (math.isfinite(Dx) and math.isfinite(Dy)):
            return None
        qx, qy = smith(zx, zy, Dx, Dy)
        if not (math.isfinite(qx) and math.isfinite(qy)):
            return None
        ox, oy = ox - qx, oy - qy
        if not (math.isfinite(ox) and math.isfinite(oy)):
            return None
        steps, q = s, (qx, qy)
        if max(abs(qx), abs(qy)) <= eps * max(abs(ox), abs(oy)):
            break
    return (ox, oy), steps, q


def parsed_centre(text, bits):
    """The fixed-point number the orbit constructor parses a decimal into: ceil(bits / 64) * 64 fractional bits, truncated, the last bit set
    when anything nonzero was dropped (round to odd)."""
    F = 64 * ((bits + 63) // 64)
    v = Fraction(text)
    scaled = abs(v) * (1 << F)
    k = scaled.numerator // scaled.denominator
    if scaled.denominator != 1 and k * scaled.denominator != scaled.numerator:
        k |= 1
    return Fraction(-k if v < 0 else k, 1 << F)


def offset_text(centre_text, bits, ox, oy, frac_digits, exp2=0):
    """The two strings of mc_mandelbrot_orbit_offset_text for an orbit at centre_text (a pair) with `bits`."""
    out = []
    for text, o in zip(centre_text, (ox, oy)):
        v = parsed_centre(text, bits) + Fraction(o) * Fraction(2) ** exp2
        t = abs(v) * 10 ** frac_digits
        k = t.numerator // t.denominator
        s = str(k).rjust(frac_digits + 1, "0")
        s = s if frac_digits == 0 else s[:-frac_digits] + "." + s[-frac_digits:]
        out.append(("-" if v < 0 else "") + s)
    return tuple(out)
