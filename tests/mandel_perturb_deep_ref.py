"""Restatements of the rescaled loop of MC_PRECISION_PERTURB below 2^-960 (include/mc_compute.h, mc_mandelbrot_orbit_create_deep), the
test views that need it, and mpmath ground truth.

- `iterate` / `plane`: numpy float64, one ufunc per operation (IEEE double, never contracted), compacted to the pixels still running, fed
  the library's own table (Orbit.table()).  `scalar_iters`: the same loop on Python floats, one pixel, written out independently.
- `misiurewicz` / `nucleus`: centres as decimal text at any precision (Newton in mpmath); `mp_iters_deep`: direct iteration of
  c = c_ref + u * 2^E in fixed point (the truth the perturbation has to reproduce).
Not a conftest: the test files import it."""
import functools
import math

import mpmath
import numpy as np

import mandel_perturb_ref as R

T = 2.0 ** -500
WIN_HI = 2.0 ** 256
WIN_LO = 2.0 ** -256

# Misiurewicz points whose orbits stay inside |z|^2 <= 2 (max |z_j|^2 1.30 and 1.59): (preperiod, period, 25-digit seed)
M33 = (3, 3, ("-0.6070310226160880532156986", "0.6052513812789340142448089"))
M41 = (4, 1, ("-0.1010963638456221610257854", "0.9562865108091415007710961"))
NUCLEUS3 = ("-0.1225611668766536", "0.7448617666197442")   # a period-3 nucleus: Z_3 = 0 exactly at the true centre


def _text(v, digits):
    return mpmath.nstr(v, digits, strip_zeros=True, min_fixed=-math.inf, max_fixed=math.inf)


@functools.lru_cache(maxsize=None)
def misiurewicz(pre, period, seed, prec):
    """The Misiurewicz point z_{pre+period}(c) = z_pre(c) near `seed`, by Newton at `prec` bits, as decimal text of prec*log10(2)+10
    digits (accurate to about 2^-prec)."""
    with mpmath.workprec(prec + 64):
        c = mpmath.mpc(mpmath.mpf(seed[0]), mpmath.mpf(seed[1]))
        tol = mpmath.mpf(2) ** -(prec + 32)
        for _ in range(200):
            z = dz = mpmath.mpc(0)
            zk = dzk = None
            for j in range(pre + period):
                z, dz = z * z + c, 2 * z * dz + 1
                if j + 1 == pre:
                    zk, dzk = z, dz
            step = (z - zk) / (dz - dzk)
            c -= step
            if abs(step) < tol:
                break
        else:
            raise RuntimeError("misiurewicz: Newton did not converge")
        digits = int(prec * 0.30103) + 10
        return _text(c.real, digits), _text(c.imag, digits)


@functools.lru_cache(maxsize=None)
def nucleus(period, seed, prec, digits):
    """The nucleus z_period(c) = 0 near `seed`, by Newton at `prec` bits, written to `digits` significant digits."""
    with mpmath.workprec(prec):
        c = mpmath.mpc(mpmath.mpf(seed[0]), mpmath.mpf(seed[1]))
        for _ in range(200):
            z = dz = mpmath.mpc(0)
            for _ in range(period):
                z, dz = z * z + c, 2 * z * dz + 1
            step = z / dz
            c -= step
            if abs(step) < mpmath.mpf(2) ** -(prec - 16):
                break
        return _text(c.real, digits), _text(c.imag, digits)


def u_axis(n, mantissa, idx=None):
    """The mantissa offsets along one axis: ((double)g / (double)n - 0.5) * mantissa (PERTURB's dc table of the mantissa)."""
    return R.dc_axis(n, mantissa, idx)


def _pow2(k):
    return np.ldexp(np.float64(1.0), k)


def iterate(Z, L, ux, uy, E, max_iter):
    """n per pixel for flat float64 arrays ux, uy (the offsets are u * 2^E) against the orbit table Z ((L+1, 2) float64)."""
    Zx = np.ascontiguousarray(Z[:, 0], np.float64)
    Zy = np.ascontiguousarray(Z[:, 1], np.float64)
    ux = np.ascontiguousarray(ux, np.float64).ravel().copy()
    uy = np.ascontiguousarray(uy, np.float64).ravel().copy()
    N = ux.size
    n = np.full(N, max_iter, np.uint32)
    live = np.arange(N)
    wx = np.zeros(N); wy = np.zeros(N); dx = np.zeros(N); dy = np.zeros(N)
    S = np.full(N, E, np.int32)
    scaled = np.ones(N, bool)
    m = np.zeros(N, np.int64)
    E32 = np.int32(E)
    two, zero, tT = np.float64(2.0), np.float64(0.0), np.float64(T)
    with np.errstate(all="ignore"):
        for i in range(max_iter):
            zmx = Zx[m]; zmy = Zy[m]
            fresh = scaled & (zmx == zero) & (zmy == zero)
            # the fresh-exponent step (Z_m = 0, scaled)
            S2 = S + S
            Sf = np.maximum(S2, E32)
            px = _pow2(S2 - Sf)
            puf = _pow2(E32 - Sf)
            t = wx * wx
            t2 = wy * wy
            t = t - t2
            t = t * px
            t2 = ux * puf
            fx = t + t2
            t = wx * wy
            t2 = wy * wx
            t = t + t2
            t = t * px
            t2 = uy * puf
            fy = t + t2
            # the general step
            pu = _pow2(E32 - S)
            ax = zmx + zmx
            ax = ax + dx
            ay = zmy + zmy
            ay = ay + dy
            gx = ax * wx
            t = ay * wy
            gx = gx - t
            t = ux * pu
            gx = gx + t
            gy = ax * wy
            t = ay * wx
            gy = gy + t
            t = uy * pu
            gy = gy + t
            nwx = np.where(fresh, fx, gx)
            nwy = np.where(fresh, fy, gy)
            nS = np.where(fresh, Sf, S)
            ndx = np.ldexp(nwx, nS)
            ndy = np.ldexp(nwy, nS)
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
            # rebase
            a = np.fmax(np.fabs(zx), np.fabs(zy))
            rplain = a >= tT
            _, ea = np.frexp(a)
            rS = np.where(rplain, np.int32(0), np.where(a == zero, E32, ea.astype(np.int32)))
            rwx = np.ldexp(zx, -rS)
            rwy = np.ldexp(zy, -rS)
            # no rebase: phase change / renormalisation of scaled lanes
            an = np.fmax(np.fabs(ndx), np.fabs(ndy))
            toplain = scaled & (an >= tT)
            aw = np.fmax(np.fabs(nwx), np.fabs(nwy))
            ren = scaled & ~toplain & ((aw > WIN_HI) | (aw < WIN_LO))
            _, ew = np.frexp(aw)
            ew = np.where(ren, ew.astype(np.int32), np.int32(0))
            kwx = np.where(toplain, ndx, np.ldexp(nwx, -ew))
            kwy = np.where(toplain, ndy, np.ldexp(nwy, -ew))
            kS = np.where(toplain, np.int32(0), nS + ew)
            kscaled = scaled & ~toplain
            wx = np.where(reb, rwx, kwx)
            wy = np.where(reb, rwy, kwy)
            dx = np.where(reb, zx, ndx)
            dy = np.where(reb, zy, ndy)
            S = np.where(reb, rS, kS).astype(np.int32)
            scaled = np.where(reb, ~rplain, kscaled)
            m = np.where(reb, 0, m)
            if esc.any():
                n[live[esc]] = i
                keep = ~esc
                live, ux, uy, wx, wy, dx, dy, S, scaled, m = (live[keep], ux[keep], uy[keep], wx[keep], wy[keep], dx[keep], dy[keep],
                                                              S[keep], scaled[keep], m[keep])
                if live.size == 0:
                    break
    return n


def plane(Z, L, W, H, max_iter, mantissa, E, rows=None, cols=None):
    """The (len(rows), len(cols)) uint32 plane of the rescaled loop for image rows `rows` and columns `cols` (default: all)."""
    rows = np.arange(H) if rows is None else np.asarray(rows)
    cols = np.arange(W) if cols is None else np.asarray(cols)
    ux = u_axis(W, mantissa[0], idx=cols)
    uy = u_axis(H, mantissa[1], idx=rows)
    UX = np.broadcast_to(ux[None, :], (rows.size, cols.size))
    UY = np.broadcast_to(uy[:, None], (rows.size, cols.size))
    return iterate(Z, L, UX, UY, E, max_iter).reshape(rows.size, cols.size)


def orbit_plane(o, W, H, M, rows=None, cols=None):
    """The plane an Orbit renders: the rescaled loop for a deep orbit, PERTURB's loop otherwise."""
    if o.deep:
        return plane(o.table(), o.length, W, H, M, o.scale, o.scale_exp2, rows=rows, cols=cols)
    return R.plane(o.table(), o.length, W, H, M, o.scale, rows=rows, cols=cols)


def _ldexp(x, k):
    try:
        return math.ldexp(x, k)
    except OverflowError:
        return math.copysign(math.inf, x)


def _fmax(a, b):
    return b if a != a else a if b != b else (a if a >= b else b)


EVENTS = ("fresh_m0", "fresh_m_gt0", "renorm_hi", "renorm_lo", "to_plain", "rebase_near", "rebase_end", "rebase_to_plain",
          "rebase_to_scaled", "rebase_to_zero", "escape_scaled", "escape_plain", "interior_scaled")


def scalar_iters(Z, L, ux, uy, E, max_iter, stats=None):
    """The rescaled loop of include/mc_compute.h on Python floats, one pixel (Z a list of (re, im)).  stats (a dict), when given,
    accumulates "iters" and "scaled" (the iterations begun in the scaled phase) and a count per event class of EVENTS: the branches
    of the loop a lane can take (the census tests/test_mandel_block_audit_host.py asserts is complete over the audit's cases)."""
    def note(key):
        if stats is not None:
            stats[key] = stats.get(key, 0) + 1

    wx = wy = dx = dy = 0.0
    S, scaled, m = E, True, 0
    for i in range(max_iter):
        if stats is not None:
            stats["iters"] = stats.get("iters", 0) + 1
            stats["scaled"] = stats.get("scaled", 0) + scaled
        zmx, zmy = Z[m]
        if scaled and zmx == 0.0 and zmy == 0.0:
            note("fresh_m0" if m == 0 else "fresh_m_gt0")
            nS = max(2 * S, E)
            px, pu = _ldexp(1.0, 2 * S - nS), _ldexp(1.0, E - nS)
            nwx = (((wx * wx) - (wy * wy)) * px) + (ux * pu)
            nwy = (((wx * wy) + (wy * wx)) * px) + (uy * pu)
        else:
            nS = S
            pu = _ldexp(1.0, E - S)
            ax = (zmx + zmx) + dx
            ay = (zmy + zmy) + dy
            nwx = ((ax * wx) - (ay * wy)) + (ux * pu)
            nwy = ((ax * wy) + (ay * wx)) + (uy * pu)
        ndx, ndy = _ldexp(nwx, nS), _ldexp(nwy, nS)
        m += 1
        zx = Z[m][0] + ndx
        zy = Z[m][1] + ndy
        r = (zx * zx) + (zy * zy)
        if r > 2.0:
            note("escape_scaled" if scaled else "escape_plain")
            return i
        if m == L or r < ((ndx * ndx) + (ndy * ndy)):
            note("rebase_end" if m == L else "rebase_near")
            m, dx, dy = 0, zx, zy
            a = _fmax(abs(zx), abs(zy))
            if a >= T:
                note("rebase_to_plain")
                scaled, S, wx, wy = False, 0, zx, zy
            else:
                note("rebase_to_zero" if a == 0.0 else "rebase_to_scaled")
                scaled = True
                S = E if a == 0.0 else math.frexp(a)[1]
                wx, wy = _ldexp(zx, -S), _ldexp(zy, -S)
        else:
            wx, wy, dx, dy, S = nwx, nwy, ndx, ndy, nS
            if scaled and _fmax(abs(ndx), abs(ndy)) >= T:
                note("to_plain")
                scaled, S, wx, wy = False, 0, ndx, ndy
            elif scaled:
                a = _fmax(abs(nwx), abs(nwy))
                if a > WIN_HI or a < WIN_LO:
                    note("renorm_hi" if a > WIN_HI else "renorm_lo")
                    e = math.frexp(a)[1]
                    wx, wy, S = _ldexp(nwx, -e), _ldexp(nwy, -e), nS + e
    if scaled:
        note("interior_scaled")
    return max_iter


def mp_iters_deep(centre, mantissa, E, W, H, gx, gy, max_iter, prec):
    """n for pixel (gx, gy) iterated directly: c = c_ref + u * 2^E, exact from the decimal centre and the double mantissa offsets,
    then R.mp_iters at `prec` fractional bits."""
    ux = float(u_axis(W, mantissa[0], idx=[gx])[0])
    uy = float(u_axis(H, mantissa[1], idx=[gy])[0])
    with mpmath.workprec(prec + 64):
        cx = mpmath.mpf(centre[0]) + mpmath.ldexp(mpmath.mpf(ux), E)
        cy = mpmath.mpf(centre[1]) + mpmath.ldexp(mpmath.mpf(uy), E)
        return R.mp_iters(cx, cy, max_iter, prec)


def view(point, depth_text, prec_extra=64):
    """(centre text, (mx, my), E) for a square view of scale `depth_text` (decimal) around a Misiurewicz point of M33 / M41."""
    import fractions
    v = fractions.Fraction(depth_text)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if v >= fractions.Fraction(2) ** e:
        e += 1
    m = float(v / fractions.Fraction(2) ** e)
    bits = max(64, 1 - e + 96)
    return misiurewicz(point[0], point[1], point[2], bits + prec_extra), (m, m), e
