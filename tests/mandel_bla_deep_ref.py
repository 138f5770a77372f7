"""Restatements of MC_PRECISION_PERTURB_BLA_DEEP (include/mc_compute.h), the reference planes of the deep BLA tests.

- `table`: the floatexp BLA table in numpy float64 / int64, one ufunc per operation, level-major, as (mantissas (n, 5), exponents (n, 3))
  from an orbit table Z_0 .. Z_L (the library's own Orbit.table()), the orbit's scale (the mantissas of a deep orbit) and E.
- `iterate` / `plane`: the per-pixel loop in numpy float64, vectorised over the pixels still running, optionally returning each pixel's
  loop-trip count (MC_MANDEL_BLA_COUNT_TRIPS).
- `scalar_iters`: the same loop on Python floats, one pixel: an independent statement of the contract.
Floatexp helpers follow the header word for word: norm, add, less.  Not a conftest: the test files import it."""
import math

import numpy as np

import mandel_bla_ref as BR
import mandel_perturb_deep_ref as D

BOUND = 1 << 20
T = D.T
WIN_HI, WIN_LO = D.WIN_HI, D.WIN_LO


# ---- floatexp, numpy -------------------------------------------------------------------------------------------------------------
def _fexp(a):
    return np.frexp(a)[1].astype(np.int64)


def _ld(x, k):
    return np.ldexp(x, np.clip(k, -(1 << 30), 1 << 30).astype(np.int32))


def norm(x, y, e):
    """(x, y) * 2^e normalised: max part in [0.5, 1), or (0, 0, 0)."""
    a = np.fmax(np.fabs(x), np.fabs(y))
    k = _fexp(a)
    z = a == 0.0
    return np.where(z, 0.0, _ld(x, -k)), np.where(z, 0.0, _ld(y, -k)), np.where(z, 0, np.asarray(e, np.int64) + k)


def add(p, q):
    """p + q (mantissas in any range): a zero operand gives the other, normalised; else aligned at the larger frexp exponent."""
    px, py, ep = p
    qx, qy, eq = q
    ep = np.asarray(ep, np.int64)
    eq = np.asarray(eq, np.int64)
    ap = np.fmax(np.fabs(px), np.fabs(py))
    aq = np.fmax(np.fabs(qx), np.fabs(qy))
    e = np.maximum(ep + _fexp(ap), eq + _fexp(aq))
    sx = _ld(px, ep - e)
    sy = _ld(py, ep - e)
    sx = sx + _ld(qx, eq - e)
    sy = sy + _ld(qy, eq - e)
    sx = np.where(ap == 0.0, qx, np.where(aq == 0.0, px, sx))
    sy = np.where(ap == 0.0, qy, np.where(aq == 0.0, py, sy))
    e = np.where(ap == 0.0, eq, np.where(aq == 0.0, ep, e))
    return norm(sx, sy, e)


def less(a, b):
    """a < b for normalised nonnegative reals (x, e)."""
    ax, ae = a
    bx, be = b
    return (bx != 0.0) & ((ax == 0.0) | (ae < be) | ((ae == be) & (ax < bx)))


def table(Z, L, scale, E):
    """(mant (n, 5) float64, exps (n, 3) int32): the floatexp table for the orbit table Z, the scale mantissas and E (0 for an orbit
    of the old scale, whose `scale` is the doubles)."""
    counts = BR.level_counts(L)
    off = BR.level_offsets(L)
    n = int(off[-1])
    Mt = np.zeros((n, 5), np.float64)
    Ex = np.zeros((n, 3), np.int64)
    if not counts:
        return Mt, Ex.astype(np.int32)
    with np.errstate(all="ignore"):
        cmx, _, cme = norm(np.float64(0.5) * (np.abs(np.float64(scale[0])) + np.abs(np.float64(scale[1]))), np.float64(0.0), int(E))
        z = np.asarray(Z, np.float64)[1:L - 1]
        ax, ay, ea = norm(z[:, 0] + z[:, 0], z[:, 1] + z[:, 1], np.zeros(counts[0], np.int64))
        zero = (ax == 0.0) & (ay == 0.0)
        c0 = counts[0]
        Mt[:c0, 0], Mt[:c0, 1], Ex[:c0, 0] = ax, ay, ea
        Mt[:c0, 2], Mt[:c0, 3], Ex[:c0, 1] = 0.5, 0.0, 1
        Mt[:c0, 4] = np.where(zero, 0.0, np.fmax(np.fabs(ax), np.fabs(ay)))
        Ex[:c0, 2] = np.where(zero, 0, ea - 53)
        for k in range(1, len(counts)):
            c = counts[k]
            x = slice(off[k - 1], off[k - 1] + 2 * c, 2)
            y = slice(off[k - 1] + 1, off[k - 1] + 2 * c, 2)
            xm, xe, ym, ye = Mt[x], Ex[x], Mt[y], Ex[y]
            Ax, Ay, eA = norm((ym[:, 0] * xm[:, 0]) - (ym[:, 1] * xm[:, 1]), (ym[:, 0] * xm[:, 1]) + (ym[:, 1] * xm[:, 0]), ye[:, 0] + xe[:, 0])
            Bx, By, eB = add(((ym[:, 0] * xm[:, 2]) - (ym[:, 1] * xm[:, 3]), (ym[:, 0] * xm[:, 3]) + (ym[:, 1] * xm[:, 2]), ye[:, 0] + xe[:, 1]),
                             (ym[:, 2], ym[:, 3], ye[:, 1]))
            na = np.abs(xm[:, 0]) + np.abs(xm[:, 1])
            nb = np.abs(xm[:, 2]) + np.abs(xm[:, 3])
            zc = np.zeros(c)
            dx, _, de = add((ym[:, 4], zc, ye[:, 2]), (-(nb * cmx), zc, xe[:, 1] + cme))
            ok = (na > 0.0) & (dx > 0.0)
            qx, _, qe = norm(np.where(ok, dx / np.where(ok, na, 1.0), 0.0), zc, de - xe[:, 0])
            take_q = less((qx, qe), (xm[:, 4], xe[:, 2]))
            Rx = np.where(ok, np.where(take_q, qx, xm[:, 4]), 0.0)
            eR = np.where(ok, np.where(take_q, qe, xe[:, 2]), 0)
            out = np.zeros(c, bool)
            for e in (eA, eB, eR):
                out |= (e < -BOUND) | (e > BOUND)
            keep = ~out
            dst = slice(off[k], off[k] + c)
            Mt[dst] = np.where(keep[:, None], np.stack([Ax, Ay, Bx, By, Rx], axis=1), 0.0)
            Ex[dst] = np.where(keep[:, None], np.stack([eA, eB, eR], axis=1), 0)
    return Mt, Ex.astype(np.int32)


# ---- the per-pixel loop, numpy ---------------------------------------------------------------------------------------------------
def iterate(Z, L, tab, ux, uy, E, max_iter, trips=False):
    """n per pixel (or the loop-trip count) for flat float64 arrays ux, uy (offsets u * 2^E) against the orbit table Z and the
    table `tab` = (mant, exps) of `table`."""
    Zx = np.ascontiguousarray(Z[:, 0], np.float64)
    Zy = np.ascontiguousarray(Z[:, 1], np.float64)
    Mt, Ex = tab
    Ex = np.asarray(Ex, np.int64)
    off = BR.level_offsets(L)
    nlev = len(off) - 1
    M = int(max_iter)
    E64 = np.int64(E)
    ux = np.ascontiguousarray(ux, np.float64).ravel().copy()
    uy = np.ascontiguousarray(uy, np.float64).ravel().copy()
    N = ux.size
    n = np.full(N, M, np.uint32)
    tr = np.zeros(N, np.uint32)
    live = np.arange(N)
    wx = np.zeros(N); wy = np.zeros(N); dx = np.zeros(N); dy = np.zeros(N)
    S = np.full(N, E, np.int64)
    scaled = np.ones(N, bool)
    m = np.zeros(N, np.int64); i = np.zeros(N, np.int64); t = np.zeros(N, np.uint32)
    two, zero, tT = np.float64(2.0), np.float64(0.0), np.float64(T)
    with np.errstate(all="ignore"):
        while live.size:
            t = t + np.uint32(1)
            nw = np.abs(wx) + np.abs(wy)
            K = np.zeros(N, np.int64)
            for k in range(1, nlev):
                s = 1 << k
                cond = (m >= 1) & (((m - 1) & (s - 1)) == 0) & (m + s <= L - 1) & (i + s <= M)
                if not cond.any():
                    break
                e = np.where(cond, off[k] + ((m - 1) >> k), 0)
                cond &= _ld(nw, S - Ex[e, 2]) < np.where(cond, Mt[e, 4], 0.0)
                K = np.where(cond, k, K)
            sk = K > 0
            if nlev:
                e = np.where(sk, off[np.minimum(K, nlev - 1)] + ((np.maximum(m, 1) - 1) >> K), 0)
                Ax, Ay, Bx, By = (Mt[e, c] if Mt.shape[0] else np.zeros(N) for c in range(4))
                eA, eB = (Ex[e, c] if Ex.shape[0] else np.zeros(N, np.int64) for c in range(2))
            else:
                Ax = Ay = Bx = By = np.zeros(N)
                eA = eB = np.zeros(N, np.int64)
            # skip: add(A w 2^S, B u 2^E), then the phase rule
            px = Ax * wx
            v = Ay * wy
            px = px - v
            py = Ax * wy
            v = Ay * wx
            py = py + v
            qx = Bx * ux
            v = By * uy
            qx = qx - v
            qy = Bx * uy
            v = By * ux
            qy = qy + v
            sx, sy, se = add((px, py, eA + S), (qx, qy, eB + E64))
            sz = (sx == 0.0) & (sy == 0.0)
            sdx = _ld(sx, se)
            sdy = _ld(sy, se)
            splain = ~sz & (np.fmax(np.fabs(sdx), np.fabs(sdy)) >= tT)
            k_wx = np.where(sz, 0.0, np.where(splain, sdx, sx))
            k_wy = np.where(sz, 0.0, np.where(splain, sdy, sy))
            k_dx = np.where(sz, 0.0, sdx)
            k_dy = np.where(sz, 0.0, sdy)
            k_S = np.where(sz, E64, np.where(splain, 0, se))
            k_scaled = ~splain
            # the rescaled iteration, exactly
            mm = np.where(sk, 0, m)
            zmx = Zx[mm]; zmy = Zy[mm]
            fresh = scaled & (zmx == zero) & (zmy == zero)
            S2 = S + S
            Sf = np.maximum(S2, E64)
            pxf = _ld(np.float64(1.0), S2 - Sf)
            puf = _ld(np.float64(1.0), E64 - Sf)
            v = wx * wx
            v2 = wy * wy
            v = v - v2
            v = v * pxf
            v2 = ux * puf
            fx = v + v2
            v = wx * wy
            v2 = wy * wx
            v = v + v2
            v = v * pxf
            v2 = uy * puf
            fy = v + v2
            pu = _ld(np.float64(1.0), E64 - S)
            ax = zmx + zmx
            ax = ax + dx
            ay = zmy + zmy
            ay = ay + dy
            gx = ax * wx
            v = ay * wy
            gx = gx - v
            v = ux * pu
            gx = gx + v
            gy = ax * wy
            v = ay * wx
            gy = gy + v
            v = uy * pu
            gy = gy + v
            nwx = np.where(fresh, fx, gx)
            nwy = np.where(fresh, fy, gy)
            nS = np.where(fresh, Sf, S)
            ndx = _ld(nwx, nS)
            ndy = _ld(nwy, nS)
            m1 = mm + 1
            zx = Zx[m1] + ndx
            zy = Zy[m1] + ndy
            r = zx * zx
            v = zy * zy
            r = r + v
            esc = (~sk) & (r > two)
            d2 = ndx * ndx
            v = ndy * ndy
            d2 = d2 + v
            reb = (m1 == L) | (r < d2)
            a = np.fmax(np.fabs(zx), np.fabs(zy))
            rplain = a >= tT
            rS = np.where(rplain, 0, np.where(a == zero, E64, _fexp(a)))
            rwx = _ld(zx, -rS)
            rwy = _ld(zy, -rS)
            an = np.fmax(np.fabs(ndx), np.fabs(ndy))
            toplain = scaled & (an >= tT)
            aw = np.fmax(np.fabs(nwx), np.fabs(nwy))
            ren = scaled & ~toplain & ((aw > WIN_HI) | (aw < WIN_LO))
            ew = np.where(ren, _fexp(aw), 0)
            e_wx = np.where(toplain, ndx, _ld(nwx, -ew))
            e_wy = np.where(toplain, ndy, _ld(nwy, -ew))
            e_S = np.where(toplain, 0, nS + ew)
            e_scaled = scaled & ~toplain
            st_wx = np.where(reb, rwx, e_wx)
            st_wy = np.where(reb, rwy, e_wy)
            st_dx = np.where(reb, zx, ndx)
            st_dy = np.where(reb, zy, ndy)
            st_S = np.where(reb, rS, e_S)
            st_scaled = np.where(reb, ~rplain, e_scaled)
            st_m = np.where(reb, 0, m1)
            size = np.left_shift(np.int64(1), K)
            wx = np.where(sk, k_wx, st_wx)
            wy = np.where(sk, k_wy, st_wy)
            dx = np.where(sk, k_dx, st_dx)
            dy = np.where(sk, k_dy, st_dy)
            S = np.where(sk, k_S, st_S)
            scaled = np.where(sk, k_scaled, st_scaled)
            m = np.where(sk, m + size, st_m)
            n[live[esc]] = i[esc]
            tr[live[esc]] = t[esc]
            i = np.where(sk, i + size, i + 1)
            done = esc | (i >= M)
            fin = done & ~esc
            tr[live[fin]] = t[fin]
            if done.any():
                keep = ~done
                live, ux, uy, wx, wy, dx, dy, S, scaled, m, i, t = (live[keep], ux[keep], uy[keep], wx[keep], wy[keep], dx[keep],
                                                                    dy[keep], S[keep], scaled[keep], m[keep], i[keep], t[keep])
                N = live.size
    return tr if trips else n


def plane(Z, L, tab, W, H, max_iter, mantissa, E, rows=None, cols=None, trips=False):
    """The (len(rows), len(cols)) uint32 plane of MC_PRECISION_PERTURB_BLA_DEEP (n, or trip counts)."""
    rows = np.arange(H) if rows is None else np.asarray(rows)
    cols = np.arange(W) if cols is None else np.asarray(cols)
    ux = D.u_axis(W, mantissa[0], idx=cols)
    uy = D.u_axis(H, mantissa[1], idx=rows)
    UX = np.broadcast_to(ux[None, :], (rows.size, cols.size))
    UY = np.broadcast_to(uy[:, None], (rows.size, cols.size))
    return iterate(Z, L, tab, UX, UY, E, max_iter, trips=trips).reshape(rows.size, cols.size)


def orbit_E(o):
    """E of an Orbit: its scale_exp2 for a deep orbit, 0 otherwise."""
    return o.scale_exp2 if o.deep else 0


def orbit_plane(o, W, H, M, rows=None, cols=None, trips=False):
    """The restated plane of a bound Orbit that carries its deep table (bla_deep())."""
    return plane(o.table(), o.length, o.bla_deep_table(), W, H, M, o.scale, orbit_E(o), rows=rows, cols=cols, trips=trips)


# ---- the per-pixel loop, Python floats -------------------------------------------------------------------------------------------
_ldexp = D._ldexp
_fmax = D._fmax


def _fe(a):
    return math.frexp(a)[1]


def _norm(x, y, e):
    a = _fmax(abs(x), abs(y))
    if a == 0.0:
        return 0.0, 0.0, 0
    k = _fe(a)
    return _ldexp(x, -k), _ldexp(y, -k), e + k


def _add(p, q):
    if p[0] == 0.0 and p[1] == 0.0:
        return _norm(*q)
    if q[0] == 0.0 and q[1] == 0.0:
        return _norm(*p)
    e = max(p[2] + _fe(_fmax(abs(p[0]), abs(p[1]))), q[2] + _fe(_fmax(abs(q[0]), abs(q[1]))))
    return _norm(_ldexp(p[0], p[2] - e) + _ldexp(q[0], q[2] - e), _ldexp(p[1], p[2] - e) + _ldexp(q[1], q[2] - e), e)


def scalar_iters(Z, L, tab, ux, uy, E, max_iter, trips=False):
    """The loop of include/mc_compute.h on Python floats, one pixel (Z, mantissas and exponents as nested lists).  Linear search over
    the levels."""
    Mt, Ex = tab
    off = [int(v) for v in BR.level_offsets(L)]
    nlev = len(off) - 1
    wx = wy = dx = dy = 0.0
    S, scaled, m, i, t = E, True, 0, 0, 0
    while i < max_iter:
        t += 1
        nw = abs(wx) + abs(wy)
        K = 0
        for k in range(1, nlev):
            s = 1 << k
            if m >= 1 and (m - 1) % s == 0 and m + s <= L - 1 and i + s <= max_iter:
                j = off[k] + (m - 1) // s
                if _ldexp(nw, S - Ex[j][2]) < Mt[j][4]:
                    K = k
        if K:
            j = off[K] + (m - 1) // (1 << K)
            Ax, Ay, Bx, By, _ = Mt[j]
            eA, eB, _ = Ex[j]
            P = ((Ax * wx) - (Ay * wy), (Ax * wy) + (Ay * wx), eA + S)
            Q = ((Bx * ux) - (By * uy), (Bx * uy) + (By * ux), eB + E)
            nx, ny, e = _add(P, Q)
            if nx == 0.0 and ny == 0.0:
                wx = wy = dx = dy = 0.0
                S, scaled = E, True
            else:
                dx, dy = _ldexp(nx, e), _ldexp(ny, e)
                if _fmax(abs(dx), abs(dy)) >= T:
                    wx, wy, S, scaled = dx, dy, 0, False
                else:
                    wx, wy, S, scaled = nx, ny, e, True
            m += 1 << K
            i += 1 << K
            continue
        zmx, zmy = Z[m]
        if scaled and zmx == 0.0 and zmy == 0.0:
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
            return t if trips else i
        if m == L or r < ((ndx * ndx) + (ndy * ndy)):
            m, dx, dy = 0, zx, zy
            a = _fmax(abs(zx), abs(zy))
            if a >= T:
                scaled, S, wx, wy = False, 0, zx, zy
            else:
                scaled = True
                S = E if a == 0.0 else _fe(a)
                wx, wy = _ldexp(zx, -S), _ldexp(zy, -S)
        else:
            wx, wy, dx, dy, S = nwx, nwy, ndx, ndy, nS
            if scaled and _fmax(abs(ndx), abs(ndy)) >= T:
                scaled, S, wx, wy = False, 0, ndx, ndy
            elif scaled:
                a = _fmax(abs(nwx), abs(nwy))
                if a > WIN_HI or a < WIN_LO:
                    e = _fe(a)
                    wx, wy, S = _ldexp(nwx, -e), _ldexp(nwy, -e), nS + e
        i += 1
    return t if trips else max_iter
