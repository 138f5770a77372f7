"""Restatement of MC_MANDEL_COLOUR_SMOOTH (include/mc_compute.h): the smooth count q, its colour, and capture variants of the
per-precision loops that return the escape state (n, zx, zy, cx, cy) the kernels hand to smooth_count.

- `smooth_count` / `colour`: numpy, one ufunc per operation (float64 for the continuation, float32 for the fraction and the colour; never
  contracted).  log2 goes through the oracle's mc_math("log2", .), the library's strict fp32 log2.
- `f32_capture`, `f64_capture`, `perturb_capture`: the vectorised loops of StateF32<false>, mandel_f64_ref.iterate and
  mandel_perturb_ref.iterate, keeping z of the escaping iteration.  `ds_capture`: the two-float loop through the oracle's ds_op.
- `deep_scalar`, `bla_scalar`, `bla_deep_scalar`: the scalar loops of mandel_perturb_deep_ref, mandel_bla_ref and mandel_bla_deep_ref, one
  pixel at a time, returning the escape state.
Every captured z is a float64 (F32: converted exactly; DS: (double)hi + (double)lo).  Not a conftest: the test files import it."""
import math

import numpy as np

import mandel_bla_deep_ref as BD
import mandel_bla_ref as BR
import mandel_perturb_deep_ref as D

TAIL_CAP = 64
MAX_ITER_LIMIT = (1 << 24) - 1
FLT_MAX = np.float32(3.4028234663852886e38)


# ---- q and its colour -------------------------------------------------------------------------------------------------------------
def smooth_count(O, n, M, zx, zy, cx, cy):
    """q (uint32) per escape state: flat or shaped arrays n (counts), zx, zy, cx, cy (float64)."""
    n = np.asarray(n, np.uint32)
    shape = n.shape
    n = n.ravel().astype(np.uint64)
    zx, zy, cx, cy = (np.array(np.broadcast_to(np.asarray(v, np.float64), shape), np.float64).ravel() for v in (zx, zy, cx, cy))
    two, big = np.float64(2.0), np.float64(65536.0)
    with np.errstate(all="ignore"):
        k = np.zeros(n.shape, np.uint64)
        a = zx * zx
        b = zy * zy
        r = a + b
        for _ in range(TAIL_CAP):
            run = ~(r > big)           # a NaN keeps running to the cap
            if not run.any():
                break
            t = zx * zx
            u = zy * zy
            t = t - u
            t = t + cx
            v = two * zx
            v = v * zy
            v = v + cy
            zx = np.where(run, t, zx)
            zy = np.where(run, v, zy)
            k = k + run.astype(np.uint64)
            a = zx * zx
            b = zy * zy
            r = np.where(run, a + b, r)
        rf = r.astype(np.float32)      # round to nearest even; overflow gives inf
        rf = np.where(rf > np.float32(65536.0), rf, np.float32(65536.0)).astype(np.float32)
        rf = np.where(rf > FLT_MAX, FLT_MAX, rf).astype(np.float32)
        l = O.mc_math("log2", rf)
        s = l * np.float32(0.0625)
        t = O.mc_math("log2", s)
        t = np.where(t > np.float32(0.0), t, np.float32(0.0)).astype(np.float32)
        t = np.where(t > np.float32(1.0), np.float32(1.0), t).astype(np.float32)
        f = np.float32(1.0) - t
        f = np.float32(256.0) * f
        F = f.astype(np.uint32).astype(np.uint64)
    q = np.uint64(256) * (n + k) + F
    q = np.minimum(q, np.uint64(256) * np.uint64(M) - np.uint64(1))
    q = np.where(n >= np.uint64(M), np.uint64(256) * np.uint64(M), q)
    return q.astype(np.uint32).reshape(shape)


def colour(q, M, lut):
    """float32 (..., 4): the colour of q from lut ((M + 1, 4) float32, mc_mandelbrot_colour_lut's table)."""
    q = np.asarray(q, np.uint32)
    lut = np.ascontiguousarray(lut, np.float32)
    interior = q == np.uint32(256 * M)
    idx = np.where(interior, 0, q >> np.uint32(8)).astype(np.int64)
    fr = (q & np.uint32(255)).astype(np.float32)
    w = fr * np.float32(0.00390625)
    a = lut[idx]
    b = lut[idx + 1]
    d = b - a
    d = d * w[..., None]
    out = (a + d).astype(np.float32)
    out[..., 3] = np.float32(1.0)
    out[interior] = lut[M]
    return out


# ---- vectorised capture loops -----------------------------------------------------------------------------------------------------
def _grid(cx, cy):
    CX = np.broadcast_to(cx[None, :], (cy.size, cx.size))
    CY = np.broadcast_to(cy[:, None], (cy.size, cx.size))
    return np.array(CX).ravel(), np.array(CY).ravel()


def f32_c_axis(n, centre_hi, scale_hi, idx=None):
    """c along one axis in fp32 source order: u = float(g) / float(n); c = centre + (u - 0.5) * scale."""
    g = (np.arange(n) if idx is None else np.asarray(idx)).astype(np.float32)
    u = g / np.float32(n)
    t = u - np.float32(0.5)
    t = t * np.float32(scale_hi)
    return (np.float32(centre_hi) + t).astype(np.float32)


def f32_capture(W, H, M, centre=(-0.445, 0.0), scale=(2.34, 2.34), rows=None):
    """(n, zx, zy, cx, cy), each (len(rows), W): MC_PRECISION_F32 in numpy float32 with the order of StateF32<false>."""
    rows = np.arange(H) if rows is None else np.asarray(rows)
    cx, cy = _grid(f32_c_axis(W, np.float32(centre[0]), np.float32(scale[0])),
                   f32_c_axis(H, np.float32(centre[1]), np.float32(scale[1]), idx=rows))
    N = cx.size
    n = np.full(N, M, np.uint32)
    ezx = np.zeros(N, np.float64); ezy = np.zeros(N, np.float64)
    live = np.arange(N)
    lcx, lcy = cx.copy(), cy.copy()
    zx = np.zeros(N, np.float32); zy = np.zeros(N, np.float32); sx = np.zeros(N, np.float32); sy = np.zeros(N, np.float32)
    two = np.float32(2.0)
    with np.errstate(all="ignore"):
        for i in range(M):
            nzx = sx - sy
            nzx = nzx + lcx
            nzy = two * zx
            nzy = nzy * zy
            nzy = nzy + lcy
            zx, zy = nzx, nzy
            sx = zx * zx
            sy = zy * zy
            esc = (sx + sy) > two
            if esc.any():
                n[live[esc]] = i
                ezx[live[esc]] = zx[esc].astype(np.float64)
                ezy[live[esc]] = zy[esc].astype(np.float64)
                keep = ~esc
                live, lcx, lcy, zx, zy, sx, sy = live[keep], lcx[keep], lcy[keep], zx[keep], zy[keep], sx[keep], sy[keep]
                if live.size == 0:
                    break
    sh = (rows.size, W)
    return n.reshape(sh), ezx.reshape(sh), ezy.reshape(sh), cx.astype(np.float64).reshape(sh), cy.astype(np.float64).reshape(sh)


def f64_capture(cx, cy, M):
    """(n, zx, zy) for flat float64 arrays cx, cy: mandel_f64_ref.iterate keeping the escaping z."""
    cx = np.ascontiguousarray(cx, np.float64).ravel()
    cy = np.ascontiguousarray(cy, np.float64).ravel()
    N = cx.size
    n = np.full(N, M, np.uint32)
    ezx = np.zeros(N); ezy = np.zeros(N)
    live = np.arange(N)
    zx = np.zeros(N); zy = np.zeros(N); sx = np.zeros(N); sy = np.zeros(N)
    two = np.float64(2.0)
    for i in range(M):
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
            ezx[live[esc]] = zx[esc]
            ezy[live[esc]] = zy[esc]
            keep = ~esc
            live, cx, cy, zx, zy, sx, sy = live[keep], cx[keep], cy[keep], zx[keep], zy[keep], sx[keep], sy[keep]
            if live.size == 0:
                break
    return n, ezx, ezy


def f64_plane_capture(F, W, H, M, centre, scale):
    """(n, zx, zy, cx, cy), each (H, W), of MC_PRECISION_F64 for a view given as doubles (F: mandel_f64_ref)."""
    cxv, cyv, sxv, syv = F.view_words(centre, scale)
    cx, cy = _grid(F.c_axis(W, cxv, sxv), F.c_axis(H, cyv, syv))
    n, zx, zy = f64_capture(cx, cy, M)
    sh = (H, W)
    return n.reshape(sh), zx.reshape(sh), zy.reshape(sh), cx.reshape(sh), cy.reshape(sh)


def perturb_capture(Z, L, dcx, dcy, M):
    """(n, zx, zy, cx, cy) for flat float64 offsets: mandel_perturb_ref.iterate keeping the escaping z; c = Z_1 + dc."""
    Zx = np.ascontiguousarray(Z[:, 0], np.float64)
    Zy = np.ascontiguousarray(Z[:, 1], np.float64)
    dcx = np.ascontiguousarray(dcx, np.float64).ravel().copy()
    dcy = np.ascontiguousarray(dcy, np.float64).ravel().copy()
    cx = Zx[1] + dcx
    cy = Zy[1] + dcy
    N = dcx.size
    n = np.full(N, M, np.uint32)
    ezx = np.zeros(N); ezy = np.zeros(N)
    live = np.arange(N)
    dx = np.zeros(N); dy = np.zeros(N); m = np.zeros(N, np.int64)
    two = np.float64(2.0)
    for i in range(M):
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
            ezx[live[esc]] = zx[esc]
            ezy[live[esc]] = zy[esc]
            keep = ~esc
            live, dcx, dcy, dx, dy, m = live[keep], dcx[keep], dcy[keep], dx[keep], dy[keep], m[keep]
            if live.size == 0:
                break
    return n, ezx, ezy, cx, cy


def perturb_plane_capture(R, Z, L, W, H, M, scale):
    """(n, zx, zy, cx, cy), each (H, W), of MC_PRECISION_PERTURB (R: mandel_perturb_ref)."""
    dcx, dcy = _grid(R.dc_axis(W, scale[0]), R.dc_axis(H, scale[1]))
    return tuple(v.reshape(H, W) for v in perturb_capture(Z, L, dcx, dcy, M))


def _pairs_to_double(p):
    return p[:, 0].astype(np.float64) + p[:, 1].astype(np.float64)


def ds_capture(O, W, H, M, view, rows=None):
    """(n, zx, zy, cx, cy), each (len(rows), W): MC_PRECISION_DS through the oracle's ds_op (view: the eight packed words of
    oracle_py.make_view); z and c as (double)hi + (double)lo."""
    rows = np.arange(H) if rows is None else np.asarray(rows)
    v = np.asarray(view, np.float32)

    def axis(n, idx, c_hi, c_lo, s_hi, s_lo):
        u = idx.astype(np.float32) / np.float32(n)
        t = (u - np.float32(0.5)).astype(np.float32)
        a = np.stack([t, np.zeros_like(t)], 1)
        s = np.broadcast_to(np.array([s_hi, s_lo], np.float32), a.shape)
        c = np.broadcast_to(np.array([c_hi, c_lo], np.float32), a.shape)
        return O.ds_op("add", c, O.ds_op("mul", a, s))

    ax = axis(W, np.arange(W), v[0], v[1], v[4], v[5])
    ay = axis(H, rows, v[2], v[3], v[6], v[7])
    cx = np.ascontiguousarray(np.broadcast_to(ax[None, :, :], (rows.size, W, 2))).reshape(-1, 2)
    cy = np.ascontiguousarray(np.broadcast_to(ay[:, None, :], (rows.size, W, 2))).reshape(-1, 2)
    N = cx.shape[0]
    n = np.full(N, M, np.uint32)
    ezx = np.zeros(N); ezy = np.zeros(N)
    live = np.arange(N)
    lcx, lcy = cx.copy(), cy.copy()
    zx = np.zeros((N, 2), np.float32); zy = np.zeros((N, 2), np.float32)
    two = np.broadcast_to(np.array([2.0, 0.0], np.float32), (N, 2))
    for i in range(M):
        zx2 = O.ds_op("mul", zx, zx)
        zy2 = O.ds_op("mul", zy, zy)
        zxy = O.ds_op("mul", zx, zy)
        twoxy = (np.float32(2.0) * zxy).astype(np.float32)
        zx = O.ds_op("add", O.ds_op("sub", zx2, zy2), lcx)
        zy = O.ds_op("add", twoxy, lcy)
        mag = O.ds_op("add", O.ds_op("mul", zx, zx), O.ds_op("mul", zy, zy))
        esc = O.ds_op("compare", mag, two[:zx.shape[0]])[:, 0] > 0
        if esc.any():
            n[live[esc]] = i
            ezx[live[esc]] = _pairs_to_double(zx[esc])
            ezy[live[esc]] = _pairs_to_double(zy[esc])
            keep = ~esc
            live, lcx, lcy, zx, zy = live[keep], lcx[keep], lcy[keep], zx[keep], zy[keep]
            if live.size == 0:
                break
    sh = (rows.size, W)
    return n.reshape(sh), ezx.reshape(sh), ezy.reshape(sh), _pairs_to_double(cx).reshape(sh), _pairs_to_double(cy).reshape(sh)


# ---- scalar capture loops (Python floats, one pixel) ---------------------------------------------------------------------------------
_ldexp = D._ldexp
_fmax = D._fmax


def perturb_scalar(Z, L, dcx, dcy, M):
    """mandel_perturb_ref.scalar_iters keeping the escape state: (n, zx, zy, cx, cy)."""
    cx, cy = Z[1][0] + dcx, Z[1][1] + dcy
    dx = dy = 0.0
    m = 0
    for i in range(M):
        ax = (Z[m][0] + Z[m][0]) + dx
        ay = (Z[m][1] + Z[m][1]) + dy
        ndx = ((ax * dx) - (ay * dy)) + dcx
        ndy = ((ax * dy) + (ay * dx)) + dcy
        m = m + 1
        zx = Z[m][0] + ndx
        zy = Z[m][1] + ndy
        r = (zx * zx) + (zy * zy)
        if r > 2.0:
            return i, zx, zy, cx, cy
        if m == L or r < ((ndx * ndx) + (ndy * ndy)):
            dx, dy, m = zx, zy, 0
        else:
            dx, dy = ndx, ndy
    return M, 0.0, 0.0, cx, cy


def _deep_step(Z, L, E, ux, uy, st):
    """One exact iteration of the rescaled loop on the state st = [wx, wy, dx, dy, S, scaled, m]; returns (escaped, zx, zy)."""
    wx, wy, dx, dy, S, scaled, m = st
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
        return True, zx, zy
    if m == L or r < ((ndx * ndx) + (ndy * ndy)):
        m, dx, dy = 0, zx, zy
        a = _fmax(abs(zx), abs(zy))
        if a >= D.T:
            scaled, S, wx, wy = False, 0, zx, zy
        else:
            scaled = True
            S = E if a == 0.0 else math.frexp(a)[1]
            wx, wy = _ldexp(zx, -S), _ldexp(zy, -S)
    else:
        wx, wy, dx, dy, S = nwx, nwy, ndx, ndy, nS
        if scaled and _fmax(abs(ndx), abs(ndy)) >= D.T:
            scaled, S, wx, wy = False, 0, ndx, ndy
        elif scaled:
            a = _fmax(abs(nwx), abs(nwy))
            if a > D.WIN_HI or a < D.WIN_LO:
                e = math.frexp(a)[1]
                wx, wy, S = _ldexp(nwx, -e), _ldexp(nwy, -e), nS + e
    st[:] = [wx, wy, dx, dy, S, scaled, m]
    return False, zx, zy


def deep_c(Z, ux, uy, E):
    """c of a deep pixel: Z_1 + ldexp(u, E) (ldexp correctly rounded, 0 when it underflows)."""
    return Z[1][0] + _ldexp(ux, E), Z[1][1] + _ldexp(uy, E)


def deep_scalar(Z, L, ux, uy, E, M):
    """mandel_perturb_deep_ref.scalar_iters keeping the escape state: (n, zx, zy, cx, cy)."""
    cx, cy = deep_c(Z, ux, uy, E)
    st = [0.0, 0.0, 0.0, 0.0, E, True, 0]
    for i in range(M):
        esc, zx, zy = _deep_step(Z, L, E, ux, uy, st)
        if esc:
            return i, zx, zy, cx, cy
    return M, 0.0, 0.0, cx, cy


def bla_scalar(Z, L, T, dcx, dcy, M):
    """mandel_bla_ref.scalar_iters keeping the escape state: (n, zx, zy, cx, cy)."""
    cx, cy = Z[1][0] + dcx, Z[1][1] + dcy
    off = [int(v) for v in BR.level_offsets(L)]
    nlev = len(off) - 1
    dx = dy = 0.0
    m = i = 0
    while i < M:
        nd = abs(dx) + abs(dy)
        K = 0
        for k in range(1, nlev):
            s = 1 << k
            if m >= 1 and (m - 1) % s == 0 and m + s <= L - 1 and i + s <= M and nd < T[off[k] + (m - 1) // s][4]:
                K = k
        if K:
            Ax, Ay, Bx, By, _ = T[off[K] + (m - 1) // (1 << K)]
            dx, dy = (((Ax * dx) - (Ay * dy)) + ((Bx * dcx) - (By * dcy)),
                      ((Ax * dy) + (Ay * dx)) + ((Bx * dcy) + (By * dcx)))
            m += 1 << K
            i += 1 << K
            continue
        ax = (Z[m][0] + Z[m][0]) + dx
        ay = (Z[m][1] + Z[m][1]) + dy
        ndx = ((ax * dx) - (ay * dy)) + dcx
        ndy = ((ax * dy) + (ay * dx)) + dcy
        m = m + 1
        zx = Z[m][0] + ndx
        zy = Z[m][1] + ndy
        r = (zx * zx) + (zy * zy)
        if r > 2.0:
            return i, zx, zy, cx, cy
        if m == L or r < ((ndx * ndx) + (ndy * ndy)):
            dx, dy, m = zx, zy, 0
        else:
            dx, dy = ndx, ndy
        i += 1
    return M, 0.0, 0.0, cx, cy


def bla_deep_scalar(Z, L, tab, ux, uy, E, M):
    """mandel_bla_deep_ref.scalar_iters keeping the escape state: (n, zx, zy, cx, cy)."""
    cx, cy = deep_c(Z, ux, uy, E)
    Mt, Ex = tab
    off = [int(v) for v in BR.level_offsets(L)]
    nlev = len(off) - 1
    st = [0.0, 0.0, 0.0, 0.0, E, True, 0]
    i = 0
    while i < M:
        wx, wy, dx, dy, S, scaled, m = st
        nw = abs(wx) + abs(wy)
        K = 0
        for k in range(1, nlev):
            s = 1 << k
            if m >= 1 and (m - 1) % s == 0 and m + s <= L - 1 and i + s <= M:
                j = off[k] + (m - 1) // s
                if _ldexp(nw, S - Ex[j][2]) < Mt[j][4]:
                    K = k
        if K:
            j = off[K] + (m - 1) // (1 << K)
            Ax, Ay, Bx, By, _ = Mt[j]
            eA, eB, _ = Ex[j]
            P = ((Ax * wx) - (Ay * wy), (Ax * wy) + (Ay * wx), eA + S)
            Q = ((Bx * ux) - (By * uy), (Bx * uy) + (By * ux), eB + E)
            nx, ny, e = BD._add(P, Q)
            if nx == 0.0 and ny == 0.0:
                wx = wy = dx = dy = 0.0
                S, scaled = E, True
            else:
                dx, dy = _ldexp(nx, e), _ldexp(ny, e)
                if _fmax(abs(dx), abs(dy)) >= D.T:
                    wx, wy, S, scaled = dx, dy, 0, False
                else:
                    wx, wy, S, scaled = nx, ny, e, True
            st[:] = [wx, wy, dx, dy, S, scaled, m + (1 << K)]
            i += 1 << K
            continue
        esc, zx, zy = _deep_step(Z, L, E, ux, uy, st)
        if esc:
            return i, zx, zy, cx, cy
        i += 1
    return M, 0.0, 0.0, cx, cy
