"""Restatements of MC_PRECISION_PERTURB_BLA (include/mc_compute.h), the reference planes of the BLA tests.

- `table`: the BLA table in numpy float64, one ufunc per operation, level-major (A.x, A.y, B.x, B.y, R) per entry, from an orbit table
  Z_0 .. Z_L (the library's own Orbit.table()) and the orbit's scale.
- `iterate` / `plane`: the per-pixel loop in numpy float64, vectorised over the pixels still running (compaction, as
  mandel_perturb_ref.iterate), optionally returning each pixel's loop-trip count (MC_MANDEL_BLA_COUNT_TRIPS).
- `scalar_iters`: the same loop on Python floats, one pixel: an independent statement of the contract.
Not a conftest: the test files import it."""
import numpy as np

from mandel_perturb_ref import dc_axis

EPS = 2.0 ** -53


def level_counts(L):
    """Entries per level: floor((L-2) / 2^k) while that is >= 1 (none when L < 3)."""
    n0 = L - 2 if L >= 3 else 0
    out = []
    k = 0
    while (n0 >> k) >= 1:
        out.append(n0 >> k)
        k += 1
    return out


def level_offsets(L):
    """The first entry of each level in the level-major table."""
    return np.concatenate([[0], np.cumsum(level_counts(L))]).astype(np.int64)


def table(Z, L, scale):
    """(entries, 5) float64: the BLA table of include/mc_compute.h for the orbit table Z ((L+1, 2) float64) and scale (sx, sy)."""
    counts = level_counts(L)
    off = level_offsets(L)
    T = np.zeros((int(off[-1]), 5), np.float64)
    if not counts:
        return T
    eps = np.float64(EPS)
    cm = np.float64(0.5) * (np.abs(np.float64(scale[0])) + np.abs(np.float64(scale[1])))
    z = np.asarray(Z, np.float64)[1:L - 1]                  # Z_1 .. Z_{L-2}
    T[:counts[0], 0] = z[:, 0] + z[:, 0]
    T[:counts[0], 1] = z[:, 1] + z[:, 1]
    T[:counts[0], 2] = 1.0
    T[:counts[0], 3] = 0.0
    T[:counts[0], 4] = eps * np.maximum(np.abs(T[:counts[0], 0]), np.abs(T[:counts[0], 1]))
    with np.errstate(all="ignore"):
        for k in range(1, len(counts)):
            c = counts[k]
            x = T[off[k - 1]:off[k - 1] + 2 * c:2]
            y = T[off[k - 1] + 1:off[k - 1] + 2 * c:2]
            e = T[off[k]:off[k] + c]
            e[:, 0] = (y[:, 0] * x[:, 0]) - (y[:, 1] * x[:, 1])
            e[:, 1] = (y[:, 0] * x[:, 1]) + (y[:, 1] * x[:, 0])
            e[:, 2] = ((y[:, 0] * x[:, 2]) - (y[:, 1] * x[:, 3])) + y[:, 2]
            e[:, 3] = ((y[:, 0] * x[:, 3]) + (y[:, 1] * x[:, 2])) + y[:, 3]
            na = np.abs(x[:, 0]) + np.abs(x[:, 1])
            nb = np.abs(x[:, 2]) + np.abs(x[:, 3])
            q = (y[:, 4] - (nb * cm)) / na
            ok = np.isfinite(e[:, :4]).all(axis=1) & np.isfinite(q) & (na > 0) & (q > 0)
            e[:, 4] = np.where(ok, np.minimum(x[:, 4], np.where(ok, q, 0.0)), 0.0)
    return T


def iterate(Z, L, T, dcx, dcy, max_iter, trips=False):
    """n per pixel (or the loop-trip count, trips=True) for flat float64 offset arrays dcx, dcy against the orbit table Z and the BLA
    table T of `table`."""
    Zx = np.ascontiguousarray(Z[:, 0], np.float64)
    Zy = np.ascontiguousarray(Z[:, 1], np.float64)
    T = np.asarray(T, np.float64)
    off = level_offsets(L)
    nlev = len(off) - 1
    M = int(max_iter)
    dcx = np.ascontiguousarray(dcx, np.float64).ravel().copy()
    dcy = np.ascontiguousarray(dcy, np.float64).ravel().copy()
    n = np.full(dcx.shape, M, np.uint32)
    tr = np.zeros(dcx.shape, np.uint32)
    live = np.arange(dcx.size)
    dx = np.zeros_like(dcx); dy = np.zeros_like(dcx)
    m = np.zeros(dcx.shape, np.int64); i = np.zeros(dcx.shape, np.int64); t = np.zeros(dcx.shape, np.uint32)
    two = np.float64(2.0)
    while live.size:
        t = t + np.uint32(1)
        # the largest valid level k >= 1 per pixel (0: none)
        nd = np.abs(dx) + np.abs(dy)
        K = np.zeros(m.shape, np.int64)
        for k in range(1, nlev):
            s = 1 << k
            cond = (m >= 1) & (((m - 1) & (s - 1)) == 0) & (m + s <= L - 1) & (i + s <= M)
            if not cond.any():
                break
            e = np.where(cond, off[k] + ((m - 1) >> k), 0)
            cond &= nd < np.where(cond, T[e, 4], 0.0)
            K = np.where(cond, k, K)
        sk = K > 0
        e = np.where(sk, off[np.minimum(K, nlev - 1) if nlev else 0] + ((np.maximum(m, 1) - 1) >> K), 0) if nlev else np.zeros_like(m)
        Ax, Ay, Bx, By = (T[e, c] if nlev else np.zeros_like(dx) for c in range(4))
        # skip
        sdx = Ax * dx
        u = Ay * dy
        sdx = sdx - u
        v = Bx * dcx
        u = By * dcy
        v = v - u
        sdx = sdx + v
        sdy = Ax * dy
        u = Ay * dx
        sdy = sdy + u
        v = Bx * dcy
        u = By * dcx
        v = v + u
        sdy = sdy + v
        # PERTURB's exact iteration
        mm = np.where(sk, 0, m)
        zmx = Zx[mm]; zmy = Zy[mm]
        ax = zmx + zmx
        ax = ax + dx
        ay = zmy + zmy
        ay = ay + dy
        ndx = ax * dx
        u = ay * dy
        ndx = ndx - u
        ndx = ndx + dcx
        ndy = ax * dy
        u = ay * dx
        ndy = ndy + u
        ndy = ndy + dcy
        m1 = mm + 1
        zx = Zx[m1] + ndx
        zy = Zy[m1] + ndy
        r = zx * zx
        u = zy * zy
        r = r + u
        esc = (~sk) & (r > two)
        d2 = ndx * ndx
        u = ndy * ndy
        d2 = d2 + u
        reb = (m1 == L) | (r < d2)
        step_dx = np.where(reb, zx, ndx)
        step_dy = np.where(reb, zy, ndy)
        step_m = np.where(reb, 0, m1)
        size = np.left_shift(np.int64(1), K)
        dx = np.where(sk, sdx, step_dx)
        dy = np.where(sk, sdy, step_dy)
        m = np.where(sk, m + size, step_m)
        n[live[esc]] = i[esc]
        tr[live[esc]] = t[esc]
        i = np.where(sk, i + size, i + 1)
        done = esc | (i >= M)
        fin = done & ~esc
        tr[live[fin]] = t[fin]
        if done.any():
            keep = ~done
            live, dcx, dcy, dx, dy, m, i, t = live[keep], dcx[keep], dcy[keep], dx[keep], dy[keep], m[keep], i[keep], t[keep]
    return tr if trips else n


def plane(Z, L, T, W, H, max_iter, scale, rows=None, cols=None, trips=False):
    """The (len(rows), len(cols)) uint32 plane of MC_PRECISION_PERTURB_BLA (n, or trip counts) for image rows `rows` and columns `cols`."""
    rows = np.arange(H) if rows is None else np.asarray(rows)
    cols = np.arange(W) if cols is None else np.asarray(cols)
    dx = dc_axis(W, scale[0], idx=cols)
    dy = dc_axis(H, scale[1], idx=rows)
    DX = np.broadcast_to(dx[None, :], (rows.size, cols.size))
    DY = np.broadcast_to(dy[:, None], (rows.size, cols.size))
    return iterate(Z, L, T, DX, DY, max_iter, trips=trips).reshape(rows.size, cols.size)


def scalar_iters(Z, L, T, dcx, dcy, max_iter, trips=False):
    """The loop of include/mc_compute.h on Python floats, one pixel (Z, T as nested lists or arrays).  Linear search over the levels
    (the kernel bisects: the passing levels are a prefix)."""
    off = [int(v) for v in level_offsets(L)]
    nlev = len(off) - 1
    dx = dy = 0.0
    m = i = t = 0
    while i < max_iter:
        t += 1
        nd = abs(dx) + abs(dy)
        K = 0
        for k in range(1, nlev):
            s = 1 << k
            if m >= 1 and (m - 1) % s == 0 and m + s <= L - 1 and i + s <= max_iter and nd < T[off[k] + (m - 1) // s][4]:
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
            return t if trips else i
        if m == L or r < ((ndx * ndx) + (ndy * ndy)):
            dx, dy, m = zx, zy, 0
        else:
            dx, dy = ndx, ndy
        i += 1
    return t if trips else max_iter


def mean_trips(Z, L, T, W, H, max_iter, scale):
    """Mean loop trips per pixel over the whole (W, H) plane."""
    return float(plane(Z, L, T, W, H, max_iter, scale, trips=True).astype(np.float64).mean())

