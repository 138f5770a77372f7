"""Restatement of MC_MANDEL_COLOUR_DISTANCE (include/mc_compute.h): the distance plane D of a whole image's smooth plane q, and the shaded
colour.  numpy, one ufunc per operation: int64 differences; float64 for g2, the square root and the quotient (numpy's sqrt and / are the
correctly rounded IEEE operations); float32 for the weight and the colour; never contracted.  The base colour is mandel_smooth_ref.colour.
`analytic_distance` is the yardstick of the accuracy test, not part of the contract: the classic 2 |z| ln |z| / |z'| in float64.
Not a conftest: the test files import it."""
import numpy as np

import mandel_smooth_ref as S

SCALE = np.float64(1477.3197218702985)      # the double literal for 1024 / ln 2
FLAT = np.float32(4096.0)                   # D where both differences are zero


def differences(q):
    """(gx, gy), int64 (H, W): central differences, the one-sided difference doubled at a border, 0 along an axis of one pixel."""
    v = np.asarray(q, np.uint32).astype(np.int64)
    out = []
    for axis in (1, 0):
        a = np.moveaxis(v, axis, 0)
        g = np.zeros_like(a)
        if a.shape[0] > 1:
            g[1:-1] = a[2:] - a[:-2]
            g[0] = np.int64(2) * (a[1] - a[0])
            g[-1] = np.int64(2) * (a[-1] - a[-2])
        out.append(np.moveaxis(g, 0, axis))
    return out[0], out[1]


def g2_of(q):
    """float64 (H, W): (a*a) + (b*b) of the contract."""
    gx, gy = differences(q)
    a = gx.astype(np.float64)
    b = gy.astype(np.float64)
    a = a * a
    b = b * b
    return a + b


def near_interior(q, M):
    """bool (H, W): the pixel is interior or has an interior 4-neighbour inside the image."""
    interior = np.asarray(q, np.uint32) == np.uint32(256 * M)
    near = interior.copy()
    near[1:] |= interior[:-1]
    near[:-1] |= interior[1:]
    near[:, 1:] |= interior[:, :-1]
    near[:, :-1] |= interior[:, 1:]
    return near


def plane(q, M):
    """D, float32 (H, W), of the whole image's smooth plane q (uint32 (H, W))."""
    q = np.asarray(q, np.uint32)
    assert q.ndim == 2 and int(q.max()) <= 256 * M
    g2 = g2_of(q)
    with np.errstate(divide="ignore"):
        r = np.sqrt(g2)
        d = SCALE / r
    D = d.astype(np.float32)                # round to nearest even
    D = np.where(g2 == np.float64(0.0), FLAT, D).astype(np.float32)
    D[near_interior(q, M)] = np.float32(0.0)
    return D


def colour(q, D, M, lut, T=1.0):
    """float32 (..., 4): lut[M] for an interior pixel, else the smooth colour of q with rgb scaled by w = D >= T ? 1 : D / T."""
    q = np.asarray(q, np.uint32)
    D = np.asarray(D, np.float32)
    T = np.float32(T)
    lut = np.ascontiguousarray(lut, np.float32)
    base = S.colour(q, M, lut)
    with np.errstate(all="ignore"):
        w = np.where(D >= T, np.float32(1.0), D / T).astype(np.float32)
    out = base.copy()
    out[..., :3] = base[..., :3] * w[..., None]
    out[..., 3] = np.float32(1.0)
    out[q == np.uint32(256 * M)] = lut[M]
    return out


def analytic_distance(cx, cy, pitch, max_steps=4096):
    """float64, the shape of cx: the exterior estimate 2 |z| ln |z| / |z'| of every c = cx + i cy, in units of `pitch`.  z and
    z' <- 2 z z' + 1 are carried in float64 until |z|^2 > 65536 (radius 256); a c that has not got there after max_steps is taken to be in
    the set: 0."""
    c = (np.asarray(cx, np.float64) + 1j * np.asarray(cy, np.float64)).ravel()
    out = np.zeros(c.size, np.float64)
    live = np.arange(c.size)
    z = np.zeros(c.size, np.complex128)
    dz = np.zeros(c.size, np.complex128)
    with np.errstate(all="ignore"):
        for _ in range(max_steps):
            dz = 2.0 * z * dz + 1.0
            z = z * z + c
            r2 = z.real * z.real + z.imag * z.imag
            esc = r2 > 65536.0
            if esc.any():
                az = np.sqrt(r2[esc])
                out[live[esc]] = 2.0 * az * np.log(az) / np.abs(dz[esc]) / pitch
                keep = ~esc
                live, z, dz, c = live[keep], z[keep], dz[keep], c[keep]
                if live.size == 0:
                    break
    return out.reshape(np.shape(cx))


# ---- synthetic smooth planes shared by the host and the GPU tests -------------------------------------------------------------------
BIG_M = (1 << 24) - 1                       # smooth's largest max_iter: differences reach 2^33, g2 passes 2^53


def synthetic_planes(W, H, M, seed=0):
    """[(name, q uint32 (H, W))]: random values, ramps, a slowly varying plane with flat patches (g2 = 0), interior blobs touching each
    border and each corner, an all-interior plane."""
    rng = np.random.default_rng(1000 * W + H + seed)
    top = 256 * M
    ys, xs = np.mgrid[0:H, 0:W]
    out = [("random", rng.integers(0, top, (H, W), dtype=np.uint32)),
           ("ramp-x", np.minimum(256 * xs, top - 1).astype(np.uint32)),
           ("ramp-xy", np.minimum(37 * xs + 211 * ys, top - 1).astype(np.uint32))]
    walk = 4096 + np.cumsum(rng.integers(-40, 41, (H, W)), axis=1) + np.cumsum(rng.integers(-40, 41, (H, 1)), axis=0)
    walk = np.clip(walk, 0, top - 1).astype(np.uint32)
    walk[: max(H // 2, 1), : max(W // 3, 1)] = 777          # a flat patch: g2 = 0 inside it
    out.append(("walk", walk))
    blobs = walk.copy()
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)):
        blobs[max(y - 1, 0): y + 2, max(x - 1, 0): x + 2] = top
    if H > 8 and W > 8:
        blobs[H // 2, W // 2] = top                         # a lone interior pixel away from the borders
    out.append(("blobs", blobs.astype(np.uint32)))
    out.append(("interior", np.full((H, W), top, np.uint32)))
    return out


def large_plane(W, H, M=BIG_M, seed=0):
    """q of 0 next to 256 * M - 1 (a random choice per pixel, and a checkerboard corner): with M = BIG_M g2 passes 2^53."""
    rng = np.random.default_rng(7000 * W + H + seed)
    q = np.where(rng.integers(0, 2, (H, W)) == 1, 256 * M - 1, 0).astype(np.uint32)
    ys, xs = np.mgrid[0:min(H, 4), 0:min(W, 4)]
    q[: min(H, 4), : min(W, 4)] = np.where((xs + ys) % 2 == 0, 0, 256 * M - 1)
    return q
