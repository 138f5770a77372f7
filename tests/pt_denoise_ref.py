"""The path-tracer denoiser restated in numpy (TEST INFRASTRUCTURE): include/mc_compute.h's contract of mc_pathtrace_guides and
mc_pathtrace_denoise, operation for operation in float32 - one ufunc per fp32 operation, in the order the contract states, so the
library's host calls and device kernels must agree with it bit for bit.  exp2 goes through the oracle's mc_math("exp2", .), the
library's strict fp32 exp2.  guides64() is the same geometry in float64 (ids and t only), for the agreement check."""
import numpy as np

f32 = np.float32
EPS, TRI_EPS, INF = f32(1e-4), f32(1e-7), f32(1e20)
H5 = [f32(0.0625), f32(0.25), f32(0.375), f32(0.25), f32(0.0625)]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]]


def _normalize(a, one):
    s = one / np.sqrt(_dot(a, a))
    return [a[0] * s, a[1] * s, a[2] * s]


def _camera(T):
    """pathTracer.comp:352-353, 360 in the type T (float32: the contract; float64: the agreement check).  The constants are the
    shader's decimal literals rounded to float32 first, as the library holds them."""
    c = lambda v: T(f32(v))   # noqa: E731
    one = T(1)
    o = [c(0.0), c(0.52), c(7.4)]
    d = _normalize([c(0.0), c(-0.06), c(-1.0)], one)
    up = [c(0.0), c(1.0), c(0.0)] if abs(d[1]) < c(0.9) else [c(0.0), c(0.0), c(1.0)]
    cx = _normalize(_cross(d, up), one)
    cy = _cross(cx, d)
    lc = [o[k] + d[k] * c(0.035) for k in range(3)]
    return o, cx, cy, lc


def _guides(W, H, planes, spheres, T):
    """Returns (nl[3], t, x[3], id) as (H, W) arrays in PIXEL order (row gy), computed in the type T."""
    c = lambda v: T(f32(v))   # noqa: E731
    one = T(1)
    planes = np.asarray(planes, f32).reshape(-1, 12).astype(T)
    spheres = np.asarray(spheres, f32).reshape(-1, 12).astype(T)
    n_planes = planes.shape[0]
    o, cx, cy, lc = _camera(T)
    gx = np.arange(W, dtype=T)[None, :] + np.zeros((H, 1), T)
    gy = np.arange(H, dtype=T)[:, None] + np.zeros((1, W), T)
    sx = ((gx + c(0.5)) / T(W) - c(0.5)) * c(0.036)
    sy = ((gy + c(0.5)) / T(H) - c(0.5)) * c(0.024)
    spos = [(o[k] + cx[k] * sx) + cy[k] * sy for k in range(3)]
    with np.errstate(all="ignore"):
        d = _normalize([lc[k] - spos[k] for k in range(3)], one)
        t = np.full((H, W), T(INF), T)
        idx = np.full((H, W), -1, np.int64)
        for i in range(n_planes):
            n = [planes[i, 0], planes[i, 1], planes[i, 2]]
            denom = _dot(d, n)
            dd = (planes[i, 3] - _dot(lc, n)) / denom
            hit = (denom > T(TRI_EPS)) & (dd < t)
            t = np.where(hit, dd, t)
            idx = np.where(hit, i, idx)
        for i in range(spheres.shape[0]):
            oc = [spheres[i, k] - lc[k] for k in range(3)]
            b = _dot(oc, d)
            det = (b * b - _dot(oc, oc)) + spheres[i, 3] * spheres[i, 3]
            ok = ~(det < T(0))
            sq = np.sqrt(np.where(ok, det, T(0)))
            lo, hi = b - sq, b + sq
            dd = np.where(lo <= T(EPS), np.where(hi <= T(EPS), T(INF), hi), lo)
            hit = ok & (dd < t)
            t = np.where(hit, dd, t)
            idx = np.where(hit, n_planes + i, idx)
        miss = ~(t < T(INF))
        idx = np.where(miss, -1, idx)
        x = [lc[k] + d[k] * t for k in range(3)]
        rec = np.concatenate([planes, spheres]) if planes.shape[0] + spheres.shape[0] else np.zeros((1, 12), T)
        geo = rec[np.where(miss, 0, idx)]
        ns = _normalize([x[k] - geo[..., k] for k in range(3)], one)
        sphere = idx >= n_planes
        n = [np.where(sphere, ns[k], geo[..., k]) for k in range(3)]
        flip = ~(_dot(n, d) < T(0))
        nl = [np.where(flip, -n[k], n[k]) for k in range(3)]
    return nl, t, x, idx, miss


def guides(W, H, planes, spheres):
    """mc_pathtrace_guides: (normal_t, position_id), float32 (H, W, 4) each, in storage order."""
    nl, t, x, idx, miss = _guides(W, H, planes, spheres, f32)
    nt = np.stack([np.where(miss, f32(0), nl[0]), np.where(miss, f32(0), nl[1]), np.where(miss, f32(0), nl[2]), np.where(miss, INF, t)], -1)
    pid = np.stack([np.where(miss, f32(0), x[0]), np.where(miss, f32(0), x[1]), np.where(miss, f32(0), x[2]), idx.astype(f32)], -1)
    return np.ascontiguousarray(nt[::-1].astype(f32)), np.ascontiguousarray(pid[::-1].astype(f32))


def guides64(W, H, planes, spheres):
    """The same geometry in float64: (t, id) as (H, W) arrays in storage order."""
    _, t, _, idx, _ = _guides(W, H, planes, spheres, np.float64)
    return t[::-1], idx[::-1]


def _d2(a, b, sl_q, sl_p):
    dx, dy, dz = (a[sl_q + (k,)] - b[sl_p + (k,)] for k in range(3))
    return (dx * dx + dy * dy) + dz * dz


def colour_weight(i, sigma_colour):
    return f32(4 ** i) / (f32(sigma_colour) * f32(sigma_colour))


def filter_pass(O, rgba, normal_t, position_id, step, kc, kn, kx):
    """One pass of the filter with the given step and weights (all float32)."""
    H, W = rgba.shape[:2]
    kc, kn, kx = f32(kc), f32(kn), f32(kx)
    ids = position_id[..., 3]
    sw = np.zeros((H, W), f32)
    s = [np.zeros((H, W), f32) for _ in range(3)]
    with np.errstate(all="ignore"):
        for b in range(-2, 3):
            for a in range(-2, 3):
                dy, dx = step * b, step * a
                y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                take = ids[Q] == ids[P]
                e = (_d2(rgba, rgba, Q, P) * kc + _d2(normal_t, normal_t, Q, P) * kn) + _d2(position_id, position_id, Q, P) * kx
                w = (H5[b + 2] * H5[a + 2]) * O.mc_math("exp2", -e).reshape(e.shape)
                sw[P] = np.where(take, sw[P] + w, sw[P])
                for k in range(3):
                    s[k][P] = np.where(take, s[k][P] + w * rgba[Q + (k,)], s[k][P])
        out = rgba.copy()
        hit = ~(ids < f32(0))
        for k in range(3):
            out[..., k] = np.where(hit, s[k] / sw, rgba[..., k])
    return out


def denoise(O, rgba, normal_t, position_id, passes=5, sigma_colour=128.0, k_normal=8.0, k_position=4.0):
    """mc_pathtrace_denoise: float32 (H, W, 4) planes in, the filtered plane out."""
    cur = np.ascontiguousarray(rgba, f32)
    nt = np.ascontiguousarray(normal_t, f32)
    pid = np.ascontiguousarray(position_id, f32)
    for i in range(passes):
        cur = filter_pass(O, cur, nt, pid, 1 << i, colour_weight(i, sigma_colour), k_normal, k_position)
    return cur
