"""The noise plane and the noise-guided filter restated in numpy (TEST INFRASTRUCTURE): include/mc_compute.h's contract of
mc_pathtrace_noise and mc_pathtrace_denoise_adaptive, one ufunc per fp32 operation in the order the contract states, so the library's host
calls and device kernels must agree with it bit for bit.  pow045 and exp2 go through the oracle's mc_math, the library's strict ones.  The
filter's pass is pt_denoise_ref.filter_pass with the colour weight read from a plane at the centre pixel; nothing else differs."""
import numpy as np

from pt_denoise_ref import H5, _d2, f32


def noise_v(O, half, scale, full):
    """v: float32 (H, W), the squared distance between the half render encoded as if it were the whole and the whole render."""
    half, full, scale = np.ascontiguousarray(half, f32), np.ascontiguousarray(full, f32), f32(scale)
    with np.errstate(all="ignore"):
        x = half[..., :3] * scale
        lo = np.where(x < f32(0), f32(0), x)
        cl = np.where(f32(1) < lo, f32(1), lo).astype(f32)
        E = O.mc_math("pow045", cl).reshape(cl.shape) * f32(255) + f32(0.5)
        e = E - full[..., :3]
        return ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]).astype(f32)


def noise(O, half, scale, full, radius):
    """mc_pathtrace_noise: float32 (H, W), the mean of v over the (2 radius + 1)^2 window clipped to the image, taps in row-major order."""
    v = noise_v(O, half, scale, full)
    H, W = v.shape
    total, cnt = np.zeros((H, W), f32), np.zeros((H, W), f32)
    with np.errstate(all="ignore"):
        for b in range(-radius, radius + 1):
            for a in range(-radius, radius + 1):
                y0, y1, x0, x1 = max(0, -b), min(H, H - b), max(0, -a), min(W, W - a)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + b, y1 + b), slice(x0 + a, x1 + a))
                total[P] = total[P] + v[Q]
                cnt[P] = cnt[P] + f32(1)
        return (total / cnt).astype(f32)


def colour_weight(i, k_noise, variance):
    """kc_i(p) = (float)4^i / ((k_noise * k_noise) * V_p + 1.0f), float32 (H, W)."""
    k = f32(k_noise)
    with np.errstate(all="ignore"):
        return (f32(4 ** i) / ((k * k) * np.ascontiguousarray(variance, f32) + f32(1))).astype(f32)


def filter_pass(O, rgba, normal_t, position_id, step, kc, kn, kx):
    """One pass with the given step; kc is a float32 (H, W) plane, kn and kx numbers."""
    H, W = rgba.shape[:2]
    kn, kx = f32(kn), f32(kx)
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
                e = (_d2(rgba, rgba, Q, P) * kc[P] + _d2(normal_t, normal_t, Q, P) * kn) + _d2(position_id, position_id, Q, P) * kx
                w = (H5[b + 2] * H5[a + 2]) * O.mc_math("exp2", -e).reshape(e.shape)
                sw[P] = np.where(take, sw[P] + w, sw[P])
                for k in range(3):
                    s[k][P] = np.where(take, s[k][P] + w * rgba[Q + (k,)], s[k][P])
        out = rgba.copy()
        hit = ~(ids < f32(0))
        for k in range(3):
            out[..., k] = np.where(hit, s[k] / sw, rgba[..., k])
    return out


def denoise_adaptive(O, rgba, normal_t, position_id, variance, k_noise=4.0, passes=5, k_normal=8.0, k_position=4.0):
    """mc_pathtrace_denoise_adaptive: float32 (H, W, 4) planes and the (H, W) variance plane in, the filtered plane out."""
    cur = np.ascontiguousarray(rgba, f32)
    nt = np.ascontiguousarray(normal_t, f32)
    pid = np.ascontiguousarray(position_id, f32)
    for i in range(passes):
        kc = colour_weight(i, k_noise, variance)
        cur = filter_pass(O, cur, nt, pid, 1 << i, kc, k_normal, k_position)
    return cur
