"""Restatement of the zoom-sequence compose contract of include/mc_compute.h (at mc_mandelbrot_zoom_compose), in vectorised numpy.

A frame whose scale is r times the wide keyframe's (r in [0.5, 1]) reads, per output pixel, the deep keyframe (half the wide one's scale,
same centre) where the pixel falls inside it and the wide keyframe elsewhere, through one bilinear tap.  Positions are IEEE double, values
fp32, every operation rounded once (numpy contracts nothing).  Written from the header's text, not from the library's source.
"""
import numpy as np

F32 = np.float32


def positions(n, ratio):
    """X of every output coordinate g in [0, n): (((double)g - 0.5 n) * ratio) + 0.5 n."""
    g = np.arange(n, dtype=np.float64)
    return ((g - 0.5 * np.float64(n)) * np.float64(ratio)) + 0.5 * np.float64(n)


def taps(X, n):
    """(i0, i1, f) of the positions X on an axis of n texels."""
    i0 = np.clip(np.floor(X).astype(np.int64), 0, n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    f = (X - i0.astype(np.float64)).astype(F32)
    return i0, i1, f


def mix(a, b, f):
    """a + ((b - a) * f) in fp32; a weight of exactly 0 takes a as it is (its sign of zero included)."""
    return np.where(f == F32(0.0), a, a + ((b - a) * f))


def sample(img, X, Y):
    """The bilinear value of img (H, W, 4) float32 at every (Y[j], X[i]): (len(Y), len(X), 4) float32, alpha 1."""
    H, W = img.shape[:2]
    x0, x1, fx = taps(X, W)
    y0, y1, fy = taps(Y, H)
    a00 = img[y0[:, None], x0[None, :]]
    a01 = img[y0[:, None], x1[None, :]]
    a10 = img[y1[:, None], x0[None, :]]
    a11 = img[y1[:, None], x1[None, :]]
    fx = fx[None, :, None]
    fy = fy[:, None, None]
    top = mix(a00, a01, fx)
    bot = mix(a10, a11, fx)
    v = mix(top, bot, fy)
    assert v.dtype == F32
    v[..., 3] = F32(1.0)
    return v


def deep_mask(W, H, r, have_deep=True):
    """(H, W) bool: the pixels of the frame at r that read the deep keyframe."""
    if not have_deep:
        return np.zeros((H, W), bool)
    r2 = np.float64(r) + np.float64(r)
    X2, Y2 = positions(W, r2), positions(H, r2)
    inx = (X2 >= 0.0) & (X2 <= np.float64(W - 1))
    iny = (Y2 >= 0.0) & (Y2 <= np.float64(H - 1))
    return iny[:, None] & inx[None, :]


def compose(wide, deep, r):
    """The frame (H, W, 4) float32 and the mask of its deep-sourced pixels.  wide, deep: (H, W, 4) float32; deep may be None."""
    wide = np.ascontiguousarray(wide, F32)
    H, W = wide.shape[:2]
    out = sample(wide, positions(W, r), positions(H, r))
    mask = deep_mask(W, H, r, deep is not None)
    if deep is not None:
        deep = np.ascontiguousarray(deep, F32)
        r2 = np.float64(r) + np.float64(r)
        # (positions outside the deep keyframe are clipped only so that the gather stays in range: the mask discards them)
        X2 = np.clip(positions(W, r2), 0.0, np.float64(W - 1))
        Y2 = np.clip(positions(H, r2), 0.0, np.float64(H - 1))
        out = np.where(mask[:, :, None], sample(deep, X2, Y2), out)
    return np.ascontiguousarray(out, F32), mask


def rgba8(v):
    """mc_convert_rgba8's conversion (scale 255, no rotation) of (…, 4) float32: truncation toward zero of the fp32 product, the low byte
    kept, 0 outside int32 or for NaN; alpha 255."""
    s = F32(255.0) * np.ascontiguousarray(v, F32)[..., :3]
    ok = (s > F32(-2147483648.0)) & (s < F32(2147483648.0))
    i = np.where(ok, np.trunc(np.where(ok, s, F32(0.0))).astype(np.int64), np.int64(-2147483648))
    out = np.empty(v.shape[:-1] + (4,), np.uint8)
    out[..., :3] = (i & 0xff).astype(np.uint8)
    out[..., 3] = 255
    return out


def ramp(W, H, scale):
    """A keyframe that is a linear ramp of the plane at the given scale (the view spans `scale` around 0): red along x, green along y,
    values in [0.25, 0.75] for scale <= 1."""
    x = (np.arange(W, dtype=np.float64) - 0.5 * W) / W * scale
    y = (np.arange(H, dtype=np.float64) - 0.5 * H) / H * scale
    img = np.zeros((H, W, 4), F32)
    img[..., 0] = ((x[None, :] + 1.0) / 2.0).astype(F32)
    img[..., 1] = ((y[:, None] + 1.0) / 2.0).astype(F32)
    img[..., 2] = F32(0.5)
    img[..., 3] = F32(1.0)
    return img
