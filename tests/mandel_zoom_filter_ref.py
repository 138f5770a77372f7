"""Restatement of the zoom sequences' area filter of include/mc_compute.h (at mc_mandelbrot_zoom_compose_filtered), in vectorised numpy.

A pixel that reads the deep keyframe takes the box of width r2 = 2 r centred at its position over the texel cells [k - 0.5, k + 0.5]: three
cells per axis, weights in IEEE double converted to fp32, nine taps accumulated in fp32 in row-major order with zero-weight taps skipped,
one division.  Everything that is unchanged comes from mandel_zoom_ref (positions, the source test, the bilinear frame, the byte
conversion) and mandel_zoom_counts_ref (the tap colours).  Written from the header's text, not from the library's source.
"""
import numpy as np

import mandel_zoom_counts_ref as ZC
import mandel_zoom_ref as Z

F32 = np.float32
BILINEAR, AREA = 0, 1


def box(X2, r2, n):
    """(idx (len, 3) int64, w (len, 3) float32, k0, a, b) of the boxes centred at the positions X2 on an axis of n texels."""
    X2 = np.asarray(X2, np.float64)
    r2 = np.float64(r2)
    h = np.float64(0.5) * r2
    a = X2 - h
    b = X2 + h
    fl = np.floor(a)
    k0 = fl.astype(np.int64) + (a >= fl + np.float64(0.5)).astype(np.int64)
    k = k0[:, None] + np.arange(3, dtype=np.int64)[None, :]
    kd = k.astype(np.float64)
    lo = np.maximum(a[:, None], kd - np.float64(0.5))
    hi = np.minimum(b[:, None], kd + np.float64(0.5))
    d = hi - lo
    w = np.where(d > 0.0, d, np.float64(0.0)).astype(F32)
    return np.clip(k, 0, n - 1), w, k0, a, b


def area_sample(img, X2, Y2, r2):
    """The box value of img (H, W, 4) float32 at every (Y2[j], X2[i]): (len(Y2), len(X2), 4) float32, alpha 1."""
    H, W = img.shape[:2]
    ix, wx, _, _, _ = box(X2, r2, W)
    iy, wy, _, _, _ = box(Y2, r2, H)
    ny, nx = len(Y2), len(X2)
    acc = np.zeros((ny, nx, 3), F32)
    sw = np.zeros((ny, nx), F32)
    first = np.ones((ny, nx), bool)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for y in range(3):
            for x in range(3):
                p = wy[:, y][:, None] * wx[:, x][None, :]
                assert p.dtype == F32
                keep = p != F32(0.0)
                t = img[iy[:, y][:, None], ix[:, x][None, :]][..., :3]
                m = p[..., None] * t
                acc = np.where((keep & first)[..., None], m, np.where(keep[..., None], acc + m, acc))
                sw = np.where(keep & first, p, np.where(keep, sw + p, sw))
                first = first & ~keep
        assert not first.any(), "a box of width >= 1 has a cell of non-zero weight on each axis"
        out = np.empty((ny, nx, 4), F32)
        out[..., :3] = acc / sw[..., None]
    out[..., 3] = F32(1.0)
    assert acc.dtype == F32 and sw.dtype == F32
    return out


def compose(wide, deep, r, filter):
    """The filtered frame (H, W, 4) float32 and the mask of its deep-sourced pixels.  filter 0: mandel_zoom_ref.compose."""
    base, mask = Z.compose(wide, deep, r)
    if filter == BILINEAR or deep is None:
        return base, mask
    assert filter == AREA
    deep = np.ascontiguousarray(deep, F32)
    H, W = deep.shape[:2]
    r2 = np.float64(r) + np.float64(r)
    # (positions outside the deep keyframe are clipped only so that the gather stays in range: the mask discards them)
    X2 = np.clip(Z.positions(W, r2), 0.0, np.float64(W - 1))
    Y2 = np.clip(Z.positions(H, r2), 0.0, np.float64(H - 1))
    out = np.where(mask[:, :, None], area_sample(deep, X2, Y2, r2), base)
    return np.ascontiguousarray(out, F32), mask


def frame_counts(mode, wide, deep, M, lut, table, r, filter):
    """The filtered frame from count keyframes: compose() of the two coloured keyframes (mandel_zoom_counts_ref.colour)."""
    cw = ZC.colour(mode, wide, M, lut, table)
    cd = None if deep is None else ZC.colour(mode, deep, M, lut, table)
    return compose(cw, cd, r, filter)


def same_bits(got, want):
    """(H, W) bool: the pixels whose four components agree bit for bit, a NaN agreeing with any NaN (the contract leaves the NaN open)."""
    g = np.ascontiguousarray(got, F32)
    w = np.ascontiguousarray(want, F32)
    return ((g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))).all(axis=-1)


def special_keyframes(W, H, seed=11):
    """Two keyframes with -0.0, +inf, -inf and NaN entries among finite values of both signs; alpha 1."""
    rng = np.random.default_rng(seed + 1000 * W + H)
    out = []
    for _ in range(2):
        a = (rng.random((H, W, 4), dtype=np.float32) - F32(0.5)) * F32(4.0)
        pick = rng.random((H, W, 4))
        a[pick < 0.15] = F32(-0.0)
        a[(pick >= 0.15) & (pick < 0.20)] = F32(np.inf)
        a[(pick >= 0.20) & (pick < 0.23)] = F32(-np.inf)
        a[(pick >= 0.23) & (pick < 0.27)] = F32(np.nan)
        a[..., 3] = 1.0
        a.setflags(write=False)
        out.append(a)
    return tuple(out)
