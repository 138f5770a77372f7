"""Restatement of the count-keyframe zoom contract of include/mc_compute.h (at mc_mandelbrot_zoom_compose_counts), from the header's text.

A keyframe is a plane of uint32 (the count n; for the two smooth colourings the smooth count q).  A tap's colour is one of the existing
colour expressions, a frame is mandel_zoom_ref.compose of the two coloured keyframes, and the map of a frame between two keyframes is the
integer blend of their maps.  Nothing here computes a colour of its own: the colourings come from mandel_equalise_ref, mandel_smooth_ref
and mandel_smooth_equalise_ref, the geometry from mandel_zoom_ref.
"""
import numpy as np

import mandel_equalise_ref as E
import mandel_smooth_equalise_ref as SE
import mandel_smooth_ref as S
import mandel_zoom_ref as Z

MODES = ("plain", "equalised", "smooth", "smooth-equalised")
BLEND_MAX = 256 * (2 ** 24 - 1)


def flag(B, mode):
    return {"plain": 0, "equalised": B.MANDEL_COLOUR_EQUALISED, "smooth": B.MANDEL_COLOUR_SMOOTH,
            "smooth-equalised": B.MANDEL_COLOUR_SMOOTH_EQUALISED}[mode]


def blend(map_wide, map_deep, step, steps):
    """(map_wide[j] (S - s) + map_deep[j] s) // S in Python integers."""
    assert steps >= 1 and 0 <= step <= steps
    out = [(int(a) * (steps - step) + int(b) * step) // steps for a, b in zip(map_wide, map_deep)]
    return np.array(out, dtype=np.uint32)


def own_map(mode, plane, M):
    """The map a keyframe is ranked by on its own: the rank map of its counts, or the knot map of its smooth counts; None without one."""
    if mode == "equalised":
        return E.rank_map(E.histogram(plane, M), M)
    if mode == "smooth-equalised":
        return SE.knot_map(SE.histogram(plane, M), M)
    return None


def colour(mode, plane, M, lut, table=None):
    """float32 (H, W, 4): the colour of every count of a plane under `table` (the rank or knot map; None for plain and smooth)."""
    lut = np.ascontiguousarray(lut, np.float32)
    v = np.asarray(plane, np.uint32)
    if mode == "plain":
        return lut[np.minimum(v.astype(np.int64), M)]
    if mode == "equalised":
        return lut[np.asarray(table, np.uint32).astype(np.int64)[np.minimum(v.astype(np.int64), M)]]
    top = np.uint32(256 * M)
    q = np.minimum(v, top)                                   # (the device takes a q above 256 M as interior; the host refuses it)
    if mode == "smooth":
        return S.colour(q, M, lut)
    assert mode == "smooth-equalised"
    return S.colour(SE.remap(q, table, M), M, lut)


def frame(mode, wide, deep, M, lut, table, r):
    """The frame at r: mandel_zoom_ref.compose of the two coloured keyframes (deep may be None).  Returns (float32 (H, W, 4), deep mask)."""
    cw = colour(mode, wide, M, lut, table)
    cd = None if deep is None else colour(mode, deep, M, lut, table)
    return Z.compose(cw, cd, r)


def equal_taps(wide, deep, r):
    """(same, n): the pixels of the frame at r whose four taps hold one count, and that count (0 elsewhere), reading the keyframe
    the contract names for each pixel."""
    H, W = wide.shape
    mask = Z.deep_mask(W, H, r, deep is not None)
    same = np.zeros((H, W), bool)
    val = np.zeros((H, W), np.uint32)
    for src, ratio, sel in ((wide, r, ~mask), (deep, np.float64(r) + np.float64(r), mask)):
        if src is None or not sel.any():
            continue
        X = np.clip(Z.positions(W, ratio), 0.0, np.float64(W - 1))
        Y = np.clip(Z.positions(H, ratio), 0.0, np.float64(H - 1))
        x0, x1, _ = Z.taps(X, W)
        y0, y1, _ = Z.taps(Y, H)
        a = src[y0[:, None], x0[None, :]]
        eq = (a == src[y0[:, None], x1[None, :]]) & (a == src[y1[:, None], x0[None, :]]) & (a == src[y1[:, None], x1[None, :]])
        same = np.where(sel, eq, same)
        val = np.where(sel, a, val)
    return same, val


def field_plane(W, H, scale, M, smooth=False):
    """A keyframe of the piecewise-constant count field ((floor(6 x) + floor(4 y)) mod 9) * 13 + 5 over the plane, seen at `scale` around
    0, with the band |y| < 0.04 interior.  smooth: the counts as 24.8 values with the fraction 77."""
    x = (np.arange(W, dtype=np.float64) - 0.5 * W) / W * scale
    y = (np.arange(H, dtype=np.float64) - 0.5 * H) / H * scale
    n = ((np.floor(6.0 * x)[None, :] + np.floor(4.0 * y)[:, None]).astype(np.int64) % 9) * 13 + 5
    assert int(n.max()) < M
    v = n * 256 + 77 if smooth else n
    v = np.where(np.abs(y)[:, None] < 0.04, (256 * M if smooth else M), v)
    return np.ascontiguousarray(v, np.uint32)
