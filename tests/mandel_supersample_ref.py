"""MC_MANDEL_SUPERSAMPLE restated (include/mc_compute.h): the sample grid's parameters, the colour of a pixel from its s x s sample counts
— float32 adds by adjacent pairs, level by level, first inside a sample row, then over the rows, then one scaling by 1 / (s * s) — and the
RGBA8 conversion.  Twice: numpy float32 arrays (every add its own ufunc, never np.sum, whose order is numpy's business) and a scalar loop
on numpy float32 scalars.  IEEE single, round to nearest, nothing to contract: every comparison with the library is bit for bit."""
import numpy as np

FACTORS = (2, 4, 8)
SUPERSAMPLE_SHIFT, SUPERSAMPLE_MASK = 8, 15 << 8
COLOUR_EQUALISED = 1 << 4


def flag(s):
    """MC_MANDEL_SUPERSAMPLE(s): bits 8-11 of mc_mandelbrot_params.flags."""
    return (s & 15) << SUPERSAMPLE_SHIFT


def factor_of(flags):
    return (flags >> SUPERSAMPLE_SHIFT) & 15


def grid_params(p):
    """mc_mandelbrot_supersample_params on a dict of the params' integer fields: the six sizes times s, the supersample bits and the
    equalised flag cleared, the rest copied.  None where the library refuses (an invalid factor, a product beyond uint32_t)."""
    s = factor_of(p["flags"])
    if s <= 1:
        s = 1
    elif s not in FACTORS:
        return None
    q = dict(p)
    for k in ("width", "height", "row_begin", "row_end", "row_block", "row_stride"):
        q[k] = p[k] * s
        if q[k] > 2 ** 32 - 1:
            return None
    q["flags"] = p["flags"] & ~(SUPERSAMPLE_MASK | COLOUR_EQUALISED)
    return q


def tree(parts):
    """tree(a_0 .. a_{k-1}): a_0 for k = 1, else tree(a_0 + a_1, a_2 + a_3, ...); float32 arrays (or scalars) of one shape."""
    parts = list(parts)
    assert len(parts) in (1, 2, 4, 8)
    while len(parts) > 1:
        parts = [parts[2 * k] + parts[2 * k + 1] for k in range(len(parts) // 2)]
        assert all(x.dtype == np.float32 for x in parts)
    return parts[0]


def resolve(samples, s, max_iter, lut, map_=None):
    """float32 (H, W, 4) from the (s * H, s * W) plane of sample counts: sample (s * y + i, s * x + j) belongs to pixel (y, x).  lut is the
    (max_iter + 1, 4) table of mc_mandelbrot_colour_lut; map_ (max_iter + 1 entries) turns lut[n] into lut[map_[n]]; a count above
    max_iter reads entry max_iter."""
    samples = np.asarray(samples)
    SH, SW = samples.shape
    assert s in FACTORS and SH % s == 0 and SW % s == 0
    H, W = SH // s, SW // s
    n = np.minimum(samples.astype(np.int64), max_iter)
    if map_ is not None:
        n = np.asarray(map_).astype(np.int64)[n]
    c = np.asarray(lut, np.float32).reshape(max_iter + 1, 4)[n].reshape(H, s, W, s, 4)
    rows = [tree([np.ascontiguousarray(c[:, i, :, j, :]) for j in range(s)]) for i in range(s)]
    t = tree(rows)
    out = t * np.float32(1.0 / (s * s))
    assert out.dtype == np.float32
    return out


def resolve_scalar(samples, s, max_iter, lut, map_=None):
    """The same colours by loops over pixels, components and samples on numpy float32 scalars: an independent statement."""
    samples = np.asarray(samples)
    H, W = samples.shape[0] // s, samples.shape[1] // s
    lut = np.asarray(lut, np.float32).reshape(max_iter + 1, 4)
    inv = np.float32(1.0) / np.float32(s * s)

    def pairwise(v):
        while len(v) > 1:
            v = [np.float32(v[k] + v[k + 1]) for k in range(0, len(v), 2)]
        return v[0]

    out = np.empty((H, W, 4), np.float32)
    for y in range(H):
        for x in range(W):
            for ch in range(4):
                rows = []
                for i in range(s):
                    vals = []
                    for j in range(s):
                        n = min(int(samples[s * y + i, s * x + j]), max_iter)
                        if map_ is not None:
                            n = int(map_[n])
                        vals.append(lut[n, ch])
                    rows.append(pairwise(vals))
                out[y, x, ch] = np.float32(pairwise(rows) * inv)
    return out


def rgba8(rgba):
    """mc_convert_rgba8 (scale 255, no rotation) of colours in [0, 1]: the float32 product truncated toward zero, its low byte; alpha 255."""
    v = np.float32(255.0) * np.asarray(rgba, np.float32)
    assert v.dtype == np.float32
    out = (v.astype(np.int32) & 0xff).astype(np.uint8)
    out[..., 3] = 255
    return out


def mixed_share(samples, s):
    """(share of pixels whose s * s samples hold more than one count, mean of max - min count inside a pixel)."""
    a = np.asarray(samples).astype(np.int64)
    H, W = a.shape[0] // s, a.shape[1] // s
    b = a.reshape(H, s, W, s).transpose(0, 2, 1, 3).reshape(H, W, s * s)
    spread = b.max(axis=-1) - b.min(axis=-1)
    return float((spread > 0).mean()), float(spread.mean())
