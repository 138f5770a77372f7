"""MC_MANDEL_SUPERSAMPLE_ADAPTIVE restated (include/mc_compute.h) on top of tests/mandel_supersample_ref.py and
tests/mandel_equalise_ref.py: the anchor plane of a full sample plane, the refined mask (a pixel whose anchor differs from one of its up to
eight neighbours inside the image), and the image — a refined pixel is the full resolve's pixel, any other is lut[anchor]; equalised, the
map is the ANCHOR plane's.  Twice: numpy, and a scalar loop.  Every comparison with the library is bit for bit."""
import numpy as np

import mandel_equalise_ref as E
import mandel_supersample_ref as S

ADAPTIVE = 1 << 5   # MC_MANDEL_SUPERSAMPLE_ADAPTIVE


def grid_params(p):
    """mc_mandelbrot_supersample_params with the adaptive bit: cleared in q like the other two."""
    q = S.grid_params(p)
    if q is not None:
        q["flags"] &= ~ADAPTIVE
    return q


def anchor_plane(samples, s):
    """a(y, x) = n(s * y, s * x): sample (0, 0) of every pixel — the plain W x H image's count plane."""
    return np.ascontiguousarray(np.asarray(samples)[::s, ::s])


def refined_mask(anchor):
    """bool (H, W): a(y', x') != a(y, x) for some |y' - y| <= 1, |x' - x| <= 1 inside the image."""
    a = np.asarray(anchor).astype(np.int64)
    H, W = a.shape
    out = np.zeros((H, W), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
            xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            out[yd, xd] |= a[ys, xs] != a[yd, xd]
    return out


def refined_mask_scalar(anchor):
    a = np.asarray(anchor)
    H, W = a.shape
    out = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            for yy in range(max(y - 1, 0), min(y + 2, H)):
                for xx in range(max(x - 1, 0), min(x + 2, W)):
                    if int(a[yy, xx]) != int(a[y, x]):
                        out[y, x] = True
    return out


def refined_list(anchor):
    """The sorted indices y * W + x of the refined pixels (the device list's order is unspecified)."""
    return np.flatnonzero(refined_mask(anchor).reshape(-1)).astype(np.uint32)


def image(samples, s, max_iter, lut, equalised=False):
    """(float32 (H, W, 4), the refined mask) from the FULL (s * H, s * W) sample plane."""
    samples = np.asarray(samples)
    lut = np.asarray(lut, np.float32).reshape(max_iter + 1, 4)
    a = np.minimum(anchor_plane(samples, s).astype(np.int64), max_iter)
    map_ = E.rank_map(E.histogram(a, max_iter), max_iter) if equalised else None
    mask = refined_mask(anchor_plane(samples, s))
    full = S.resolve(samples, s, max_iter, lut, map_)
    plain = lut[a] if map_ is None else lut[map_.astype(np.int64)[a]]
    out = np.where(mask[..., None], full, plain)
    assert out.dtype == np.float32
    return out, mask


def image_scalar(samples, s, max_iter, lut, equalised=False):
    """The same image pixel by pixel: only a refined pixel's samples are ever looked at."""
    samples = np.asarray(samples)
    lut = np.asarray(lut, np.float32).reshape(max_iter + 1, 4)
    H, W = samples.shape[0] // s, samples.shape[1] // s
    a = [[min(int(samples[s * y, s * x]), max_iter) for x in range(W)] for y in range(H)]
    map_ = None
    if equalised:
        map_ = E.rank_map_scalar(E.histogram_scalar(np.array(a), max_iter), max_iter)
    mask = refined_mask_scalar(anchor_plane(samples, s))
    out = np.empty((H, W, 4), np.float32)
    for y in range(H):
        for x in range(W):
            if mask[y, x]:
                out[y, x] = S.resolve_scalar(samples[s * y:s * y + s, s * x:s * x + s], s, max_iter, lut, map_)[0, 0]
            else:
                out[y, x] = lut[a[y][x] if map_ is None else int(map_[a[y][x]])]
    return out, mask


def missed(samples, s, mask):
    """Pixels with mixed samples that the rule does not refine: where adaptive and full supersampling may differ."""
    b = np.asarray(samples).astype(np.int64)
    H, W = b.shape[0] // s, b.shape[1] // s
    b = b.reshape(H, s, W, s).transpose(0, 2, 1, 3).reshape(H, W, s * s)
    return (b.max(axis=-1) != b.min(axis=-1)) & ~np.asarray(mask)
