"""MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE restated (include/mc_compute.h): the refine rule over smooth counts, twice (numpy, and a scalar
loop), and the image as a selection between two images the other restatements already give: where(mask, full, plain).  Nothing new is
computed in floating point.  Not a conftest: the test files import it."""
import numpy as np

import mandel_smooth_equalise_ref as Q
import mandel_smooth_ref as S
import mandel_smooth_supersample_ref as X

SMOOTH_ADAPTIVE = 1 << 14
DEFAULT_THRESHOLD = 256
FACTORS = X.FACTORS


def grid_flags(flags):
    """The flags of mc_mandelbrot_supersample_params' grid: mandel_smooth_supersample_ref.grid_flags; with bit 14 set, the bit cleared and
    the colouring MC_MANDEL_COLOUR_SMOOTH, exactly as for bit 13."""
    out = X.grid_flags(flags)
    if out & SMOOTH_ADAPTIVE:
        if out & X.COLOUR_SMOOTH_EQUALISED:
            out = (out & ~X.COLOUR_SMOOTH_EQUALISED) | X.COLOUR_SMOOTH
        out &= ~SMOOTH_ADAPTIVE
    return out


def refine(q, max_iter, tau):
    """bool (H, W): |a - a'| > tau for one of the up to eight neighbours inside the plane, a = min(q, 256 M); int64, so no wrap."""
    a = np.minimum(np.asarray(q).astype(np.int64), 256 * max_iter)
    H, W = a.shape
    mask = np.zeros((H, W), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy == 0 and dx == 0:
                continue
            ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
            xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            mask[yd, xd] |= np.abs(a[yd, xd] - a[ys, xs]) > tau
    return mask


def refine_scalar(q, max_iter, tau):
    """The same rule by one loop over the pixels, Python integers only."""
    rows = [[min(int(v), 256 * max_iter) for v in r] for r in np.asarray(q).tolist()]
    H, W = len(rows), len(rows[0])
    out = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            a = rows[y][x]
            for yy in range(max(y - 1, 0), min(y + 2, H)):
                for xx in range(max(x - 1, 0), min(x + 2, W)):
                    b = rows[yy][xx]
                    if (a - b if a > b else b - a) > tau:
                        out[y, x] = True
    return out


def anchor(grid_q, s):
    """The anchor plane of a grid's smooth plane: sample (0, 0) of every pixel."""
    return np.ascontiguousarray(np.asarray(grid_q)[::s, ::s])


def image(grid_q, s, max_iter, lut, tau, ranked=False):
    """(image float32 (H, W, 4), mask): where(mask, full, plain).  The anchor plane is the grid's (s * y, s * x) samples; the ranked form's
    knot map is the ANCHOR plane's (the plain smooth-equalised image's), for refined and unrefined pixels alike."""
    a = anchor(grid_q, s)
    mask = refine(a, max_iter, tau)
    qmap = Q.knot_map(Q.histogram(a, max_iter), max_iter) if ranked else None
    full = X.resolve(grid_q, s, max_iter, lut, qmap)
    plain = Q.colour(a, max_iter, lut) if ranked else S.colour(a, max_iter, lut)
    return np.where(mask[..., None], full, plain), mask


def seeded_plane(rng, W, H, max_iter):
    """A random (H, W) plane holding 0, 256 M - 1, 256 M, values above 256 M (clamped by the rule) and 0xffffffff, with smooth stretches
    (small steps between neighbours) so that thresholds near one iteration split the plane."""
    top = 256 * max_iter
    walk = np.cumsum(rng.integers(-300, 301, size=(H, W)), axis=1) + rng.integers(0, top + 1, size=(H, 1))
    q = np.clip(walk, 0, top).astype(np.int64)
    flat = q.reshape(-1)
    pick = rng.random(flat.size)
    flat[pick < 0.10] = top
    flat[(pick >= 0.10) & (pick < 0.15)] = top + 1 + rng.integers(0, 5000, int(((pick >= 0.10) & (pick < 0.15)).sum()))
    flat[(pick >= 0.15) & (pick < 0.18)] = 0xffffffff
    flat[(pick >= 0.18) & (pick < 0.22)] = rng.integers(0, top + 1, int(((pick >= 0.18) & (pick < 0.22)).sum()))
    edge = [0, top - 1, top, top + 1, 0xffffffff, 1, max(top - 256, 0)]
    flat[:min(len(edge), flat.size)] = edge[:flat.size]
    return q.astype(np.uint32)
