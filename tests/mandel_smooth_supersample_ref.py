"""MC_MANDEL_SUPERSAMPLE_SMOOTH restated (include/mc_compute.h): the resolve over fractional counts.  Nothing new is computed here: a
sample's colour is mandel_smooth_ref.colour of its smooth count (of mandel_smooth_equalise_ref.remap of it under a knot map), a pixel's
colour is mandel_supersample_ref.tree over its s x s sample colours, rows first, and one scaling by 1 / (s * s).  numpy float32, every add
its own ufunc: every comparison with the library is bit for bit.  Not a conftest: the test files import it."""
import numpy as np

import mandel_smooth_equalise_ref as Q
import mandel_smooth_ref as S
import mandel_supersample_ref as SS

SUPERSAMPLE_SMOOTH = 1 << 13
COLOUR_SMOOTH, COLOUR_SMOOTH_EQUALISED = 1 << 6, 1 << 12
FACTORS = SS.FACTORS


def grid_flags(flags):
    """The flags of mc_mandelbrot_supersample_params' grid: as mandel_supersample_ref.grid_params; with the bit set, the bit cleared and
    the colouring MC_MANDEL_COLOUR_SMOOTH."""
    out = flags & ~(SS.SUPERSAMPLE_MASK | SS.COLOUR_EQUALISED | (1 << 5))
    if out & SUPERSAMPLE_SMOOTH:
        if out & COLOUR_SMOOTH_EQUALISED:
            out = (out & ~COLOUR_SMOOTH_EQUALISED) | COLOUR_SMOOTH
        out &= ~SUPERSAMPLE_SMOOTH
    return out


def sample_colours(q, max_iter, lut, qmap=None):
    """float32 (..., 4): the colour of every sample; a q above 256 * max_iter is interior."""
    q = np.minimum(np.asarray(q, np.uint32), np.uint32(256 * max_iter))
    if qmap is not None:
        q = Q.remap(q, qmap, max_iter)
    return S.colour(q, max_iter, lut)


def resolve(q, s, max_iter, lut, qmap=None):
    """float32 (H, W, 4) from the (s * H, s * W) plane of smooth sample counts: sample (s * y + i, s * x + j) belongs to pixel (y, x)."""
    q = np.asarray(q)
    SH, SW = q.shape
    assert s in FACTORS and SH % s == 0 and SW % s == 0
    H, W = SH // s, SW // s
    c = sample_colours(q, max_iter, lut, qmap).reshape(H, s, W, s, 4)
    rows = [SS.tree([np.ascontiguousarray(c[:, i, :, j, :]) for j in range(s)]) for i in range(s)]
    out = SS.tree(rows) * np.float32(1.0 / (s * s))
    assert out.dtype == np.float32
    return out


def ranked_map(q, max_iter):
    """The knot map of ALL samples of the plane: the ranked form's qmap."""
    return Q.knot_map(Q.histogram(q, max_iter), max_iter)


def seeded_plane(rng, rows, width, s, max_iter):
    """A random (rows * s, width * s) plane of valid smooth counts holding the edge values: 0, fractions 0 and 255, 256 M - 1, 256 M."""
    top = 256 * max_iter
    q = rng.integers(0, top + 1, size=(rows * s, width * s), dtype=np.int64)
    flat = q.reshape(-1)
    pick = rng.random(flat.size)
    flat[pick < 0.15] = top
    flat[(pick >= 0.15) & (pick < 0.25)] &= ~255                 # fraction 0
    flat[(pick >= 0.25) & (pick < 0.35)] |= 255                  # fraction 255 (an interior value passes the top and is clamped back below)
    np.minimum(flat, top, out=flat)
    edge = [0, 255, 256, top - 1, top, max(top - 256, 0), 1]
    flat[:min(len(edge), flat.size)] = edge[:flat.size]
    return q.astype(np.uint32)


def knot_maps(rng, max_iter):
    """[(name, qmap)]: the identity, a random non-decreasing map, one with long runs of coinciding knots, everything at 0."""
    top = 256 * max_iter
    ident = 256 * np.arange(max_iter + 1, dtype=np.int64)
    rand = np.sort(rng.integers(0, top + 1, size=max_iter + 1))
    rand[max_iter] = top
    few = np.sort(rng.integers(0, top + 1, size=max(max_iter // 5, 1)))
    runs = np.sort(few[rng.integers(0, few.size, size=max_iter + 1)])
    runs[max_iter] = top
    flat = np.zeros(max_iter + 1, np.int64)
    flat[max_iter] = top
    return [(n, m.astype(np.uint32)) for n, m in (("identity", ident), ("random", rand), ("runs", runs), ("flat", flat))]
