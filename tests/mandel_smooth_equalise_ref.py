"""MC_MANDEL_COLOUR_SMOOTH_EQUALISED restated (include/mc_compute.h): the histogram of a smooth plane keyed by q >> 8, the knot map and the
remap, twice — numpy (Python integers where a product could pass 64 bits: the knot map) and an independent scalar loop on Python integers.
Integer arithmetic end to end: every comparison with the library is bit for bit.  The colour is mandel_smooth_ref.colour of the remapped
plane.  Not a conftest: the test files import it."""
import numpy as np

import mandel_smooth_ref as S


def histogram(q, max_iter):
    """uint32[max_iter + 1]: the number of values with min(q >> 8, max_iter) = j (a q above 256 * max_iter counts in bin max_iter)."""
    key = np.minimum(np.asarray(q).reshape(-1).astype(np.int64) >> 8, max_iter)
    h = np.bincount(key, minlength=max_iter + 1)
    assert h.size == max_iter + 1 and int(h.sum()) < 2 ** 32
    return h.astype(np.uint32)


def histogram_scalar(q, max_iter):
    out = [0] * (max_iter + 1)
    for v in np.asarray(q).reshape(-1).tolist():
        out[min(int(v) // 256, max_iter)] += 1
    return np.array(out, dtype=np.uint32)


def knot_map(hist, max_iter):
    """uint32[max_iter + 1]: qmap[M] = 256 M; j < M: (256 M C(j)) // E, C the exclusive cumulative sum, E the escaped total, exact."""
    h = [int(v) for v in np.asarray(hist).reshape(-1)]
    assert len(h) == max_iter + 1 and max_iter >= 1
    below = np.concatenate(([0], np.cumsum(np.array(h[:max_iter], dtype=object))))   # Python integers
    escaped = int(below[max_iter])
    out = np.zeros(max_iter + 1, np.uint32)
    if escaped:
        out[:max_iter] = [(256 * max_iter * int(c)) // escaped for c in below[:max_iter]]
    out[max_iter] = 256 * max_iter
    return out


def knot_map_scalar(hist, max_iter):
    """The same map by one loop over the bins, Python integers only."""
    escaped = 0
    for j in range(max_iter):
        escaped += int(hist[j])
    out = [0] * (max_iter + 1)
    below = 0
    for j in range(max_iter):
        out[j] = (256 * max_iter * below) // escaped if escaped else 0
        below += int(hist[j])
    out[max_iter] = 256 * max_iter
    return np.array(out, dtype=np.uint32)


def remap(q, qmap, max_iter):
    """uint32 of q's shape: q' = qmap[j] + ((qmap[j + 1] - qmap[j]) * f >> 8), j = q >> 8, f = q & 255; 256 M at and above 256 M."""
    v = np.asarray(q, np.uint32).astype(np.int64)
    m = np.asarray(qmap, np.uint32).astype(np.int64)
    top = 256 * max_iter
    inside = v < top
    j = np.where(inside, v >> 8, 0)
    moved = m[j] + (((m[j + 1] - m[j]) * (v & 255)) >> 8)               # int64: a step is below 2^32, the product below 2^40
    out = np.where(inside, moved, top)
    return out.astype(np.uint32)


def remap_scalar(q, qmap, max_iter):
    top = 256 * max_iter
    out = []
    for v in np.asarray(q).reshape(-1).tolist():
        if v >= top:
            out.append(top)
        else:
            j, f = v // 256, v % 256
            out.append(int(qmap[j]) + ((int(qmap[j + 1]) - int(qmap[j])) * f) // 256)
    return np.array(out, dtype=np.uint32).reshape(np.asarray(q).shape)


def ranked(q, max_iter):
    """q' of a whole plane under the knot map of its own histogram."""
    return remap(q, knot_map(histogram(q, max_iter), max_iter), max_iter)


def colour(q, max_iter, lut):
    """float32 (..., 4): the smooth colour of the plane's ranked counts."""
    return S.colour(ranked(q, max_iter), max_iter, lut)


def synthetic_planes(W, H, M, seed=0):
    """[(name, q uint32 (H, W))]: random values with interior pixels, a skewed plane (a few hundred values, long runs: what a deep frame
    holds), one value, all interior, all above 256 M, every bin's first and last fraction."""
    rng = np.random.default_rng(3000 * W + H + seed)
    top = 256 * M
    n = W * H
    rand = rng.integers(0, top, n, dtype=np.int64)
    rand[rng.random(n) < 0.2] = top
    few = rng.integers(0, top, 300, dtype=np.int64)
    skew = np.repeat(few[rng.integers(0, 300, n // 7 + 1)], 7)[:n]
    noise = rng.random(n) < 0.05
    skew[noise] = rng.integers(0, top, int(noise.sum()), dtype=np.int64)
    edges = np.where(np.arange(n) % 2 == 0, 256 * (np.arange(n) % M), 256 * (np.arange(n) % M) + 255)
    out = [("random", rand), ("skewed", skew), ("one value", np.full(n, 256 * (M // 3) + 17)), ("interior", np.full(n, top)),
           ("above", np.full(n, top + 1 + (np.arange(n) % 1000))), ("edges", edges)]
    return [(name, np.asarray(v, np.int64).astype(np.uint32).reshape(H, W)) for name, v in out]
