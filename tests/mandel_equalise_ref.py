"""MC_MANDEL_COLOUR_EQUALISED restated (include/mc_compute.h): the histogram of a count plane, the rank map and the equalised colour, twice
— numpy (bincount, a cumulative sum in Python integers) and an independent scalar loop on Python integers.  Integer arithmetic end to end:
every comparison with the library is bit for bit."""
import numpy as np


def histogram(iters, max_iter):
    """uint32[max_iter + 1]: the number of values equal to j; a value above max_iter counts in bin max_iter."""
    n = np.minimum(np.asarray(iters).reshape(-1).astype(np.int64), max_iter)
    h = np.bincount(n, minlength=max_iter + 1)
    assert h.size == max_iter + 1 and int(h.sum()) < 2 ** 32
    return h.astype(np.uint32)


def rank_map(hist, max_iter):
    """uint32[max_iter + 1]: map[M] = M; j < M: (M * C(j)) // E with C the exclusive cumulative sum and E the escaped total, exact."""
    h = [int(v) for v in np.asarray(hist).reshape(-1)]
    assert len(h) == max_iter + 1 and max_iter >= 1
    below = np.concatenate(([0], np.cumsum(np.array(h[:max_iter], dtype=object))))   # Python integers: no width to overflow
    escaped = int(below[max_iter])
    out = np.zeros(max_iter + 1, np.uint32)
    if escaped:
        out[:max_iter] = [(max_iter * int(c)) // escaped for c in below[:max_iter]]
    out[max_iter] = max_iter
    return out


def rank_map_scalar(hist, max_iter):
    """The same map by one loop over the bins, Python integers only."""
    escaped = 0
    for j in range(max_iter):
        escaped += int(hist[j])
    out = [0] * (max_iter + 1)
    below = 0
    for j in range(max_iter):
        out[j] = (max_iter * below) // escaped if escaped else 0
        below += int(hist[j])
    out[max_iter] = max_iter
    return np.array(out, dtype=np.uint32)


def histogram_scalar(iters, max_iter):
    out = [0] * (max_iter + 1)
    for v in np.asarray(iters).reshape(-1).tolist():
        out[min(int(v), max_iter)] += 1
    return np.array(out, dtype=np.uint32)


def colour(iters, max_iter, lut):
    """float32 (..., 4): lut[map[n]] with the map of the plane's own histogram; lut is the (max_iter + 1, 4) table of
    mc_mandelbrot_colour_lut."""
    n = np.minimum(np.asarray(iters).astype(np.int64), max_iter)
    m = rank_map(histogram(n, max_iter), max_iter)
    return np.asarray(lut, np.float32).reshape(max_iter + 1, 4)[m[n]]


def percentile_span(t, lo=1, hi=99):
    a, b = np.percentile(np.asarray(t, np.float64).reshape(-1), [lo, hi])
    return float(b - a)
