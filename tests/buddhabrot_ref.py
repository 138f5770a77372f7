"""The Buddhabrot contract of include/mc_compute.h restated in numpy, one ufunc per operation (numpy contracts nothing, keeps denormals
and rounds every double operation once, as the header demands).  Written from the header's words, not from the kernels: the tests hold
mc_buddhabrot_density, both device forms, the maps and the tone map to what this file computes, bit for bit.

`p` is anything with mc_buddhabrot_params' field names (the ctypes structure of the bindings, or params() below)."""
from types import SimpleNamespace

import numpy as np

K = np.uint32(1103515245)
STATS = ("samples", "skipped", "contributing", "points", "added")


def params(width, height, samples, max_iter=1000, min_iter=0, seed=1, view=None, sample_window=None, sample_begin=0, flags=0):
    """mc_buddhabrot_default_params and the overrides of bindings.buddhabrot_params, as a plain namespace."""
    v = (-0.5, 0.0, 3.0, (3.0 * float(height)) / float(width)) if view is None else view
    s = (-0.5, 0.0, 4.0, 4.0) if sample_window is None else sample_window
    return SimpleNamespace(view_centre_x=v[0], view_centre_y=v[1], view_scale_x=v[2], view_scale_y=v[3],
                           sample_centre_x=s[0], sample_centre_y=s[1], sample_scale_x=s[2], sample_scale_y=s[3],
                           sample_begin=sample_begin, sample_end=sample_begin + samples, width=width, height=height,
                           max_iter=max_iter, min_iter=min_iter, seed=seed, flags=flags)


def hash_words(k, seed):
    """(ux, uy): x = low word of k, y = high word, z = seed, after three rounds of the integer hash; the integers are kept."""
    k = np.asarray(k, np.uint64)
    x = (k & np.uint64(0xffffffff)).astype(np.uint32)
    y = (k >> np.uint64(32)).astype(np.uint32)
    z = np.full(k.shape, seed, np.uint32)
    s8 = np.uint32(8)
    with np.errstate(over="ignore"):
        for _ in range(3):
            x, y, z = ((x >> s8) ^ y) * K, ((y >> s8) ^ z) * K, ((z >> s8) ^ x) * K
    return x, y


def sample_c(p, k):
    ux, uy = hash_words(k, p.seed)
    tx = (ux.astype(np.float64) + 0.5) * 2.0 ** -32
    ty = (uy.astype(np.float64) + 0.5) * 2.0 ** -32
    cx = np.float64(p.sample_centre_x) + ((tx - 0.5) * np.float64(p.sample_scale_x))
    cy = np.float64(p.sample_centre_y) + ((ty - 0.5) * np.float64(p.sample_scale_y))
    return cx, cy


def interior(cx, cy):
    xm = cx - 0.25
    y2 = cy * cy
    q = (xm * xm) + y2
    xp = cx + 1.0
    return ((q * (q + xm)) <= (0.25 * y2)) | (((xp * xp) + y2) <= 0.0625)


def _step(zx, zy, sx, sy, cx, cy):
    nzx = (sx - sy) + cx
    nzy = ((2.0 * zx) * zy) + cy
    return nzx, nzy, nzx * nzx, nzy * nzy


def classify(cx, cy, max_iter):
    """n per sample: the i at which sx + sy > 4.0 first held, or max_iter for a sample that never escaped."""
    n = np.full(cx.shape, max_iter, np.int64)
    live = np.arange(cx.size)
    zx = np.zeros(cx.size)
    zy, sx, sy = zx.copy(), zx.copy(), zx.copy()
    c_x, c_y = cx.copy(), cy.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(max_iter):
            if not live.size:
                break
            zx, zy, sx, sy = _step(zx, zy, sx, sy, c_x, c_y)
            out = (sx + sy) > 4.0
            n[live[out]] = i
            keep = ~out
            live, zx, zy, sx, sy, c_x, c_y = live[keep], zx[keep], zy[keep], sx[keep], sy[keep], c_x[keep], c_y[keep]
    return n


def density(p, plane=None, stats=None, chunk=1 << 16):
    """ADDS the density of p's samples to plane (uint32 (height, width); zeros when None) and their counts to stats (a dict; zeros when
    None).  Returns (plane, stats)."""
    W, H, M = int(p.width), int(p.height), int(p.max_iter)
    plane = np.zeros((H, W), np.uint32) if plane is None else plane
    flat = plane.reshape(-1)
    stats = dict.fromkeys(STATS, 0) if stats is None else stats
    wf, hf = np.float64(W), np.float64(H)
    kx, ky = wf / np.float64(p.view_scale_x), hf / np.float64(p.view_scale_y)
    ox, oy = 0.5 * wf, 0.5 * hf
    vcx, vcy = np.float64(p.view_centre_x), np.float64(p.view_centre_y)
    for lo in range(int(p.sample_begin), int(p.sample_end), chunk):
        k = np.arange(lo, min(lo + chunk, int(p.sample_end)), dtype=np.uint64)
        stats["samples"] += k.size
        cx, cy = sample_c(p, k)
        skip = interior(cx, cy)
        stats["skipped"] += int(skip.sum())
        cx, cy = cx[~skip], cy[~skip]
        n = classify(cx, cy, M)
        use = (n < M) & (n >= int(p.min_iter))
        stats["contributing"] += int(use.sum())
        stats["points"] += int(n[use].sum())
        cx, cy, n = cx[use], cy[use], n[use]
        zx = np.zeros(cx.size)
        zy, sx, sy = zx.copy(), zx.copy(), zx.copy()
        i = 0
        with np.errstate(over="ignore", invalid="ignore"):
            while cx.size:
                keep = n > i   # z_(i+1) is plotted for the samples with n >= i + 1
                cx, cy, n, zx, zy, sx, sy = cx[keep], cy[keep], n[keep], zx[keep], zy[keep], sx[keep], sy[keep]
                if not cx.size:
                    break
                zx, zy, sx, sy = _step(zx, zy, sx, sy, cx, cy)
                fx = ((zx - vcx) * kx) + ox
                fy = ((zy - vcy) * ky) + oy
                inside = (fx >= 0.0) & (fx < wf) & (fy >= 0.0) & (fy < hf)
                idx = fy[inside].astype(np.uint32).astype(np.int64) * W + fx[inside].astype(np.uint32).astype(np.int64)
                np.add.at(flat, idx, np.uint32(1))   # (uint32: wraps modulo 2^32)
                stats["added"] += int(inside.sum())
                i += 1
    return plane, stats


def stats_tuple(stats):
    return tuple(int(stats[f]) for f in STATS)


def sqrt_map(levels):
    L = np.float64(levels)
    j = np.arange(levels + 1, dtype=np.float64)
    m = (L * np.sqrt(j / L)).astype(np.uint32)
    return np.minimum(m, np.uint32(levels))


def tonemap(d0, d1, d2, levels, m0, m1, m2):
    """float32 (H, W, 4): channel c = (float)m_c[min(d_c, L)] / (float)L, one fp32 division; alpha 1."""
    out = np.empty(d0.shape + (4,), np.float32)
    lf = np.float32(levels)
    for c, (d, m) in enumerate(((d0, m0), (d1, m1), (d2, m2))):
        out[..., c] = np.asarray(m, np.uint32)[np.minimum(d, np.uint32(levels))].astype(np.float32) / lf
    out[..., 3] = np.float32(1.0)
    return out


def white_level(planes, pct, cap=(1 << 20) - 1):
    """The app's policy (bin/mandelbrot --white PCT; DESIGN.md section 3.26, not part of the ABI): L = the smallest density v >= 1 such that
    the non-empty bins with density <= v are at least pct % of all non-empty bins, read from ONE histogram of min(d, cap) over all the
    planes; 1 when every bin is empty."""
    d = np.concatenate([np.minimum(np.asarray(q, np.uint32).reshape(-1), np.uint32(cap)) for q in planes])
    hist = np.bincount(d, minlength=cap + 1).astype(np.uint64)
    total = int(hist[1:].sum())
    if not total:
        return 1
    need = (float(pct) / 100.0) * float(total)
    run = np.cumsum(hist[1:]).astype(np.float64)
    return int(np.argmax(run >= need)) + 1
