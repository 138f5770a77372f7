"""The importance map, the cell list and the guided samples of include/mc_compute.h (the Buddhabrot's guided calls) restated in numpy,
on top of tests/buddhabrot_ref.py: the hash, the window, the interior test, the classification and the step are that file's, one ufunc
per operation.  Written from the header's words, not from the kernels: the tests hold the host calls, both device forms and the blocking
chain to what this file computes, bit for bit.

`p` is anything with mc_buddhabrot_params' field names; a map is uint32[G * G], row-major, the cell rows following cy."""
import numpy as np

import buddhabrot_ref as R

CELLS_COMPLEMENT = 1
GUIDE_DEFAULTS = dict(grid_log2=8, pilot_samples=1 << 24, threshold=1, dilate=1, complement_weight=0)


def cell_of(ux, uy, g):
    """(uy >> (32 - g)) * G + (ux >> (32 - g)), G = 2^g."""
    s = np.uint32(32 - g)
    return (uy >> s).astype(np.int64) * (1 << g) + (ux >> s).astype(np.int64)


def guided_words(ux, uy, cell, g):
    """ux' = ((cell mod G) << (32 - g)) | (ux >> g), uy' = ((cell / G) << (32 - g)) | (uy >> g): the hash's HIGH bits, shifted down."""
    G = 1 << g
    cell = np.asarray(cell, np.int64)
    hx = ((cell % G) << (32 - g)).astype(np.uint32)
    hy = ((cell // G) << (32 - g)).astype(np.uint32)
    return hx | (ux >> np.uint32(g)), hy | (uy >> np.uint32(g))


def _c_of_words(p, ux, uy):
    tx = (ux.astype(np.float64) + 0.5) * 2.0 ** -32
    ty = (uy.astype(np.float64) + 0.5) * 2.0 ** -32
    cx = np.float64(p.sample_centre_x) + ((tx - 0.5) * np.float64(p.sample_scale_x))
    cy = np.float64(p.sample_centre_y) + ((ty - 0.5) * np.float64(p.sample_scale_y))
    return cx, cy


def _samples(p, ux, uy, flat, stats, weight):
    """The contract from `tx` on for the samples with hash words ux, uy: interior skip, classify, plot.  ADDS weight per point inside the
    view to flat (unless None) and the counts to stats; returns added_k, the points inside the view of each sample."""
    W, H, M = int(p.width), int(p.height), int(p.max_iter)
    wf, hf = np.float64(W), np.float64(H)
    kx, ky = wf / np.float64(p.view_scale_x), hf / np.float64(p.view_scale_y)
    ox, oy = 0.5 * wf, 0.5 * hf
    vcx, vcy = np.float64(p.view_centre_x), np.float64(p.view_centre_y)
    added_k = np.zeros(ux.size, np.int64)
    who = np.arange(ux.size)
    stats["samples"] += ux.size
    cx, cy = _c_of_words(p, ux, uy)
    skip = R.interior(cx, cy)
    stats["skipped"] += int(skip.sum())
    cx, cy, who = cx[~skip], cy[~skip], who[~skip]
    n = R.classify(cx, cy, M)
    use = (n < M) & (n >= int(p.min_iter))
    stats["contributing"] += int(use.sum())
    stats["points"] += int(n[use].sum())
    cx, cy, n, who = cx[use], cy[use], n[use], who[use]
    zx = np.zeros(cx.size)
    zy, sx, sy = zx.copy(), zx.copy(), zx.copy()
    i = 0
    with np.errstate(over="ignore", invalid="ignore"):
        while cx.size:
            keep = n > i
            cx, cy, n, who, zx, zy, sx, sy = cx[keep], cy[keep], n[keep], who[keep], zx[keep], zy[keep], sx[keep], sy[keep]
            if not cx.size:
                break
            zx, zy, sx, sy = R._step(zx, zy, sx, sy, cx, cy)
            fx = ((zx - vcx) * kx) + ox
            fy = ((zy - vcy) * ky) + oy
            inside = (fx >= 0.0) & (fx < wf) & (fy >= 0.0) & (fy < hf)
            if flat is not None:
                idx = fy[inside].astype(np.uint32).astype(np.int64) * W + fx[inside].astype(np.uint32).astype(np.int64)
                np.add.at(flat, idx, np.uint32(weight))   # (uint32: wraps modulo 2^32)
            np.add.at(added_k, who[inside], 1)
            i += 1
    stats["added"] += int(added_k.sum())
    return added_k


def importance(p, g, map=None, plane=None, stats=None, want_plane=True, chunk=1 << 16):
    """mc_buddhabrot_importance: the uniform call's samples, statistics and (want_plane) plane, and map[cell(k)] += added_k for every
    sample with added_k > 0.  ADDS to map, plane and stats (zeros when None).  Returns (map, plane or None, stats)."""
    G = 1 << g
    map = np.zeros(G * G, np.uint32) if map is None else map
    stats = dict.fromkeys(R.STATS, 0) if stats is None else stats
    if want_plane and plane is None:
        plane = np.zeros((int(p.height), int(p.width)), np.uint32)
    flat = plane.reshape(-1) if want_plane else None
    for lo in range(int(p.sample_begin), int(p.sample_end), chunk):
        k = np.arange(lo, min(lo + chunk, int(p.sample_end)), dtype=np.uint64)
        ux, uy = R.hash_words(k, p.seed)
        added_k = _samples(p, ux, uy, flat, stats, 1)
        with np.errstate(over="ignore"):
            np.add.at(map, cell_of(ux, uy, g), added_k.astype(np.uint32))   # (wraps modulo 2^32; a sample with added_k = 0 adds 0)
    return map, (plane if want_plane else None), stats


def cells(g, map, threshold=1, dilate=0, flags=0):
    """mc_buddhabrot_importance_cells: the cells with map >= threshold, grown by `dilate` rings of the 8-neighbourhood clipped at the
    grid's edge, in ascending order; CELLS_COMPLEMENT: the cells NOT in that set."""
    G = 1 << g
    m = (np.asarray(map, np.uint32).reshape(G, G) >= np.uint32(threshold))
    for _ in range(dilate):
        q = np.zeros((G + 2, G + 2), bool)
        q[1:-1, 1:-1] = m
        m = np.zeros((G, G), bool)
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                m |= q[dy:dy + G, dx:dx + G]
    if flags & CELLS_COMPLEMENT:
        m = ~m
    return np.flatnonzero(m.reshape(-1)).astype(np.uint32)


def density_guided(p, cell_list, g, weight=1, plane=None, stats=None, chunk=1 << 16):
    """mc_buddhabrot_density_guided: sample k takes cell_list[k mod n_cells]; its hash words' high bits, shifted down by g, fill the cell;
    every plotted point adds `weight`.  ADDS to plane and stats (zeros when None).  Returns (plane, stats)."""
    cell_list = np.asarray(cell_list, np.uint32)
    n_cells = int(cell_list.size)
    assert n_cells >= 1 and int(cell_list.max()) < (1 << (2 * g))
    plane = np.zeros((int(p.height), int(p.width)), np.uint32) if plane is None else plane
    stats = dict.fromkeys(R.STATS, 0) if stats is None else stats
    for lo in range(int(p.sample_begin), int(p.sample_end), chunk):
        k = np.arange(lo, min(lo + chunk, int(p.sample_end)), dtype=np.uint64)
        j = (k % np.uint64(n_cells)).astype(np.int64)   # (uint64: the 64-bit modulo, exact)
        ux, uy = R.hash_words(k, p.seed)
        ux, uy = guided_words(ux, uy, cell_list[j], g)
        _samples(p, ux, uy, plane.reshape(-1), stats, weight)
    return plane, stats


def complement_range(p, n_cells, n_comp, B):
    """[sample_end, sample_end + ceil(samples * n_comp / (n_cells * B))): the chain's complement pass."""
    samples = int(p.sample_end) - int(p.sample_begin)
    count = -((-samples * n_comp) // (n_cells * B))
    return int(p.sample_end), int(p.sample_end) + count


def render_guided(p, guide):
    """mc_buddhabrot_render_guided: the chain, step by step.  Returns (plane, stats, info), info = dict(n_cells, n_complement, pilot,
    complement) with the two statistics as dicts."""
    from types import SimpleNamespace
    g, B = guide["grid_log2"], guide["complement_weight"]
    pilot = SimpleNamespace(**dict(vars(p), sample_begin=0, sample_end=guide["pilot_samples"]))
    map, _, pst = importance(pilot, g, want_plane=False)
    lst = cells(g, map, guide["threshold"], guide["dilate"])
    comp = cells(g, map, guide["threshold"], guide["dilate"], CELLS_COMPLEMENT)
    info = dict(n_cells=int(lst.size), n_complement=int(comp.size), pilot=pst, complement=dict.fromkeys(R.STATS, 0))
    plane = np.zeros((int(p.height), int(p.width)), np.uint32)
    stats = dict.fromkeys(R.STATS, 0)
    if not lst.size:
        return plane, stats, info
    density_guided(p, lst, g, 1, plane, stats)
    if B > 0 and comp.size:
        lo, hi = complement_range(p, int(lst.size), int(comp.size), B)
        q = SimpleNamespace(**dict(vars(p), sample_begin=lo, sample_end=hi))
        density_guided(q, comp, g, B, plane, info["complement"])
    return plane, stats, info
