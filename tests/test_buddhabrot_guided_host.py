"""The Buddhabrot's importance map, cell list and guided samples on the host (no GPU): mc_buddhabrot_importance,
mc_buddhabrot_importance_cells and mc_buddhabrot_density_guided against the numpy restatement of include/mc_compute.h
(tests/buddhabrot_guided_ref.py), map, plane and statistics EQUAL; the list builder against a numpy dilation; the invariants the
restatement must satisfy too; every refusal with its detail text; the ctypes mirrors' layout."""
import ctypes as C

import numpy as np
import pytest

import buddhabrot_guided_ref as GR
import buddhabrot_ref as R

INVALID = 1
VIEW = (-0.5, 0.0, 3.0, 2.0)
ZOOM = (-0.75, 0.1, 0.2, 0.2 * 32 / 48)
SMALL = dict(width=48, height=32, max_iter=64, view=VIEW)
IMPORTANCE = {
    "default view": dict(SMALL, samples=1 << 14),
    "zoomed M200": dict(width=48, height=32, max_iter=200, view=ZOOM, samples=1 << 15),
    "min_iter 20": dict(width=48, height=32, max_iter=200, min_iter=20, view=VIEW, samples=1 << 14, seed=9),
    "k across 2^32": dict(SMALL, samples=65, sample_begin=(5 << 32) - 17),
    "1 x 1": dict(width=1, height=1, samples=1000, max_iter=64, seed=3, view=(0.0, 0.0, 8.0, 8.0)),
    "nothing reaches the view": dict(SMALL, samples=1 << 12, view=(40.0, 40.0, 1.0, 1.0)),
}
_maps = {}


def restated(name, g):
    """(map, plane, stats tuple) of an importance case by the restatement: computed once, shared, never written to."""
    if (name, g) not in _maps:
        m, plane, st = GR.importance(R.params(**IMPORTANCE[name]), g)
        m.setflags(write=False)
        plane.setflags(write=False)
        _maps[name, g] = (m, plane, R.stats_tuple(st))
    return _maps[name, g]


@pytest.mark.parametrize("g", [1, 6, 12])
@pytest.mark.parametrize("name", list(IMPORTANCE))
def test_importance_equals_the_restatement(B, name, g):
    kw = IMPORTANCE[name]
    want_map, want_plane, ws = restated(name, g)
    m, plane, st = B.buddhabrot_importance(B.buddhabrot_params(**kw), g)
    assert st.as_tuple() == ws and np.array_equal(m, want_map) and np.array_equal(plane, want_plane)
    uniform, us = B.buddhabrot_density(B.buddhabrot_params(**kw))                     # the uniform call's samples, exactly
    assert np.array_equal(plane, uniform) and st.as_tuple() == us.as_tuple()
    m2, none, st2 = B.buddhabrot_importance(B.buddhabrot_params(**kw), g, want_plane=False)   # no plane: the same map and statistics
    assert none is None and st2.as_tuple() == ws and np.array_equal(m2, want_map)
    assert int(m.sum(dtype=np.uint64)) == ws[4]                                       # sum(map) == added
    if name == "nothing reaches the view":
        assert ws[2] > 0 and ws[4] == 0 and not m.any()
    else:
        assert ws[4] > 0


def test_the_map_of_g_is_the_map_of_g_plus_1_summed_2_by_2(B):
    for name in ("default view", "zoomed M200"):
        for g in (1, 5, 11):
            fine = (restated(name, g + 1)[0] if g + 1 in (1, 6, 12) else GR.importance(R.params(**IMPORTANCE[name]), g + 1)[0])
            G = 1 << g
            coarse = fine.reshape(G, 2, G, 2).sum(axis=(1, 3), dtype=np.uint64).astype(np.uint32).reshape(-1)
            assert np.array_equal(GR.importance(R.params(**IMPORTANCE[name]), g)[0], coarse)
            assert np.array_equal(B.buddhabrot_importance(B.buddhabrot_params(**IMPORTANCE[name]), g)[0], coarse)


def test_importance_adds_and_wraps_inside_guard_words(B):
    kw, g = IMPORTANCE["default view"], 3
    fresh = GR.importance(R.params(**kw), g)[0]
    rng = np.random.default_rng(2)
    buf = rng.integers(0, 2 ** 32, 64 + 32, dtype=np.uint32)
    hot = int(np.argmax(fresh))
    buf[16 + hot] = 2 ** 32 - 1                                                         # a word that wraps
    before = buf.copy()
    inner = buf[16:16 + 64]
    st = B.BuddhabrotStats(1, 2, 3, 4, 5)
    N = kw["samples"]
    B.buddhabrot_importance(B.buddhabrot_params(**dict(kw, samples=N // 3)), g, inner, stats=st, want_plane=False)       # two ranges compose
    B.buddhabrot_importance(B.buddhabrot_params(**dict(kw, samples=N - N // 3, sample_begin=N // 3)), g, inner, stats=st, want_plane=False)
    assert np.array_equal(inner, before[16:16 + 64] + fresh) and inner[hot] == fresh[hot] - 1
    assert np.array_equal(buf[:16], before[:16]) and np.array_equal(buf[-16:], before[-16:])
    want = R.stats_tuple(R.density(R.params(**kw))[1])
    assert st.as_tuple() == tuple(a + b for a, b in zip(want, (1, 2, 3, 4, 5)))
    p = B.buddhabrot_params(**kw)
    m = np.zeros(64, np.uint32)
    assert B.lib().mc_buddhabrot_importance(C.byref(p), g, m.ctypes.data_as(C.c_void_p), None, None) == 0   # NULL plane, NULL statistics
    assert np.array_equal(m, fresh)


# ---- the list builder ---------------------------------------------------------------------------------------------------------------
def numpy_dilation(mask, rings):
    """The cells within Chebyshev distance `rings` of a set cell: the 8-neighbourhood grown ring by ring, clipped at the edge."""
    G = mask.shape[0]
    ys, xs = np.nonzero(mask)
    out = np.zeros_like(mask)
    for y, x in zip(ys, xs):
        out[max(0, y - rings):min(G, y + rings + 1), max(0, x - rings):min(G, x + rings + 1)] = True
    return out


def edge_map(g):
    """A set touching all four edges of the grid (and two corners), a lone interior cell, counts on both sides of threshold 5."""
    G = 1 << g
    m = np.zeros((G, G), np.uint32)
    m[0, 0] = 9
    m[0, G // 2] = 5
    m[G - 1, G - 1] = 7
    m[G // 2, 0] = 4
    m[G // 3, G - 1] = 1
    m[G - 1, 1] = 2 ** 32 - 1
    m[G // 2, G // 2] = 5
    m[min(G // 2 + 1, G - 1), min(G // 2 + 3, G - 1)] += 3
    return m


@pytest.mark.parametrize("dilate", [0, 1, 8])
@pytest.mark.parametrize("threshold", [1, 5])
@pytest.mark.parametrize("g", [1, 5, 6])
def test_cell_list_against_a_numpy_dilation(B, g, threshold, dilate):
    G = 1 << g
    for m in (edge_map(g), restated("zoomed M200", 6)[0].reshape(64, 64) if g == 6 else edge_map(g).T.copy()):
        mask = numpy_dilation(m >= threshold, dilate)
        want = np.flatnonzero(mask.reshape(-1)).astype(np.uint32)
        got = B.buddhabrot_importance_cells(g, m, threshold, dilate)
        assert got.dtype == np.uint32 and np.array_equal(got, want) and np.array_equal(GR.cells(g, m, threshold, dilate), want)
        comp = B.buddhabrot_importance_cells(g, m, threshold, dilate, B.BUDDHA_CELLS_COMPLEMENT)
        assert np.array_equal(comp, np.flatnonzero(~mask.reshape(-1))) and np.array_equal(GR.cells(g, m, threshold, dilate, 1), comp)
        assert got.size + comp.size == G * G and got.size > 0


def test_cell_list_empty_and_full(B):
    g, G = 4, 16
    empty = np.zeros(G * G, np.uint32)
    for dilate in (0, 8):
        assert B.buddhabrot_importance_cells(g, empty, 1, dilate).size == 0                     # valid: n_cells = 0
        assert np.array_equal(B.buddhabrot_importance_cells(g, empty, 1, dilate, 1), np.arange(G * G))
    full = np.full(G * G, 3, np.uint32)
    assert np.array_equal(B.buddhabrot_importance_cells(g, full, 3, 1), np.arange(G * G))
    assert B.buddhabrot_importance_cells(g, full, 3, 1, 1).size == 0 and B.buddhabrot_importance_cells(g, full, 4, 8).size == 0
    one = empty.copy()
    one[5 * G + 7] = 1
    assert B.buddhabrot_importance_cells(g, one, 1, 8).size == (5 + 8 + 1) * G                   # rows 0 .. 13, every column: clipped
    n = C.c_uint32(77)
    assert B.lib().mc_buddhabrot_importance_cells(g, one.ctypes.data_as(C.c_void_p), 1, 1, 0, None, C.byref(n)) == 0 and n.value == 9


# ---- guided density -----------------------------------------------------------------------------------------------------------------
def boundary_cells(g=6):
    return GR.cells(g, restated("zoomed M200", 6)[0], 1, 0)


GUIDED = {   # (params keywords, the list, g, weight)
    "zoomed list": (dict(width=48, height=32, max_iter=200, view=ZOOM, samples=1 << 12), "boundary", 6, 1),
    "weight 7, 3 cells": (dict(width=48, height=32, max_iter=200, view=ZOOM, samples=1000), "boundary3", 6, 7),
    "k across 2^32, 3 cells": (dict(width=48, height=32, max_iter=200, view=ZOOM, samples=65, sample_begin=(5 << 32) - 17), "boundary3", 6, 1),
    "near 2^40, 1000 cells": (dict(SMALL, samples=65, sample_begin=1000 * ((1 << 40) // 1000 + 1) - 30), "first1000", 6, 1),
    "corners g = 1": (dict(SMALL, samples=1 << 10), [0, 3], 1, 1),
    "corners g = 12": (dict(SMALL, samples=1 << 10), [0, (1 << 24) - 1, 2048 * 4096 + 1500], 12, 2),
    "repeated cell": (dict(SMALL, samples=1 << 10), "repeated", 6, 1),
}


def guided_list(which):
    if isinstance(which, list):
        return np.array(which, np.uint32)
    b = boundary_cells()
    return {"boundary": b, "boundary3": b[[0, b.size // 2, b.size - 1]], "first1000": np.arange(1000, dtype=np.uint32),
            "repeated": np.array([2080, 2081, 2080, 2080, 1500], np.uint32)}[which]


@pytest.mark.parametrize("name", list(GUIDED))
def test_guided_equals_the_restatement(B, name):
    kw, which, g, weight = GUIDED[name]
    lst = guided_list(which)
    want, ws = GR.density_guided(R.params(**kw), lst, g, weight)
    got, gs = B.buddhabrot_density_guided(B.buddhabrot_params(**kw), lst, g, weight)
    assert gs.as_tuple() == R.stats_tuple(ws) and np.array_equal(got, want)
    assert int(got.sum(dtype=np.uint64)) == weight * ws["added"]
    if "corners" not in name:
        assert ws["added"] > 0
    # every sample lies in its cell: the cell of the guided words is the list's entry
    k = np.arange(kw.get("sample_begin", 0), kw.get("sample_begin", 0) + kw["samples"], dtype=np.uint64)
    j = (k % np.uint64(lst.size)).astype(np.int64)
    ux, uy = GR.guided_words(*R.hash_words(k, kw.get("seed", 1)), lst[j], g)
    assert np.array_equal(GR.cell_of(ux, uy, g), lst[j].astype(np.int64))


def test_guided_over_the_whole_grid_at_g_1_matches_the_window(B):
    """The four cells of g = 1 tile the sample window: guided samples fall in every quadrant the list names, and only there."""
    kw = dict(SMALL, samples=1 << 10)
    p = R.params(**kw)
    k = np.arange(1 << 10, dtype=np.uint64)
    for cell in range(4):
        ux, uy = GR.guided_words(*R.hash_words(k, 1), np.full(k.size, cell), 1)
        cx, cy = GR._c_of_words(p, ux, uy)
        assert ((cx >= -0.5) == bool(cell & 1)).all() and ((cy >= 0.0) == bool(cell & 2)).all()
        assert cx.min() >= -2.5 and cx.max() < 1.5 and cy.min() >= -2.0 and cy.max() < 2.0


def test_guided_ranges_compose_weights_wrap_and_stats_add(B):
    kw, which, g, _ = GUIDED["zoomed list"]
    lst = guided_list(which)
    N = kw["samples"]
    whole, ws = GR.density_guided(R.params(**kw), lst, g, 1)
    plane, st = B.buddhabrot_density_guided(B.buddhabrot_params(**dict(kw, samples=N // 3)), lst, g)
    plane, st = B.buddhabrot_density_guided(B.buddhabrot_params(**dict(kw, samples=N - N // 3, sample_begin=N // 3)), lst, g, 1, plane, st)
    assert np.array_equal(plane, whole) and st.as_tuple() == R.stats_tuple(ws)
    rng = np.random.default_rng(3)
    pre = rng.integers(0, 2 ** 32, (32, 48), dtype=np.uint32)
    got, _ = B.buddhabrot_density_guided(B.buddhabrot_params(**kw), lst, g, 1 << 31, pre.copy())
    assert np.array_equal(got, pre + whole * np.uint32(1 << 31)) and (whole % 2 == 1).any()      # (uint32: wraps as the plane does)
    assert np.array_equal(got, GR.density_guided(R.params(**kw), lst, g, 1 << 31, pre.copy())[0])


def test_list_plus_complement_covers_every_cell_once(B):
    """The composition the header states: list and complement partition the grid, so at equal samples per cell and weight 1 their sum
    visits every cell of the grid equally often."""
    g, G2 = 3, 64
    lst = np.array([9, 10, 17, 18, 30], np.uint32)
    m = np.zeros(G2, np.uint32)
    m[lst] = 1
    comp = B.buddhabrot_importance_cells(g, m, 1, 0, 1)
    assert np.array_equal(B.buddhabrot_importance_cells(g, m, 1, 0), lst) and np.array_equal(np.sort(np.concatenate([lst, comp])), np.arange(G2))
    kw = dict(SMALL)
    a, sa = B.buddhabrot_density_guided(B.buddhabrot_params(samples=4 * lst.size, **kw), lst, g)
    b, sb = B.buddhabrot_density_guided(B.buddhabrot_params(samples=4 * comp.size, sample_begin=4 * lst.size, **kw), comp, g, 1, a, sa)
    assert sb.samples == 4 * G2
    lo, hi = GR.complement_range(R.params(samples=4 * lst.size, **kw), lst.size, comp.size, 4)
    assert (lo, hi) == (20, 20 + comp.size)                                                      # N / B = 1 sample per cell


# ---- validation ---------------------------------------------------------------------------------------------------------------------
def test_refusals(B):
    L = B.lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    detail = lambda: L.mc_last_error_detail().decode()
    p = B.buddhabrot_params(8, 8, 10, max_iter=8)
    m = np.zeros(16, np.uint32)
    plane = np.zeros((8, 8), np.uint32)
    cells = np.array([0, 15], np.uint32)
    n = C.c_uint32(0)
    out = np.zeros(16, np.uint32)
    for call, who, cases in (
        (lambda g=2, mp=m, q=p: L.mc_buddhabrot_importance(C.byref(q) if q is not None else None, g, None if mp is None else vp(mp), vp(plane), None),
         "mc_buddhabrot_importance",
         [(dict(g=0), "grid_log2 is outside 1 .. 12"), (dict(g=13), "grid_log2 is outside 1 .. 12"), (dict(mp=None), "map is NULL"),
          (dict(q=None), "p is NULL")]),
        (lambda g=2, mp=m, t=1, d=0, f=0, np_=n: L.mc_buddhabrot_importance_cells(g, None if mp is None else vp(mp), t, d, f, vp(out),
                                                                                None if np_ is None else C.byref(np_)),
         "mc_buddhabrot_importance_cells",
         [(dict(g=0), "grid_log2 is outside 1 .. 12"), (dict(g=13), "grid_log2 is outside 1 .. 12"), (dict(mp=None), "map is NULL"),
          (dict(np_=None), "n_cells is NULL"), (dict(t=0), "threshold is 0"), (dict(d=9), "dilate exceeds 8"), (dict(f=2), "flags has unknown bits")]),
        (lambda g=2, c=cells, nc=2, w=1, pl=plane, q=p: L.mc_buddhabrot_density_guided(C.byref(q), None if c is None else vp(c), nc, g, w,
                                                                                     None if pl is None else vp(pl), None),
         "mc_buddhabrot_density_guided",
         [(dict(g=0), "grid_log2 is outside 1 .. 12"), (dict(g=13), "grid_log2 is outside 1 .. 12"), (dict(c=None), "cells is NULL"),
          (dict(nc=0), "n_cells is 0"), (dict(w=0), "weight is 0"), (dict(pl=None), "plane is NULL"),
          (dict(c=np.array([0, 16], np.uint32)), "a cell index is outside the grid"), (dict(g=1), "a cell index is outside the grid")]),
    ):
        assert call() == 0, who
        before = (plane.copy(), m.copy(), out.copy())
        for change, text in cases:
            assert call(**change) == INVALID, (who, change)
            assert all(np.array_equal(a, b) for a, b in zip(before, (plane, m, out))), (who, change)   # a refused call writes nothing
            assert text in detail() and detail().startswith(who + ":"), (who, change, detail())
    bad = B.buddhabrot_params(8, 8, 10, max_iter=8)
    bad.max_iter = 0
    for call, who in ((lambda: L.mc_buddhabrot_importance(C.byref(bad), 2, vp(m), None, None), "mc_buddhabrot_importance"),
                      (lambda: L.mc_buddhabrot_density_guided(C.byref(bad), vp(cells), 2, 2, 1, vp(plane), None), "mc_buddhabrot_density_guided")):
        assert call() == INVALID and detail() == who + ": max_iter is 0"
    assert L.mc_buddhabrot_guide_default_params(None) == INVALID and "out is NULL" in detail()


def test_guide_defaults_and_struct_layout(B):
    g = B.buddhabrot_guide_params()
    assert (g.grid_log2, g.pilot_samples, g.threshold, g.dilate, g.complement_weight) == (8, 1 << 24, 1, 1, 0)
    assert {k: getattr(g, k) for k in GR.GUIDE_DEFAULTS} == GR.GUIDE_DEFAULTS
    P, I = B.BuddhabrotGuideParams, B.BuddhabrotGuideInfo
    assert C.sizeof(P) == 24 and [getattr(P, f).offset for f, _ in P._fields_] == [0, 4, 8, 16, 20]
    assert C.sizeof(I) == 88 and [getattr(I, f).offset for f, _ in I._fields_] == [0, 4, 8, 48]
    assert C.sizeof(B.BuddhabrotParams) == 104 and B.BUDDHA_CELLS_COMPLEMENT == 1 == GR.CELLS_COMPLEMENT


def test_restated_chain_is_the_separate_calls(B):
    """render_guided of the restatement (what the GPU suite holds mc_buddhabrot_render_guided to) against the host calls chained by hand."""
    kw = dict(width=48, height=32, max_iter=100, view=ZOOM, samples=3000, sample_begin=11)
    guide = dict(grid_log2=5, pilot_samples=1 << 13, threshold=1, dilate=1, complement_weight=4)
    plane, st, info = GR.render_guided(R.params(**kw), guide)
    m, _, pst = B.buddhabrot_importance(B.buddhabrot_params(**dict(kw, samples=1 << 13, sample_begin=0)), 5, want_plane=False)
    lst = B.buddhabrot_importance_cells(5, m, 1, 1)
    comp = B.buddhabrot_importance_cells(5, m, 1, 1, 1)
    assert (info["n_cells"], info["n_complement"]) == (lst.size, comp.size) and 0 < lst.size < 1024
    assert pst.as_tuple() == R.stats_tuple(info["pilot"]) and pst.added > 0
    got, gs = B.buddhabrot_density_guided(B.buddhabrot_params(**kw), lst, 5)
    assert gs.as_tuple() == R.stats_tuple(st)
    count = -(-3000 * comp.size // (lst.size * 4))
    got, cs = B.buddhabrot_density_guided(B.buddhabrot_params(**dict(kw, samples=count, sample_begin=3011)), comp, 5, 4, got)
    assert cs.as_tuple() == R.stats_tuple(info["complement"]) and cs.samples == count and np.array_equal(got, plane)
