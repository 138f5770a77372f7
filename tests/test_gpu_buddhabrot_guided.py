"""The Buddhabrot's importance map, guided density and the blocking chain on the MI355X: every case checks the device map, plane AND
the five statistics EQUAL to the numpy restatement of include/mc_compute.h (tests/buddhabrot_guided_ref.py) for the shipped form and
for both forms through their measurement bits.  Shapes are the smallest at which the kernels can still go wrong: one lane, one wave and
one more, a refilled run and its tail, k across 2^32 and a 64-bit k mod n_cells near 2^40, lists of 1 and 3 cells (the modulo turns over
inside every refill), of 64, 65 and more cells than samples, the grid's corner cells, g = 1 and 12, waves that skip or never plot,
lanes in both phases with orbit lengths from 0 to 2000.  Before a case is used the restatement is asserted to make it what it is meant
to be.  Then the chain against the separate calls and the app end to end."""
import os
import subprocess

import numpy as np
import pytest

import buddhabrot_guided_ref as GR
import buddhabrot_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "mandelbrot")
VIEW = (-0.5, 0.0, 3.0, 2.0)
ZOOM = (-0.75, 0.1, 0.2, 0.133)
SMALL = dict(width=48, height=32, max_iter=64, view=VIEW)
FORMS = [0, 1, 2]   # the shipped choice, MC_BUDDHA_KERNEL_PLAIN, MC_BUDDHA_KERNEL_POOLED
FORM_IDS = ["shipped", "plain", "pooled"]
GRIDS = [1, 6, 12]

IMPORTANCE = {
    "1 sample": dict(SMALL, samples=1),
    "63 samples": dict(SMALL, samples=63),
    "64 samples": dict(SMALL, samples=64),
    "65 samples": dict(SMALL, samples=65),
    "1000 samples": dict(SMALL, samples=1000),
    "2^16 + 1 samples": dict(SMALL, samples=(1 << 16) + 1),
    "nothing reaches the view": dict(SMALL, samples=1 << 12, view=(40.0, 40.0, 1.0, 1.0)),
    "1 x 1": dict(width=1, height=1, samples=1000, max_iter=64, seed=3, view=(0.0, 0.0, 8.0, 8.0)),
    "k across 2^32": dict(SMALL, samples=65, sample_begin=(5 << 32) - 17),
}
_importance = {}


def importance_reference(name):
    """{g: map}, plane, stats tuple of an importance case by the restatement: computed once, shared, never written to."""
    if name not in _importance:
        p = R.params(**IMPORTANCE[name])
        maps, plane, st = {}, None, None
        for g in GRIDS:
            maps[g], plane, st = GR.importance(p, g)
            maps[g].setflags(write=False)
        plane.setflags(write=False)
        _importance[name] = (maps, plane, R.stats_tuple(st))
    return _importance[name]


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def stats_of(d_stats):
    return tuple(int(v) for v in d_stats.cpu().numpy().view(np.uint64))


def device_importance(ctx, B, kws, g, flags=0, with_plane=True, want_stats=True, streams=None):
    """The requests `kws` launched into ONE zeroed device map, plane (unless with_plane is false) and statistics record.  Returns
    (map, plane or None, stats tuple or None)."""
    import torch
    p0 = B.buddhabrot_params(**kws[0])
    d_map = torch.zeros(1 << (2 * g), dtype=torch.int32, device="cuda")
    d_plane = torch.zeros(p0.height * p0.width, dtype=torch.int32, device="cuda")
    d_stats = torch.zeros(5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for j, kw in enumerate(kws):
        ctx.buddhabrot_importance_device(B.buddhabrot_params(flags=flags, **kw), g, d_map.data_ptr(), d_plane.data_ptr() if with_plane else 0,
                                         d_stats.data_ptr() if want_stats else 0, stream=streams[j % len(streams)].cuda_stream if streams else 0)
    for s in streams or []:
        s.synchronize()
    ctx.synchronize()
    torch.cuda.synchronize()
    plane = d_plane.cpu().numpy().view(np.uint32).reshape(p0.height, p0.width)
    if not with_plane:
        assert not plane.any()   # no plane add was issued anywhere
    return d_map.cpu().numpy().view(np.uint32), (plane if with_plane else None), (stats_of(d_stats) if want_stats else None)


def device_guided(ctx, B, kws, cells, g, weight=1, flags=0, plane=None, want_stats=True, streams=None):
    """The guided requests `kws` over one device list into ONE device plane (starting from `plane`) and one statistics record."""
    import torch
    p0 = B.buddhabrot_params(**kws[0])
    start = np.zeros((p0.height, p0.width), np.uint32) if plane is None else plane
    d_plane, d_cells = to_device(start), to_device(np.asarray(cells, np.uint32))
    d_stats = torch.zeros(5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for j, kw in enumerate(kws):
        ctx.buddhabrot_guided_device(B.buddhabrot_params(flags=flags, **kw), d_cells.data_ptr(), len(cells), g, weight, d_plane.data_ptr(),
                                     d_stats.data_ptr() if want_stats else 0, stream=streams[j % len(streams)].cuda_stream if streams else 0)
    for s in streams or []:
        s.synchronize()
    ctx.synchronize()
    torch.cuda.synchronize()
    return d_plane.cpu().numpy().view(np.uint32).reshape(start.shape), (stats_of(d_stats) if want_stats else None)


# ---- importance ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("name", list(IMPORTANCE))
def test_importance_equals_the_restatement(ctx, B, name, flags):
    maps, want_plane, ws = importance_reference(name)
    if name == "nothing reaches the view":
        assert ws[2] > 0 and ws[4] == 0 and not maps[6].any()
    elif name == "1 x 1":
        assert ws[4] > 1000 and np.count_nonzero(maps[1]) <= 4          # many adds to few map words
    elif name != "1 sample":
        assert ws[4] > 0
    for g in GRIDS:
        for with_plane in (True, False):
            m, plane, gs = device_importance(ctx, B, [IMPORTANCE[name]], g, flags, with_plane)
            assert gs == ws, (g, with_plane, gs, ws)
            assert np.array_equal(m, maps[g]), (g, with_plane, int((m != maps[g]).sum()))
            assert plane is None or np.array_equal(plane, want_plane)
    if flags == 0:   # with a plane: the plane and the statistics are mc_buddhabrot_density's
        uniform, us = ctx.buddhabrot(B.buddhabrot_params(**IMPORTANCE[name]))
        assert np.array_equal(uniform, want_plane) and us.as_tuple() == ws


@pytest.mark.parametrize("flags", FORMS, ids=FORM_IDS)
def test_importance_two_ranges_two_streams_one_map(ctx, B, flags):
    import torch
    maps, want_plane, ws = importance_reference("2^16 + 1 samples")
    N = (1 << 16) + 1
    parts = [dict(SMALL, samples=N // 3), dict(SMALL, samples=N - N // 3, sample_begin=N // 3)]
    for streams in (None, [torch.cuda.Stream(), torch.cuda.Stream()]):
        m, plane, gs = device_importance(ctx, B, parts, 6, flags, streams=streams)
        assert gs == ws and np.array_equal(m, maps[6]) and np.array_equal(plane, want_plane)


@pytest.mark.parametrize("flags", FORMS, ids=FORM_IDS)
def test_importance_prefilled_map_guard_words_and_null_stats(ctx, B, flags):
    g, kw = 3, IMPORTANCE["1000 samples"]
    fresh = GR.importance(R.params(**kw), g, want_plane=False)[0]
    hot = int(np.argmax(fresh))
    assert fresh[hot] > 1
    rng = np.random.default_rng(7)
    before = rng.integers(0, 2 ** 32, 64 + 32, dtype=np.uint32)
    before[16 + hot] = 2 ** 32 - 1                                       # a map word that wraps
    buf = to_device(before)
    ctx.synchronize()
    ctx.buddhabrot_importance_device(B.buddhabrot_params(flags=flags, **kw), g, buf.data_ptr() + 64)   # d_plane = d_stats = NULL
    ctx.synchronize()
    after = buf.cpu().numpy().view(np.uint32)
    assert np.array_equal(after[16:16 + 64], before[16:16 + 64] + fresh) and after[16 + hot] == fresh[hot] - 1
    assert np.array_equal(after[:16], before[:16]) and np.array_equal(after[-16:], before[-16:])


# ---- guided -------------------------------------------------------------------------------------------------------------------------
def _lists():
    """Cell lists of the 64 x 64 grid over the default window, from the restated map of the default view: the hottest cells first."""
    m = GR.importance(R.params(**dict(SMALL, samples=1 << 14)), 6, want_plane=False)[0]
    order = np.argsort(-m.astype(np.int64), kind="stable").astype(np.uint32)
    assert m[order[64]] > 0
    grown = GR.cells(6, m, 1, 1)
    assert grown.size >= 1000
    return {1: order[:1], 3: order[:3], 64: order[:64], 65: order[:65], 1000: grown[:1000]}


_cache = {}


def lists():
    if "lists" not in _cache:
        _cache["lists"] = _lists()
    return _cache["lists"]


def guided_reference(key, kw, cells, g, weight=1):
    if key not in _cache:
        plane, st = GR.density_guided(R.params(**kw), cells, g, weight)
        plane.setflags(write=False)
        _cache[key] = (plane, R.stats_tuple(st))
    return _cache[key]


@pytest.mark.parametrize("flags", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("n_cells", [1, 3, 64, 65, 1000])
def test_guided_list_lengths_and_sample_counts(ctx, B, n_cells, flags):
    cells = lists()[n_cells]
    for samples in (1, 63, 64, 65, 1000):
        kw = dict(SMALL, samples=samples)
        want, ws = guided_reference(("len", n_cells, samples), kw, cells, 6)
        assert samples < 63 or ws[4] > 0
        got, gs = device_guided(ctx, B, [kw], cells, 6, 1, flags)
        assert gs == ws, (samples, gs, ws)
        assert np.array_equal(got, want), (samples, int((got != want).sum()))


def _near_2_40(n):
    return n * ((1 << 40) // n + 1) - 30   # 65 samples from here cross a multiple of n just above 2^40


RANGES = {
    "k across 2^32, 3 cells": (dict(SMALL, samples=65, sample_begin=(5 << 32) - 17), 3),
    "k across 2^32, 1000 cells": (dict(SMALL, samples=65, sample_begin=(5 << 32) - 17), 1000),
    "a multiple of 3 near 2^40": (dict(SMALL, samples=65, sample_begin=_near_2_40(3)), 3),
    "a multiple of 1000 near 2^40": (dict(SMALL, samples=65, sample_begin=_near_2_40(1000)), 1000),
    "a multiple of 65 near 2^40, 1000 samples": (dict(SMALL, samples=1000, sample_begin=_near_2_40(65)), 65),
}


@pytest.mark.parametrize("flags", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("name", list(RANGES))
def test_guided_64_bit_modulo(ctx, B, name, flags):
    kw, n_cells = RANGES[name]
    cells = lists()[n_cells]
    want, ws = guided_reference(("range", name), kw, cells, 6)
    k = np.arange(kw["sample_begin"], kw["sample_begin"] + kw["samples"], dtype=np.uint64)
    j = [int(q) % n_cells for q in k.tolist()]                            # python integers: the modulo beyond doubt
    begin, end = kw["sample_begin"], kw["sample_begin"] + kw["samples"]
    assert ws[4] > 0 and ((begin >> 32) != (end >> 32) if begin < 1 << 40 else 0 in j[1:])   # the range crosses what it is meant to cross
    low = GR.density_guided(R.params(**dict(kw, sample_begin=kw["sample_begin"] & 0xffffffff)), cells, 6)[0]
    assert not np.array_equal(low, want)                                  # the high word of k reaches the samples
    got, gs = device_guided(ctx, B, [kw], cells, 6, 1, flags)
    assert gs == ws and np.array_equal(got, want)


HOT = 33 * 64 + 28                # g = 6: c in [-0.75, -0.6875) x [0.0625, 0.125), on the boundary
CARDIOID, FAR = 32 * 64 + 38, 0   # g = 6: c in [-0.125, -0.0625) x [0, 0.0625), inside the cardioid; c near (-2.5, -2), |c|^2 > 4
CELLS = {   # name: (params keywords, list, g, weight)
    "cells 0 and G^2 - 1": (dict(SMALL, samples=1000), [0, 4095], 6, 1),
    "g = 1": (dict(SMALL, samples=1000), [0, 3, 1], 1, 1),
    "g = 12": (dict(SMALL, samples=1000), [0, (1 << 24) - 1, 2150 * 4096 + 1792, 2151 * 4096 + 1790], 12, 1),
    "inside the cardioid": (dict(SMALL, samples=1000), [CARDIOID], 6, 1),
    "far outside": (dict(SMALL, samples=1000), [FAR], 6, 1),
    "a repeated cell": (dict(SMALL, samples=1000), [HOT, HOT + 1, HOT, HOT, CARDIOID], 6, 1),
    "boundary-hugging M2000": (dict(width=48, height=32, max_iter=2000, view=VIEW, samples=1 << 12), [33 * 64 + 28, 33 * 64 + 27, 34 * 64 + 28], 6, 1),
}


@pytest.mark.parametrize("flags", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("name", list(CELLS))
def test_guided_cell_choices(ctx, B, name, flags):
    kw, cells, g, weight = CELLS[name]
    want, ws = guided_reference(("cells", name), kw, cells, g, weight)
    if name == "inside the cardioid":
        assert ws == (1000, 1000, 0, 0, 0)
    elif name in ("far outside", "cells 0 and G^2 - 1"):
        assert ws == (1000, 0, 1000, 0, 0)                                # classify ends at i = 0: contributing, nothing plotted
    elif name == "boundary-hugging M2000" and flags == 0:
        k = np.arange(1 << 12, dtype=np.uint64)
        ux, uy = GR.guided_words(*R.hash_words(k, 1), np.asarray(cells)[k.astype(np.int64) % 3], g)
        cx, cy = GR._c_of_words(R.params(**kw), ux, uy)
        n = R.classify(cx, cy, 2000)[~R.interior(cx, cy)]
        assert ws[1] > 100 and n.min() < 30 and ((n > 1000) & (n < 2000)).any() and (n == 2000).any() and ws[4] > 10000
    else:
        assert ws[4] > 0
    got, gs = device_guided(ctx, B, [kw], cells, g, weight, flags)
    assert gs == ws and np.array_equal(got, want), (gs, ws)


@pytest.mark.parametrize("flags", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("weight", [1, 7, 1 << 31])
def test_guided_weights_on_a_prefilled_plane_inside_guard_words(ctx, B, weight, flags):
    kw = dict(width=7, height=5, max_iter=64, view=VIEW, samples=1000)
    cells = lists()[65]
    ones, ws = guided_reference(("weights",), kw, cells, 6)
    assert (ones % 2 == 1).any() and ones.max() > 1                     # 2^31 times an odd count wraps to 2^31, an even one to 0
    rng = np.random.default_rng(weight & 0xff)
    before = rng.integers(0, 2 ** 32, 35 + 32, dtype=np.uint32)
    buf = to_device(before)
    d_cells = to_device(cells)
    ctx.synchronize()
    ctx.buddhabrot_guided_device(B.buddhabrot_params(flags=flags, **kw), d_cells.data_ptr(), 65, 6, weight, buf.data_ptr() + 64)   # d_stats = NULL
    ctx.synchronize()
    after = buf.cpu().numpy().view(np.uint32)
    assert np.array_equal(after[16:16 + 35], before[16:16 + 35] + ones.reshape(-1) * np.uint32(weight))   # (uint32: wraps as the plane does)
    assert np.array_equal(after[:16], before[:16]) and np.array_equal(after[-16:], before[-16:])
    got, gs = device_guided(ctx, B, [kw], cells, 6, weight, flags)
    assert gs == ws and np.array_equal(got, GR.density_guided(R.params(**kw), cells, 6, weight)[0])        # added counts points, not weight


@pytest.mark.parametrize("flags", FORMS, ids=FORM_IDS)
def test_guided_ranges_and_streams_compose(ctx, B, flags):
    import torch
    cells = lists()[65]
    N = 1 << 12
    want, ws = guided_reference(("compose",), dict(SMALL, samples=N, sample_begin=5), cells, 6)
    parts = [dict(SMALL, samples=N // 3, sample_begin=5), dict(SMALL, samples=N - N // 3, sample_begin=5 + N // 3)]
    for streams in (None, [torch.cuda.Stream(), torch.cuda.Stream()]):
        got, gs = device_guided(ctx, B, parts, cells, 6, 1, flags, streams=streams)
        assert gs == ws and np.array_equal(got, want)


def test_a_cell_beyond_the_grid_is_clamped_on_the_device_and_refused_on_the_host(ctx, B):
    kw = dict(SMALL, samples=1000)
    broken, clamped = np.array([5000, HOT], np.uint32), np.array([4095, HOT], np.uint32)
    want, ws = guided_reference(("clamped",), kw, clamped, 6)
    assert ws[4] > 0
    for flags in FORMS:
        got, gs = device_guided(ctx, B, [kw], broken, 6, 1, flags)
        assert gs == ws and np.array_equal(got, want)
    with pytest.raises(B.McError) as e:
        B.buddhabrot_density_guided(B.buddhabrot_params(**kw), broken, 6)
    assert e.value.status == 1 and "a cell index is outside the grid" in str(e.value)


def test_device_refusals(ctx, B):
    import torch
    d = torch.zeros(256, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    p = B.buddhabrot_params(8, 8, 10, max_iter=8)
    ptr = d.data_ptr()
    for call, detail in (
        (lambda: ctx.buddhabrot_importance_device(p, 0, ptr, ptr + 512), "grid_log2 is outside 1 .. 12"),
        (lambda: ctx.buddhabrot_importance_device(p, 13, ptr, ptr + 512), "grid_log2 is outside 1 .. 12"),
        (lambda: ctx.buddhabrot_importance_device(p, 2, 0, ptr + 512), "d_map is NULL"),
        (lambda: ctx.buddhabrot_importance_device(p, 2, ptr + 2, ptr + 512), "d_map is NULL or not 4-byte aligned"),
        (lambda: ctx.buddhabrot_importance_device(p, 2, ptr, ptr + 512, ptr + 4), "d_stats 8-byte aligned"),
        (lambda: ctx.buddhabrot_guided_device(p, ptr, 4, 0, 1, ptr + 512), "grid_log2 is outside 1 .. 12"),
        (lambda: ctx.buddhabrot_guided_device(p, 0, 4, 2, 1, ptr + 512), "cells is NULL"),
        (lambda: ctx.buddhabrot_guided_device(p, ptr, 0, 2, 1, ptr + 512), "n_cells is 0"),
        (lambda: ctx.buddhabrot_guided_device(p, ptr, 4, 2, 0, ptr + 512), "weight is 0"),
        (lambda: ctx.buddhabrot_guided_device(p, ptr, 4, 2, 1, 0), "ctx or d_plane is NULL"),
        (lambda: ctx.buddhabrot_guided_device(p, ptr + 2, 4, 2, 1, ptr + 512), "d_cells must be 4-byte aligned"),
        (lambda: ctx.buddhabrot_guided(p, B.buddhabrot_guide_params(grid_log2=13)), "grid_log2 is outside 1 .. 12"),
        (lambda: ctx.buddhabrot_guided(p, B.buddhabrot_guide_params(threshold=0)), "threshold is 0"),
        (lambda: ctx.buddhabrot_guided(p, B.buddhabrot_guide_params(dilate=9)), "dilate exceeds 8"),
        (lambda: ctx.buddhabrot_guided(p, B.buddhabrot_guide_params(pilot_samples=(1 << 40) + 1)), "pilot_samples exceeds 2^40"),
    ):
        with pytest.raises(B.McError) as e:
            call()
        assert e.value.status == 1 and detail in str(e.value), e.value
    bad = B.buddhabrot_params(8, 8, 10, max_iter=8)
    bad.flags = 3
    for call in (lambda: ctx.buddhabrot_importance_device(bad, 2, ptr), lambda: ctx.buddhabrot_guided_device(bad, ptr, 4, 2, 1, ptr + 512),
                 lambda: ctx.buddhabrot_guided(bad, B.buddhabrot_guide_params())):
        with pytest.raises(B.McError) as e:
            call()
        assert "names both" in str(e.value)
    ctx.synchronize()
    assert not d.cpu().numpy().any()


# ---- the chain ----------------------------------------------------------------------------------------------------------------------
CHAIN = dict(width=96, height=64, max_iter=200, view=ZOOM, samples=1 << 16)
GUIDE = dict(grid_log2=6, pilot_samples=1 << 16, threshold=1, dilate=1)


def chain_by_hand(ctx, B, kw, guide, flags=0):
    """The chain through the separate calls: (plane, stats tuple, pilot stats tuple, list, complement, complement stats tuple)."""
    g, Bw = guide["grid_log2"], guide.get("complement_weight", 0)
    m, _, pst = device_importance(ctx, B, [dict(kw, samples=guide["pilot_samples"], sample_begin=0)], g, flags, with_plane=False)
    lst = B.buddhabrot_importance_cells(g, m, guide["threshold"], guide["dilate"])
    comp = B.buddhabrot_importance_cells(g, m, guide["threshold"], guide["dilate"], B.BUDDHA_CELLS_COMPLEMENT)
    plane, st = device_guided(ctx, B, [kw], lst, g, 1, flags)
    cst = (0, 0, 0, 0, 0)
    if Bw and comp.size:
        begin = kw.get("sample_begin", 0) + kw["samples"]
        count = -(-kw["samples"] * int(comp.size) // (int(lst.size) * Bw))
        plane, cst = device_guided(ctx, B, [dict(kw, samples=count, sample_begin=begin)], comp, g, Bw, flags, plane=plane)
    return plane, st, pst, lst, comp, cst


@pytest.mark.parametrize("flags", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("weight", [0, 4], ids=["list alone", "complement at weight 4"])
def test_render_guided_equals_the_chain_by_hand(ctx, B, weight, flags):
    guide = dict(GUIDE, complement_weight=weight)
    if ("chain", weight) not in _cache:
        _cache["chain", weight] = GR.render_guided(R.params(**CHAIN), guide)
    want, ws, winfo = _cache["chain", weight]
    assert 0 < winfo["n_cells"] < 4096 // 4 and ws["added"] > 4 * winfo["pilot"]["added"] > 0     # the case is a zoomed view worth guiding
    assert (winfo["complement"]["samples"] > 0) == (weight > 0)
    hand, hs, pst, lst, comp, cst = chain_by_hand(ctx, B, CHAIN, guide, flags)
    plane, st, info = ctx.buddhabrot_guided(B.buddhabrot_params(flags=flags, **CHAIN), B.buddhabrot_guide_params(**guide))
    k, c = ctx.last_timing()
    assert k > 0 and c >= 0
    assert (info.n_cells, info.n_complement) == (lst.size, comp.size) == (winfo["n_cells"], winfo["n_complement"])
    assert st.as_tuple() == hs == R.stats_tuple(ws)
    assert info.pilot.as_tuple() == pst == R.stats_tuple(winfo["pilot"])
    assert info.complement.as_tuple() == cst == R.stats_tuple(winfo["complement"])
    assert np.array_equal(plane, hand) and np.array_equal(plane, want)


def test_render_guided_empty_list_and_reuse(ctx, B):
    kw = dict(CHAIN, view=(40.0, 40.0, 1.0, 1.0), samples=1 << 12)
    for weight in (0, 4):
        plane, st, info = ctx.buddhabrot_guided(B.buddhabrot_params(**kw), B.buddhabrot_guide_params(**dict(GUIDE, pilot_samples=1 << 12, complement_weight=weight)))
        assert not plane.any() and st.as_tuple() == (0, 0, 0, 0, 0)
        assert (info.n_cells, info.n_complement) == (0, 4096) and info.pilot.samples == 1 << 12 and info.pilot.added == 0
        assert info.pilot.contributing > 0 and info.complement.as_tuple() == (0, 0, 0, 0, 0)
    # a pilot of no samples is an empty list too; and the next render starts from zero again, with another grid
    plane, st, info = ctx.buddhabrot_guided(B.buddhabrot_params(**CHAIN), B.buddhabrot_guide_params(**dict(GUIDE, pilot_samples=0)))
    assert not plane.any() and info.n_cells == 0 and info.pilot.samples == 0
    guide = dict(GUIDE, grid_log2=4, pilot_samples=1 << 14)
    kw = dict(SMALL, samples=1000)
    plane, st, info = ctx.buddhabrot_guided(B.buddhabrot_params(**kw), B.buddhabrot_guide_params(**guide))
    want, ws, winfo = GR.render_guided(R.params(**kw), dict(guide, complement_weight=0))
    assert np.array_equal(plane, want) and st.as_tuple() == R.stats_tuple(ws) and info.n_cells == winfo["n_cells"] > 0


# ---- the app ------------------------------------------------------------------------------------------------------------------------
def run_app(tmp_path, name, *args):
    out = tmp_path / name
    r = subprocess.run([APP, "--out", str(out), "--quiet"] + list(args), capture_output=True, text=True, cwd=tmp_path, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    from PIL import Image
    return np.asarray(Image.open(out).convert("RGBA")), r.stdout


def test_app_guided_end_to_end(ctx, B, tmp_path):
    W, H, N = 96, 64, 1 << 16
    opts = ["--buddhabrot", str(N), "--width", str(W), "--height", str(H), "--max-iter", "200", "--centre", "-0.75", "0.1", "--scale", "0.2", "0.133"]
    hand, hs, pst, lst, comp, cst = chain_by_hand(ctx, B, CHAIN, dict(GUIDE, complement_weight=4))
    L = R.white_level([hand], 99.9)
    m = B.buddhabrot_sqrt_map(L)
    want = ctx.convert_rgba8(B.buddhabrot_tonemap(hand, hand, hand, L, m, m, m), 255.0)
    img, text = run_app(tmp_path, "guided.png", *opts, "--guided=6", "--pilot", str(1 << 16), "--dilate", "1", "--unbiased", "4")
    assert np.array_equal(img, want) and len(np.unique(img[..., 0])) > 2   # (a picture, not a flat plane)
    assert f"samples {hs[0]}, skipped {hs[1]}, contributing {hs[2]}, points {hs[3]}, added {hs[4]}" in text, text
    line = (f"guided: {lst.size} of 4096 cells ({100.0 * lst.size / 4096:.2f} %), pilot added {pst[4]} of {1 << 16} samples, "
            f"complement {comp.size} cells: samples {cst[0]}, added {cst[4]} at weight 4")
    assert line in text, text
    # the defaults of --guided are the library's: g = 8, dilate 1 (the pilot is cut down to keep the test quick)
    img, text = run_app(tmp_path, "guided8.png", *opts, "--guided", "--pilot", str(1 << 14))
    plane, st, info = ctx.buddhabrot_guided(B.buddhabrot_params(**CHAIN), B.buddhabrot_guide_params(pilot_samples=1 << 14))
    L = R.white_level([plane], 99.9)
    m = B.buddhabrot_sqrt_map(L)
    assert np.array_equal(img, ctx.convert_rgba8(B.buddhabrot_tonemap(plane, plane, plane, L, m, m, m), 255.0))
    assert f"guided: {info.n_cells} of 65536 cells" in text and "complement" not in text
    # --nebula: one pilot per channel
    img, text = run_app(tmp_path, "nebula.png", *opts, "--nebula", "50", "100", "200", "--guided=6", "--pilot", str(1 << 14))
    assert text.count("guided: ") == 3 and text.count("buddhabrot: max_iter") == 3
    # without --guided: today's output for the same options
    plane, st = ctx.buddhabrot(B.buddhabrot_params(**CHAIN))
    L = R.white_level([plane], 99.9)
    m = B.buddhabrot_sqrt_map(L)
    img, text = run_app(tmp_path, "uniform.png", *opts)
    assert np.array_equal(img, ctx.convert_rgba8(B.buddhabrot_tonemap(plane, plane, plane, L, m, m, m), 255.0)) and "guided:" not in text
    assert f"samples {st.samples}, skipped {st.skipped}, contributing {st.contributing}, points {st.points}, added {st.added}" in text


def test_app_refuses_guided_options_out_of_place(tmp_path):
    for args, why in ((["--guided"], "only with --buddhabrot"), (["--pilot", "100"], "only with --buddhabrot"),
                      (["--buddhabrot", "100", "--dilate", "2"], "only with --guided"), (["--buddhabrot", "100", "--guided=13"], "--guided="),
                      (["--buddhabrot", "100", "--guided=0"], "G is 1 to 12"), (["--buddhabrot", "100", "--guided", "--dilate", "9"], "--dilate 9")):
        r = subprocess.run([APP, "--out", str(tmp_path / "no.png"), "--quiet", "--width", "16", "--height", "16"] + args, capture_output=True,
                           text=True, cwd=tmp_path, timeout=60)
        assert r.returncode != 0 and why in r.stdout, (args, r.stdout)
        assert not (tmp_path / "no.png").exists()
