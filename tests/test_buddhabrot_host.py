"""The Buddhabrot's host calls (no GPU): mc_buddhabrot_density against the numpy restatement of include/mc_compute.h
(tests/buddhabrot_ref.py), plane and statistics EQUAL, on the header's cross-check cases and on every edge the contract names; every
validation refusal with its detail text; the sqrt map and the tone map against numpy; the ctypes mirror's layout."""
import ctypes as C

import numpy as np
import pytest

import buddhabrot_ref as R

INVALID = 1
VIEW = (-0.5, 0.0, 3.0, 2.0)
# (keywords of params(), what the header's table says: contributing, points, added, largest bin)
CASES = {
    "M64": (dict(width=48, height=32, samples=1 << 14, max_iter=64, view=VIEW), (14785, 28561, 17509, 32)),
    "M200-min20": (dict(width=48, height=32, samples=1 << 16, max_iter=200, min_iter=20, view=VIEW), (816, 40097, 38739, 134)),
    "1x1": (dict(width=1, height=1, samples=1000, max_iter=64, seed=3, view=(0.0, 0.0, 8.0, 8.0)), (None, None, None, 1850)),
}


def both(B, kw, plane=None):
    """(library plane, library stats tuple, restated plane, restated stats tuple) of one request, each from its own copy of `plane`."""
    got, gs = B.buddhabrot_density(B.buddhabrot_params(**kw), None if plane is None else plane.copy())
    want, ws = R.density(R.params(**kw), None if plane is None else plane.copy())
    return got, gs.as_tuple(), want, R.stats_tuple(ws)


def check(B, kw, plane=None):
    got, gs, want, ws = both(B, kw, plane)
    assert gs == ws, (kw, gs, ws)
    assert got.dtype == np.uint32 and np.array_equal(got, want), (kw, int((got != want).sum()))
    return got, gs


@pytest.mark.parametrize("name", list(CASES))
def test_cross_check_cases(B, name):
    kw, (contributing, points, added, largest) = CASES[name]
    plane, st = check(B, kw)
    assert int(plane.max()) == largest
    if contributing is not None:
        assert st[2:] == (contributing, points, added)
    assert st[0] == kw["samples"] and int(plane.sum(dtype=np.uint64)) == st[4]


def test_ranges_compose(B):
    kw = dict(CASES["M64"][0])
    N = kw.pop("samples")
    whole, ws = check(B, dict(kw, samples=N))
    plane, st = B.buddhabrot_density(B.buddhabrot_params(samples=N // 3, **kw))
    plane, st = B.buddhabrot_density(B.buddhabrot_params(samples=N - N // 3, sample_begin=N // 3, **kw), plane, st)
    assert np.array_equal(plane, whole) and st.as_tuple() == ws


def test_k_crossing_2_pow_32(B):
    kw = dict(width=48, height=32, samples=65, sample_begin=(5 << 32) - 17, max_iter=64, view=VIEW)
    plane, st = check(B, kw)
    assert st[0] == 65 and st[4] > 0
    low = R.density(R.params(**dict(kw, sample_begin=(1 << 32) - 17)))[0]
    assert not np.array_equal(plane, low)   # the high word of k reaches the hash


def test_negative_view_scale_mirrors(B):
    kw = dict(width=48, height=32, samples=1 << 12, max_iter=64)
    mirrored, _ = check(B, dict(kw, view=(-0.5, 0.0, -3.0, 2.0)))
    assert mirrored.sum() > 0
    check(B, dict(kw, view=(-0.5, 0.0, 3.0, -2.0)))
    check(B, dict(kw, sample_window=(-0.5, 0.0, -4.0, 4.0)))


def test_min_iter_edges(B):
    M = 64
    kw = dict(width=48, height=32, samples=1 << 14, max_iter=M, view=VIEW)
    _, st = check(B, dict(kw, min_iter=M - 1))        # only n = M - 1 contributes
    assert st[3] == st[2] * (M - 1)
    for m in (M, M + 1, 2 ** 32 - 1):                  # valid, adds nothing: the plane is untouched
        pre = np.arange(48 * 32, dtype=np.uint32).reshape(32, 48)
        plane, st = check(B, dict(kw, min_iter=m), pre)
        assert np.array_equal(plane, pre) and st[2:] == (0, 0, 0)


def test_max_iter_1_plots_nothing(B):
    plane, st = check(B, dict(width=48, height=32, samples=1 << 12, max_iter=1, view=VIEW))
    assert not plane.any() and st[2] > 0 and st[3] == 0 and st[4] == 0   # n = 0: contributing, no points


def test_window_inside_the_cardioid_skips_everything(B):
    plane, st = check(B, dict(width=48, height=32, samples=1 << 12, max_iter=64, view=VIEW, sample_window=(-0.1, 0.0, 0.2, 0.2)))
    assert st == (1 << 12, 1 << 12, 0, 0, 0) and not plane.any()


def test_window_far_outside_escapes_at_once(B):
    plane, st = check(B, dict(width=48, height=32, samples=1 << 12, max_iter=64, view=VIEW, sample_window=(3.0, 3.0, 0.5, 0.5)))
    assert st == (1 << 12, 0, 1 << 12, 0, 0) and not plane.any()


def test_adds_to_a_prefilled_plane_inside_guard_words(B):
    kw = dict(width=7, height=5, samples=1 << 12, max_iter=64, view=VIEW)
    rng = np.random.default_rng(1)
    buf = rng.integers(0, 2 ** 32, 7 * 5 + 32, dtype=np.uint32)
    before = buf.copy()
    inner = buf[16:16 + 35].reshape(5, 7)
    fresh, _ = check(B, kw)
    B.buddhabrot_density(B.buddhabrot_params(**kw), inner)
    assert np.array_equal(inner, before[16:16 + 35].reshape(5, 7) + fresh)             # (uint32 sums wrap, as the plane does)
    assert np.array_equal(buf[:16], before[:16]) and np.array_equal(buf[-16:], before[-16:])
    check(B, kw, before[16:16 + 35].reshape(5, 7).copy())


def test_counts_wrap(B):
    kw = CASES["1x1"][0]
    pre = np.full((1, 1), 2 ** 32 - 1, np.uint32)
    plane, _ = check(B, kw, pre)
    assert int(plane[0, 0]) == 1850 - 1


def test_stats_may_be_null_and_are_added_to(B):
    kw = CASES["M64"][0]
    p = B.buddhabrot_params(**kw)
    plane = np.zeros((32, 48), np.uint32)
    assert B.lib().mc_buddhabrot_density(C.byref(p), plane.ctypes.data_as(C.c_void_p), None) == 0
    assert np.array_equal(plane, R.density(R.params(**kw))[0])
    st = B.BuddhabrotStats(1, 2, 3, 4, 5)
    B.buddhabrot_density(p, None, st)
    want = R.stats_tuple(R.density(R.params(**kw))[1])
    assert st.as_tuple() == tuple(a + b for a, b in zip(want, (1, 2, 3, 4, 5)))


def test_default_params(B):
    p = B.BuddhabrotParams()
    assert B.lib().mc_buddhabrot_default_params(96, 64, 12345, C.byref(p)) == 0
    assert (p.view_centre_x, p.view_centre_y, p.view_scale_x, p.view_scale_y) == (-0.5, 0.0, 3.0, 2.0)
    assert (p.sample_centre_x, p.sample_centre_y, p.sample_scale_x, p.sample_scale_y) == (-0.5, 0.0, 4.0, 4.0)
    assert (p.sample_begin, p.sample_end, p.width, p.height, p.max_iter, p.min_iter, p.seed, p.flags) == (0, 12345, 96, 64, 1000, 0, 1, 0)
    assert B.lib().mc_buddhabrot_default_params(96, 64, 1, None) == INVALID


# ---- validation ---------------------------------------------------------------------------------------------------------------------
REFUSALS = [
    (dict(width=0), "width is 0"), (dict(height=0), "height is 0"),
    (dict(width=65536, height=65536), "width * height exceeds 2^32 - 1"),
    (dict(max_iter=0), "max_iter is 0"), (dict(max_iter=(1 << 24) + 1), "max_iter exceeds 2^24"),
    (dict(view_scale_x=0.0), "view_scale_x is zero"), (dict(view_scale_y=float("inf")), "view_scale_y is not finite"),
    (dict(sample_scale_x=float("nan")), "sample_scale_x is not finite"), (dict(sample_scale_y=-0.0), "sample_scale_y is zero"),
    (dict(view_centre_x=float("nan")), "view_centre_x is not finite"), (dict(view_centre_y=float("-inf")), "view_centre_y is not finite"),
    (dict(sample_centre_x=float("inf")), "sample_centre_x is not finite"), (dict(sample_centre_y=float("nan")), "sample_centre_y is not finite"),
    (dict(sample_begin=10, sample_end=9), "sample_end is below sample_begin"),
    (dict(sample_begin=1, sample_end=(1 << 40) + 2), "exceeds 2^40 samples"),
    (dict(flags=4), "flags has unknown bits"), (dict(flags=1 << 31), "flags has unknown bits"), (dict(flags=3), "names both"),
]


@pytest.mark.parametrize("change,detail", REFUSALS, ids=[d for _, d in REFUSALS])
def test_refusals(B, change, detail):
    p = B.buddhabrot_params(48, 32, 100, max_iter=64)
    for k, v in change.items():
        setattr(p, k, v)
    plane = np.zeros((2, 2), np.uint32)   # never touched: the refusal comes first
    with pytest.raises(B.McError) as e:
        B.lib().mc_buddhabrot_density.restype = C.c_int
        B._check(B.lib().mc_buddhabrot_density(C.byref(p), plane.ctypes.data_as(C.c_void_p), None), "mc_buddhabrot_density")
    assert e.value.status == INVALID and detail in str(e.value) and "mc_buddhabrot_density" in str(e.value), e.value
    assert not plane.any()


def test_refusals_null_pointers_and_accepted_edges(B):
    L = B.lib()
    p = B.buddhabrot_params(4, 4, 10, max_iter=8)
    plane = np.zeros((4, 4), np.uint32)
    assert L.mc_buddhabrot_density(None, plane.ctypes.data_as(C.c_void_p), None) == INVALID
    assert b"p is NULL" in L.mc_last_error_detail()
    assert L.mc_buddhabrot_density(C.byref(p), None, None) == INVALID
    assert b"plane is NULL" in L.mc_last_error_detail()
    for ok in (dict(max_iter=1 << 24, sample_end=0), dict(sample_begin=7, sample_end=7), dict(flags=1), dict(flags=2),
               dict(view_scale_x=-3.0), dict(width=65535, height=65537, sample_end=0)):   # (2^32 - 1 bins; no sample: nothing is written)
        q = B.buddhabrot_params(4, 4, 10, max_iter=8)
        for k, v in ok.items():
            setattr(q, k, v)
        big = np.zeros(1, np.uint32) if q.width > 4 else plane
        assert L.mc_buddhabrot_density(C.byref(q), big.ctypes.data_as(C.c_void_p), None) == 0, ok


# ---- the maps and the tone map ------------------------------------------------------------------------------------------------------
LEVELS = [1, 2, 255, 1 << 20]


@pytest.mark.parametrize("L", LEVELS)
def test_sqrt_map(B, L):
    m = B.buddhabrot_sqrt_map(L)
    assert np.array_equal(m, R.sqrt_map(L))
    assert m[0] == 0 and m[L] == L and (np.diff(m.astype(np.int64)) >= 0).all()


@pytest.mark.parametrize("L", LEVELS)
def test_tonemap(B, L):
    rng = np.random.default_rng(L)
    H, W = 13, 19
    planes = [rng.integers(0, 2 * L + 2, (H, W)).astype(np.uint32) for _ in range(3)]
    planes[0][0, :4] = (0, L, L + 1, 2 ** 32 - 1)                       # densities at, above and far above L
    maps = [B.buddhabrot_sqrt_map(L), rng.integers(0, L + 1, L + 1).astype(np.uint32), np.arange(L + 1, dtype=np.uint32)]
    got = B.buddhabrot_tonemap(*planes, L, *maps)
    want = R.tonemap(*planes, L, *maps)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got[..., 3] == 1.0).all() and got[..., :3].min() >= 0.0 and got[..., :3].max() <= 1.0
    grey = B.buddhabrot_tonemap(planes[0], planes[0], planes[0], L, maps[0], maps[0], maps[0])   # aliased planes and maps
    assert np.array_equal(grey.view(np.uint32), R.tonemap(planes[0], planes[0], planes[0], L, maps[0], maps[0], maps[0]).view(np.uint32))
    assert np.array_equal(grey[..., 0], grey[..., 1]) and np.array_equal(grey[..., 0], grey[..., 2])


def test_map_refusals(B):
    L = B.lib()
    out = np.zeros(8, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for levels in (0, (1 << 20) + 1):
        assert L.mc_buddhabrot_sqrt_map(levels, vp(out)) == INVALID and b"levels is outside 1 .. 2^20" in L.mc_last_error_detail()
    assert L.mc_buddhabrot_sqrt_map(4, None) == INVALID and b"map is NULL" in L.mc_last_error_detail()
    d = np.zeros((2, 2), np.uint32)
    m = np.arange(5, dtype=np.uint32)
    rgba = np.zeros((2, 2, 4), np.float32)
    assert L.mc_buddhabrot_tonemap(2, 2, vp(d), vp(d), vp(d), 4, vp(m), vp(m), vp(m), vp(rgba)) == 0
    assert L.mc_buddhabrot_tonemap(2, 2, vp(d), None, vp(d), 4, vp(m), vp(m), vp(m), vp(rgba)) == INVALID
    assert b"a pointer is NULL" in L.mc_last_error_detail()
    assert L.mc_buddhabrot_tonemap(0, 2, vp(d), vp(d), vp(d), 4, vp(m), vp(m), vp(m), vp(rgba)) == INVALID
    assert L.mc_buddhabrot_tonemap(2, 2, vp(d), vp(d), vp(d), 0, vp(m), vp(m), vp(m), vp(rgba)) == INVALID
    bad = m.copy()
    bad[2] = 5
    assert L.mc_buddhabrot_tonemap(2, 2, vp(d), vp(d), vp(d), 4, vp(m), vp(m), vp(bad), vp(rgba)) == INVALID
    assert b"a map entry exceeds levels" in L.mc_last_error_detail()


def test_white_level_policy_restated():
    """The app's white level (tests/buddhabrot_ref.py white_level; the GPU suite holds the app to it): hand-made planes."""
    d = np.array([0, 0, 1, 1, 1, 2, 5, 9, 9, 100], np.uint32)      # 8 non-empty bins
    assert R.white_level([d], 100.0) == 100 and R.white_level([d], 87.5) == 9 and R.white_level([d], 50.0) == 2
    assert R.white_level([d], 37.5) == 1 and R.white_level([np.zeros(4, np.uint32)], 99.9) == 1
    assert R.white_level([np.array([2 ** 32 - 1], np.uint32)], 99.9) == (1 << 20) - 1


# ---- the ctypes mirror --------------------------------------------------------------------------------------------------------------
def test_struct_layout(B):
    P, S = B.BuddhabrotParams, B.BuddhabrotStats
    assert C.sizeof(P) == 104 and C.sizeof(S) == 40
    names = [f for f, _ in P._fields_]
    assert names == ["view_centre_x", "view_centre_y", "view_scale_x", "view_scale_y", "sample_centre_x", "sample_centre_y",
                     "sample_scale_x", "sample_scale_y", "sample_begin", "sample_end", "width", "height", "max_iter", "min_iter", "seed",
                     "flags"]
    assert [getattr(P, f).offset for f in names] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 84, 88, 92, 96, 100]
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 8, 16, 24, 32]
    assert (B.BUDDHA_KERNEL_PLAIN, B.BUDDHA_KERNEL_POOLED) == (1, 2)
