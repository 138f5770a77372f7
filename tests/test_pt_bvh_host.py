"""The path tracer's sphere BVH without a GPU: mc_pathtrace_accel_intersect (the walk the kernels run, csrc/pt_bvh.h) must return what
the shader's linear loop returns - restated in numpy, tests/pt_bvh_ref.py - on EVERY ray: the same id, the same bits of t, no ray
left out.  The cull's proof (csrc/pt_bvh.h) covers every ray: a direction whose squared length is more than 0.01 off 1, or a NaN,
culls nothing, so the families below include rays of that kind too and none is excused."""
import numpy as np
import pytest

import pt_bvh_ref as R


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _room_with(spheres):
    return R.ROOM.copy(), np.asarray(spheres, np.float32).reshape(-1, 12)


def _scenes(B, O):
    P, S = B.default_scene()
    rng200 = np.random.default_rng(100 + 200)      # the generator test_gpu_scenes.py gives its (12, 200, 5) scene
    yield "reference", np.float32(P).reshape(-1, 12), np.float32(S).reshape(-1, 12), 25000
    yield "large-sphere-walls", np.float32(O.LARGE_SPHERE_PLANES).reshape(-1, 12), np.float32(O.LARGE_SPHERE_SPHERES).reshape(-1, 12), 25000
    yield ("random(12, 200, 5)",) + R.random_scene(rng200, 12, 200, 5) + (25000,)
    yield ("lattice 700",) + _room_with(R.lattice(700)) + (25000,)
    yield ("lattice 3500",) + _room_with(R.lattice(3500)) + (25000,)
    yield "0 spheres", R.ROOM.copy(), np.zeros((0, 12), np.float32), 25000
    yield ("1 sphere",) + _room_with(R.lattice(1)) + (25000,)
    yield "0 planes", np.zeros((0, 12), np.float32), R.random_scene(np.random.default_rng(5), 6, 60, 2)[1], 25000
    yield ("duplicates",) + R.duplicate_scene() + (25000,)
    yield ("concentric",) + R.concentric_scene() + (25000,)
    yield ("unboxable",) + R.unboxable_scene() + (25000,)


@pytest.fixture(scope="module")
def scenes(B, O):
    return {name: (planes, spheres, n) for name, planes, spheres, n in _scenes(B, O)}


SCENE_NAMES = ["reference", "large-sphere-walls", "random(12, 200, 5)", "lattice 700", "lattice 3500", "0 spheres", "1 sphere", "0 planes",
               "duplicates", "concentric", "unboxable"]


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_accel_intersect_equals_the_linear_loop_on_every_ray(B, scenes, name):
    """>= 1e5 rays per scene (camera, interior, from sphere surfaces, at silhouettes from 1, 1e3 and 1e5 away, NaN and off-unit rays):
    zero mismatches allowed."""
    planes, spheres, n_each = scenes[name]
    o, d = R.ray_families(planes, spheres, n_each, seed=len(name) * 7919 + spheres.shape[0])
    assert o.shape[0] >= 100000
    ref_id, ref_t = R.intersect(planes, spheres, o, d)
    with B.PathtraceAccel(planes, spheres) as a:
        got_id, got_t = a.intersect(o, d)
        info = a.info()
    bad = (got_id != ref_id) | (bits(got_t) != bits(ref_t))
    hits = int((ref_id >= 0).sum())
    print(f"{name}: {o.shape[0]} rays, {hits} hits, {int((ref_id >= planes.shape[0]).sum())} on spheres, {int(bad.sum())} mismatches; {info}")
    assert not bad.any(), (int(bad.sum()), o[bad][:3], d[bad][:3], got_id[bad][:3], ref_id[bad][:3], got_t[bad][:3], ref_t[bad][:3])
    assert info["boxed"] + info["unboxed"] == spheres.shape[0] and info["n_planes"] == planes.shape[0]
    if spheres.shape[0]:
        assert hits > 0


def test_the_lower_index_wins_a_tie(B):
    """Two identical spheres: every ray that hits one reports the lower index, with either order of the pair in the tree's leaves."""
    planes, spheres = R.duplicate_scene()
    o, d = R.surface_rays(spheres[1:2], 4000, np.random.default_rng(1))
    o2, d2 = R.camera_rays(4000, np.random.default_rng(2))
    o, d = np.concatenate([o, o2]), np.concatenate([d, d2])
    with B.PathtraceAccel(planes, spheres) as a:
        ids, _ = a.intersect(o, d)
    np_ = planes.shape[0]
    assert (ids == np_ + 1).any() and (ids == np_ + 3).any()
    assert not (ids == np_ + 2).any() and not (ids == np_ + 4).any()


def test_unboxable_spheres_are_kept_on_the_linear_list(B):
    planes, spheres = R.unboxable_scene()
    with B.PathtraceAccel(planes, spheres) as a:
        info = a.info()
    assert info["unboxed"] == 3 and info["boxed"] == spheres.shape[0] - 3      # NaN centre, infinite radius, overflowing box
    everything = spheres.copy()
    everything[:, 3] = np.inf
    with B.PathtraceAccel(planes, everything) as a:
        info = a.info()
        assert (info["nodes"], info["depth"], info["leaves"], info["boxed"]) == (0, 0, 0, 0) and info["unboxed"] == spheres.shape[0]


@pytest.mark.parametrize("n", [0, 1, 4, 5, 700, 3500])
def test_tree_shape(B, n):
    """Leaves of at most 4 spheres, every boxed sphere in exactly one leaf, depth bounded by the median split."""
    with B.PathtraceAccel(R.ROOM, R.lattice(n)) as a:
        info = a.info()
        raw = a.bytes()
    assert info["boxed"] == n and info["unboxed"] == 0 and info["bytes"] == raw.size == 32 * info["nodes"] + 20 * n
    if n == 0:
        assert info["nodes"] == 0
        return
    assert info["leaves"] >= (n + 3) // 4 and info["nodes"] == 2 * info["leaves"] - 1
    assert info["depth"] <= int(np.ceil(np.log2(max(n / 4.0, 1.0)))) + 1
    nodes = raw[:32 * info["nodes"]].view(np.int32).reshape(-1, 8)
    skip, leaf = nodes[:, 3], nodes[:, 7]
    assert (skip > np.arange(info["nodes"])).all() and skip.max() == info["nodes"] and skip[0] == info["nodes"]
    counts = leaf[leaf != 0] & 7
    assert counts.min() >= 1 and counts.max() <= 4 and counts.sum() == n
    index = raw[32 * info["nodes"] + 16 * n:32 * info["nodes"] + 20 * n].view(np.uint32)
    assert np.array_equal(np.sort(index), np.arange(n, dtype=np.uint32))
    # every leaf sphere inside its leaf's box, every box inside the root's
    lo, hi = raw[:32 * info["nodes"]].view(np.float32).reshape(-1, 8)[:, 0:3], raw[:32 * info["nodes"]].view(np.float32).reshape(-1, 8)[:, 4:7]
    assert (lo >= lo[0]).all() and (hi <= hi[0]).all()
    sph = raw[32 * info["nodes"]:32 * info["nodes"] + 16 * n].view(np.float32).reshape(-1, 4)
    for k in np.nonzero(leaf)[0][:50]:
        first, count = leaf[k] >> 3, leaf[k] & 7
        s = sph[first:first + count]
        assert (s[:, :3] - s[:, 3:4] > lo[k]).all() and (s[:, :3] + s[:, 3:4] < hi[k]).all()


def test_the_build_is_deterministic(B):
    """Two builds of one scene give the same bytes and the same info; so does a build from a copy of the tables at another address."""
    planes, spheres = R.random_scene(np.random.default_rng(12), 8, 1500, 3)
    spheres[100:140, 0:3] = spheres[200:240, 0:3]          # equal centres: the split's ties go by table index
    with B.PathtraceAccel(planes, spheres) as a, B.PathtraceAccel(planes.copy(), spheres.copy()) as b:
        assert a.info() == b.info()
        assert np.array_equal(a.bytes(), b.bytes())
        assert a.info()["device_copies"] == 0


def test_select_kernel_reports_the_bvh_and_the_tier(B):
    with B.PathtraceAccel(R.ROOM, R.lattice(700)) as a:
        for mode, tier in ((B.PT_MATH_STRICT, B.PT_MATH_STRICT), (B.PT_MATH_FAST, B.PT_MATH_FAST_CAREFUL),
                           (B.PT_MATH_FAST_CAREFUL, B.PT_MATH_FAST_CAREFUL)):
            k = a.select_kernel(B.pathtrace_params(900, 600, 500, math_mode=mode))
            assert (k.kernel, k.lanes_per_pixel, k.math_mode, k.launches) == (B.PT_KERNEL_BVH, 16, tier, 2)   # 500 = 31 x 16 + 4
        assert a.select_kernel(B.pathtrace_params(24, 16, 2)).lanes_per_pixel == 1
        k = a.select_kernel(B.pathtrace_params(24, 16, 6))
        assert (k.lanes_per_pixel, k.launches) == (4, 2)
    # the automatic choice of the plain calls is untouched: never the BVH
    k = B.pathtrace_select_kernel(B.pathtrace_params(900, 600, 500), R.ROOM, R.lattice(3500))
    assert k.kernel == B.PT_KERNEL_GENERIC_MEMORY


def _refused(B, status, fn, *args):
    with pytest.raises(B.McError) as e:
        fn(*args)
    assert e.value.status == status, e.value
    assert e.value.args and "mc_pathtrace" in str(e.value)      # the detail names the call
    return e.value


def test_refusals(B):
    import ctypes as C
    L = B.lib()
    INVALID, UNSUPPORTED = 1, 5
    planes, spheres = R.ROOM, R.lattice(5)
    # create: NULL out, a NULL table with a count, more than 2^20 objects
    assert L.mc_pathtrace_accel_create(None, 0, None, 0, None) == INVALID
    h = C.c_void_p()
    assert L.mc_pathtrace_accel_create(None, 3, None, 0, C.byref(h)) == INVALID and not h
    huge = np.zeros(((1 << 20) + 1, 12), np.float32)
    e = _refused(B, UNSUPPORTED, B.PathtraceAccel, planes[:0], huge)
    assert "2^20" in str(e)
    # exactly 2^20 objects is accepted (the depth bound of the issue: 19 levels)
    huge[:, 0] = np.arange(huge.shape[0], dtype=np.float32)
    huge[:, 3] = 0.25
    with B.PathtraceAccel(planes[:0], huge[:1 << 20]) as big:
        info = big.info()
        assert info["boxed"] == 1 << 20 and info["depth"] == 19 and info["leaves"] == 1 << 18
    with B.PathtraceAccel(planes, spheres) as a:
        # info / copy / intersect: NULL pointers, a short buffer
        assert L.mc_pathtrace_accel_info(a._h, None) == INVALID and L.mc_pathtrace_accel_info(None, None) == INVALID
        assert L.mc_pathtrace_accel_copy(a._h, None, 0) == INVALID
        buf = np.zeros(8, np.uint8)
        assert L.mc_pathtrace_accel_copy(a._h, buf.ctypes.data_as(C.c_void_p), 8) == INVALID
        ray = np.zeros(3, np.float32)
        assert L.mc_pathtrace_accel_intersect(a._h, 1, ray.ctypes.data_as(C.c_void_p), ray.ctypes.data_as(C.c_void_p), None, None) == INVALID
        assert L.mc_pathtrace_accel_intersect(None, 0, None, None, None, None) == INVALID
        # the request: flags, extended precision (named), empty ranges, a bad mode, a NULL object / params / out
        e = _refused(B, INVALID, a.select_kernel, B.pathtrace_params(8, 8, 1, flags=B.PT_SCENE_IN_MEMORY))
        assert "flags must be 0" in str(e)
        for prec, word in ((B.PT_PREC_FP64, "MC_PT_PREC_FP64"), (2, "MC_PT_PREC_DS"), (3, "MC_PT_PREC_DF64")):
            e = _refused(B, UNSUPPORTED, a.select_kernel, B.pathtrace_params(8, 8, 1, flags=B.pt_precision(prec)))
            assert word in str(e)
        _refused(B, INVALID, a.select_kernel, B.pathtrace_params(8, 8, 1, flags=B.pt_force_s(4)))
        _refused(B, INVALID, a.select_kernel, B.pathtrace_params(0, 8, 1))
        _refused(B, INVALID, a.select_kernel, B.pathtrace_params(8, 8, 4, sample_begin=2, sample_end=2))
        _refused(B, INVALID, a.select_kernel, B.pathtrace_params(8, 8, 1, row_begin=3, row_end=9))
        _refused(B, INVALID, a.select_kernel, B.pathtrace_params(8, 8, 1, math_mode=7))
        p = B.pathtrace_params(8, 8, 1)
        out = B.PathtraceKernelInfo()
        assert L.mc_pathtrace_accel_select_kernel(None, C.byref(p), C.byref(out)) == INVALID
        assert L.mc_pathtrace_accel_select_kernel(a._h, None, C.byref(out)) == INVALID
        assert L.mc_pathtrace_accel_select_kernel(a._h, C.byref(p), None) == INVALID
        # the render calls without a context
        img = np.zeros((8, 8, 4), np.float32)
        assert L.mc_pathtrace_render_accel(None, a._h, C.byref(p), img.ctypes.data_as(C.c_void_p)) == INVALID
        assert L.mc_pathtrace_render_accel_rgba8(None, a._h, C.byref(p), img.ctypes.data_as(C.c_void_p)) == INVALID
        assert L.mc_pathtrace_render_accel_device_async(None, a._h, C.byref(p), None, None) == INVALID
        stale = C.c_void_p(a._h.value)
    # a destroyed object is refused by name, not dereferenced; destroy(NULL) is fine
    assert L.mc_pathtrace_accel_info(stale, C.byref(B.PathtraceAccelStats())) == INVALID
    assert b"not a live" in L.mc_last_error_detail()
    assert L.mc_pathtrace_accel_destroy(stale) == INVALID
    assert L.mc_pathtrace_accel_destroy(None) == 0
