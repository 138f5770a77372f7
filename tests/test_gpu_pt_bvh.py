"""The path tracer through a sphere BVH on the MI355X (mc_pathtrace_render_accel*, csrc/pt_bvh_kernel.h).  Strict math: bit-identical
to the CPU oracle - the contract of the linear kernels, carried over unchanged - at the smallest shapes at which the kernel can go wrong:
every sample-parallel width, a width and a sample count that fit no tile, thousands of spheres, ties, unboxable spheres, empty tables;
sample ranges, row bands and interleaved row blocks that compose with one another and with the linear kernel's parts.  Careful tier: the
bound tests/test_gpu_scenes.py applies to careful-tier many-sphere scenes at 24 x 16 x 6, against the oracle."""
import json
import os
import subprocess

import numpy as np
import pytest

import pt_bvh_ref as R

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _scene(name):
    if name == "random200":
        return R.random_scene(np.random.default_rng(100 + 200), 12, 200, 5)      # test_gpu_scenes.py's (12, 200, 5)
    if name == "random700":
        return R.random_scene(np.random.default_rng(700), 12, 700, 4)            # test_gpu_scenes.py's (12, 700, 4)
    if name == "random4000":
        return R.random_scene(np.random.default_rng(9), 6, 4000, 3)
    if name == "lattice700":
        return R.ROOM.copy(), R.lattice(700)
    if name == "duplicates":
        return R.duplicate_scene()
    if name == "unboxable":
        return R.unboxable_scene()
    if name == "one":
        return R.ROOM.copy(), R.lattice(1)
    if name == "none":
        return R.ROOM.copy(), np.zeros((0, 12), np.float32)
    raise KeyError(name)


@pytest.fixture(scope="module")
def world(B, O):
    """Scenes, their accel objects and the oracle's renders, each made once and shared (never modified)."""
    class World:
        def __init__(self):
            self.scenes, self.accels, self.refs = {}, {}, {}

        def scene(self, name):
            if name not in self.scenes:
                self.scenes[name] = _scene(name)
            return self.scenes[name]

        def accel(self, name):
            if name not in self.accels:
                self.accels[name] = B.PathtraceAccel(*self.scene(name))
            return self.accels[name]

        def ref(self, name, W, H, spp, mode=None, max_depth=12):
            mode = O.MATH_MC if mode is None else mode
            key = (name, W, H, spp, mode, max_depth)
            if key not in self.refs:
                planes, spheres = self.scene(name)
                self.refs[key] = O.pathtrace(W, H, spp, planes=planes, spheres=spheres, math_mode=mode, max_depth=max_depth)
            return self.refs[key]

    w = World()
    yield w
    for a in w.accels.values():
        a.close()


@pytest.mark.parametrize("name,W,H,spp", [("random200", 24, 16, 6), ("lattice700", 24, 16, 6), ("duplicates", 24, 16, 6),
                                          ("unboxable", 24, 16, 6), ("random200", 37, 23, 5), ("random4000", 8, 6, 2),
                                          ("one", 24, 16, 6), ("none", 24, 16, 6)])
def test_strict_is_bit_identical_to_the_oracle(ctx, B, world, name, W, H, spp):
    p = B.pathtrace_params(W, H, spp)
    out = ctx.pathtrace_accel(world.accel(name), p)
    ref = world.ref(name, W, H, spp)
    assert np.array_equal(bits(out), bits(ref)), (name, int((bits(out) != bits(ref)).sum()))
    assert np.isfinite(ref).all()
    if name not in ("none",):
        assert ref[..., :3].max() > 1.0


@pytest.mark.parametrize("spp,S,launches", [(2, 1, 1), (4, 4, 1), (6, 4, 2), (16, 16, 1), (21, 16, 2)])
def test_every_width_the_kernel_is_built_for(ctx, B, world, spp, S, launches):
    """S = 1, 4 and 16 lanes per pixel, alone and as the narrower second launch of a ragged sample count (6 = 4 + 2 x 1, 21 = 16 + 4 + 1)."""
    W, H = 12, 8
    p = B.pathtrace_params(W, H, spp)
    k = world.accel("random200").select_kernel(p)
    assert (k.kernel, k.lanes_per_pixel, k.math_mode, k.launches) == (B.PT_KERNEL_BVH, S, B.PT_MATH_STRICT, launches)
    assert np.array_equal(bits(ctx.pathtrace_accel(world.accel("random200"), p)), bits(world.ref("random200", W, H, spp)))


@pytest.mark.parametrize("max_depth", [0, 1, 15])
def test_depth_limits(ctx, B, world, max_depth):
    W, H, spp = 16, 12, 4
    p = B.pathtrace_params(W, H, spp, max_depth=max_depth)
    out = ctx.pathtrace_accel(world.accel("random200"), p)
    assert np.array_equal(bits(out), bits(world.ref("random200", W, H, spp, max_depth=max_depth)))


def test_sample_ranges_compose_with_each_other_and_with_the_linear_kernel(ctx, B, world):
    W, H, spp = 24, 16, 6
    planes, spheres = world.scene("random200")
    a = world.accel("random200")
    whole = world.ref("random200", W, H, spp)
    head, tail = B.pathtrace_params(W, H, spp, sample_end=3), B.pathtrace_params(W, H, spp, sample_begin=3)
    acc = ctx.pathtrace_accel(a, head)
    assert np.array_equal(bits(ctx.pathtrace_accel(a, tail, acc=acc)), bits(whole))
    # a range continued by the accel call on an accumulator the linear call wrote, and the reverse
    lin = ctx.pathtrace(head, planes=planes, spheres=spheres)
    assert np.array_equal(bits(lin), bits(acc))
    assert np.array_equal(bits(ctx.pathtrace_accel(a, tail, acc=lin)), bits(whole))
    assert np.array_equal(bits(ctx.pathtrace(tail, planes=planes, spheres=spheres, acc=acc)), bits(whole))


def test_row_bands_and_interleaved_blocks_equal_the_whole_image(ctx, B, world):
    W, H, spp = 24, 16, 6
    a = world.accel("random200")
    whole = world.ref("random200", W, H, spp)
    for r0, r1 in ((0, 5), (5, 6), (6, 16)):                        # bands that split wave tiles
        band = ctx.pathtrace_accel(a, B.pathtrace_params(W, H, spp, row_begin=r0, row_end=r1))
        assert np.array_equal(bits(band), bits(whole[r0:r1])), (r0, r1)
    block, n = 3, 2                                                 # interleaved blocks of 3 rows over 2 owners: 16 = 2 x 6 + 3 + 1
    for rank in range(n):
        p = B.pathtrace_params(W, H, spp, row_begin=rank * block, row_end=H, row_block=block, row_stride=n * block)
        tile = ctx.pathtrace_accel(a, p)
        rows = [r for r in range(H) if (r // block) % n == rank]
        assert tile.shape[0] == len(rows) == B.tile_rows(p)
        assert np.array_equal(bits(tile), bits(whole[rows])), rank


def test_device_form_writes_between_untouched_guard_rows(ctx, B, world):
    import torch
    W, H, spp = 37, 23, 5
    guard = 12345.5
    t = torch.full((H + 2, W, 4), guard, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.pathtrace_accel_device(world.accel("random200"), B.pathtrace_params(W, H, spp), t[1:].data_ptr())
    ctx.synchronize()
    got = t.cpu().numpy()
    assert (got[0] == guard).all() and (got[-1] == guard).all()
    assert np.array_equal(bits(got[1:-1]), bits(world.ref("random200", W, H, spp)))
    # a band into a buffer of exactly its size
    t2 = torch.full((4 + 2, W, 4), guard, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.pathtrace_accel_device(world.accel("random200"), B.pathtrace_params(W, H, spp, row_begin=7, row_end=11), t2[1:].data_ptr())
    ctx.synchronize()
    got = t2.cpu().numpy()
    assert (got[0] == guard).all() and (got[-1] == guard).all()
    assert np.array_equal(bits(got[1:-1]), bits(world.ref("random200", W, H, spp)[7:11]))


def test_rgba8_form_equals_the_conversion_of_the_float_form(ctx, B, world):
    W, H, spp = 37, 23, 5
    a = world.accel("random200")
    p = B.pathtrace_params(W, H, spp)
    u8 = ctx.pathtrace_accel_rgba8(a, p)
    assert np.array_equal(u8, ctx.convert_rgba8(ctx.pathtrace_accel(a, p), 1.0, rotate180=True))
    with pytest.raises(B.McError) as e:
        ctx.pathtrace_accel_rgba8(a, B.pathtrace_params(W, H, spp, row_end=8))
    assert e.value.status == 1


def test_two_objects_used_alternately_and_the_copies_they_hold(ctx, B, world):
    W, H, spp = 24, 16, 6
    p = B.pathtrace_params(W, H, spp)
    with B.PathtraceAccel(*world.scene("lattice700")) as x, B.PathtraceAccel(*world.scene("duplicates")) as y:
        assert x.info()["device_copies"] == 0
        for a, name in ((x, "lattice700"), (y, "duplicates"), (x, "lattice700"), (y, "duplicates")):
            assert np.array_equal(bits(ctx.pathtrace_accel(a, p)), bits(world.ref(name, W, H, spp))), name
        assert x.info()["device_copies"] == 1 and y.info()["device_copies"] == 1       # made once per (object, context)
        # a second context gets its own copy; destroying that context takes its copy with it, and the object goes on working
        with B.Context(0) as other:
            assert np.array_equal(bits(other.pathtrace_accel(x, p)), bits(world.ref("lattice700", W, H, spp)))
            assert x.info()["device_copies"] == 2
        assert x.info()["device_copies"] == 1
        assert np.array_equal(bits(ctx.pathtrace_accel(x, p)), bits(world.ref("lattice700", W, H, spp)))
    # refusals that need a context: a NULL output, flags, an extended precision
    import ctypes as C
    a = world.accel("random200")
    assert B.lib().mc_pathtrace_render_accel(ctx._h, a._h, C.byref(p), None) == 1
    assert B.lib().mc_pathtrace_render_accel_device_async(ctx._h, a._h, C.byref(p), None, None) == 1
    with pytest.raises(B.McError) as e:
        ctx.pathtrace_accel(a, B.pathtrace_params(W, H, spp, flags=B.PT_SCENE_IN_MEMORY))
    assert e.value.status == 1
    with pytest.raises(B.McError) as e:
        ctx.pathtrace_accel(a, B.pathtrace_params(W, H, spp, flags=B.pt_precision(B.PT_PREC_DS)))
    assert e.value.status == 5 and "MC_PT_PREC_DS" in str(e.value)


@pytest.mark.parametrize("name", ["random700", "random200"])
def test_careful_tier_against_the_oracle(ctx, B, O, world, name):
    """MC_PT_MATH_FAST and MC_PT_MATH_FAST_CAREFUL both run the careful tier.  Against the oracle evaluated with libm (the reference of
    every fast-math test here): finite, and inside the bound test_gpu_scenes.py applies to careful-tier renders of many-sphere scenes at
    this size and sample count (test_generic_scene_read_from_memory_is_bit_identical: at most 3 % of the values more than 1.0 apart,
    median difference at most 1e-3).  Reported, not asserted: whether it is bit-equal to the linear kernel's careful output."""
    W, H, spp = 24, 16, 6
    planes, spheres = world.scene(name)
    a = world.accel(name)
    outs = {}
    for mode in (B.PT_MATH_FAST, B.PT_MATH_FAST_CAREFUL):
        p = B.pathtrace_params(W, H, spp, math_mode=mode)
        k = a.select_kernel(p)
        assert (k.kernel, k.math_mode) == (B.PT_KERNEL_BVH, B.PT_MATH_FAST_CAREFUL)
        outs[mode] = ctx.pathtrace_accel(a, p)
    assert np.array_equal(bits(outs[B.PT_MATH_FAST]), bits(outs[B.PT_MATH_FAST_CAREFUL]))
    out = outs[B.PT_MATH_FAST_CAREFUL]
    # (the measurement switch keeps the linear call in the careful tier: as a caller makes it, a scene whose light touches a diffuse
    # sphere - these random rooms - is rendered strict, MC_PT_SCENE_LIGHT_ENCLOSED)
    q = B.pathtrace_params(W, H, spp, math_mode=B.PT_MATH_FAST_CAREFUL, flags=B.PT_NO_FAST_GUARD)
    assert B.pathtrace_select_kernel(q, planes, spheres).math_mode == B.PT_MATH_FAST_CAREFUL
    linear = ctx.pathtrace(q, planes=planes, spheres=spheres)
    same = np.array_equal(bits(out), bits(linear))
    print(f"{name}: BVH careful output bit-equal to the linear kernel's careful output: {same}"
          f" ({int((bits(out) != bits(linear)).sum())} of {out.size} words differ)")
    for label, mode in (("libm", O.MATH_LIBM), ("mc", O.MATH_MC)):
        d = np.abs(out[..., :3].astype(np.float64) - world.ref(name, W, H, spp, mode=mode)[..., :3].astype(np.float64))
        print(f"{name}: careful BVH against oracle({label}): share above 1.0 = {(d > 1.0).mean():.4f}, median = {np.median(d):.3e}, max = {d.max():.3f}")
    d = np.abs(out[..., :3].astype(np.float64) - world.ref(name, W, H, spp, mode=O.MATH_LIBM)[..., :3].astype(np.float64))
    assert np.isfinite(out).all() and (d > 1.0).mean() <= 0.03 and np.median(d) <= 1e-3, ((d > 1.0).mean(), np.median(d))


def test_app_scene_file_and_accel(ctx, B, world, tmp_path):
    """--scene FILE --accel bvh writes the PNG bytes of --accel linear (strict), on both save routes; bad values end the run early."""
    app = os.path.join(os.path.dirname(os.path.dirname(B.LIB_PATH)), "bin", "pathtracer")
    planes, spheres = world.scene("random200")
    with open(tmp_path / "room.scene", "w") as f:
        f.write("# 12 planes, 200 spheres\n\n")
        for kind, table in (("plane", planes), ("sphere", spheres)):
            for rec in table:
                f.write(kind + " " + " ".join(repr(float(v)) for v in rec) + "\n")
    spp, H = 6, 16

    def run(*extra):
        r = subprocess.run([app, str(spp), str(H), "--out", "o.png", "--quiet", "--timing-json", "--full-teardown", "--scene", "room.scene"] +
                           list(extra), capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 0, r.stdout + r.stderr
        j = json.loads([l for l in r.stdout.splitlines() if l.startswith('{"timing_ms"')][0])
        return (tmp_path / "o.png").read_bytes(), j

    linear, j = run()
    assert j["accel"] == "linear"
    explicit, j = run("--accel", "linear")
    assert j["accel"] == "linear" and explicit == linear
    for route in ([], ["--gpu-postprocess"]):
        data, j = run("--accel", "bvh", *route)
        assert j["accel"] == "bvh" and data == linear, route
    # the file holds the scene the library renders: the picture is the oracle's
    from PIL import Image
    img = np.asarray(Image.open(tmp_path / "o.png").convert("RGBA"))
    ref = world.ref("random200", 24, 16, spp)
    want = ctx.convert_rgba8(ref, 1.0, rotate180=True)
    assert np.array_equal(img, want)
    (tmp_path / "bad.scene").write_text("plane 1 0 0 2\n")
    for bad, word in ((["--accel", "tree"], "--accel"), (["--scene", "bad.scene"], "--scene"), (["--scene", "absent.scene"], "--scene"),
                      (["--accel", "bvh", "--gpus", "2"], "--accel"), (["--accel", "bvh", "--denoise"], "--accel")):
        r = subprocess.run([app, str(spp), str(H), "--quiet"] + bad, capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode != 0 and word in r.stdout and "now running app" not in r.stdout, (bad, r.stdout)
