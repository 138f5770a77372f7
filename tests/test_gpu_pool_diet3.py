"""The third VALU diet of the sample-pool kernels (csrc/pathtrace_pool.h): the depth-over-5 lane mask is carried over the loop edge
instead of being compared again, the light's cosine is dot(l, n) with its sign flipped (the vector nl is formed only for a bounce off a
diffuse sphere), the three -w_neg of the slab intersection stay in vector registers, the roulette compares the unscaled draw with
p * 2^32 from the staged record, the "emits" flag of a record has a word of its own, and `id >= 0` of the stash entries taken is asked
only while a wave can take an empty one.  No image may change a bit, in any math tier (the strict tier takes none of them: its
build must equal the parent's all the same).  The forms before stay compilable for exactly this comparison
(-DMC_PT_POOL_DIET3_PARENT through `make exp`, one library per tier's translation unit: the parent commit's listing): the shipped
library and those three render every case below in a child process each, and the storage buffers must be equal bit for bit, every pixel.  A render that trips the loop bound sets the status word and
fails its blocking call: every call must return MC_OK."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (W, H, spp, max_depth).  38 x 22 x 20: a ragged last batch (16 + 4) and pixels outside the 4 x 4 block tiles in both directions (a wave
# with a pixel outside the image asks `id >= 0` of every entry, a wave inside only of the last batch's).  16 x 8 x 48 at the default depth
# limit: three full batches (no entry is ever empty), lanes past depth 5, roulette ends on the light, paths cut at the depth limit —
# test_small_case_reaches_the_changed_code asserts these of the oracle's bounce counts.
SHAPES = {"38x22x20": (38, 22, 20, 12), "16x8x48": (16, 8, 48, 12)}
# the sample range 16 .. 20 of 38x22x20 continued from the range before it, and the two interleaved tiles of the whole image
RANGES = ("38x22_samples_0_16", "38x22_samples_16_20")
TILES = ("38x22_rows_0_8_of_16", "38x22_rows_8_8_of_16")
ROW_BLOCK, ROW_STRIDE = 8, 16
# 48 x 32 x 32 each: the light as sphere 0 (the unrolled light loop's first block), two lights, none (the host's round-synchronous kernels), a
# diffuse sphere (the general basis: the vector nl), two spheres, five (a fast request would go to the careful tier: rendered by every
# tier here), overlapping spheres (Disjoint = false: the shadow rays' root form)
SCENES = ("default", "light_first", "two_lights", "no_light", "diffuse_sphere", "two_spheres", "five_spheres", "overlapping_spheres")
SCENE_SHAPE = (48, 32, 32)
CASES = list(SHAPES) + list(RANGES) + list(TILES) + list(SCENES)
TIERS = {"fast": ("PT_MATH_FAST", "pathtrace_fast"), "careful": ("PT_MATH_FAST_CAREFUL", "pathtrace_careful"),
         "strict": ("PT_MATH_STRICT", "pathtrace_strict")}


def scene(O, name):
    planes, spheres = O.DEFAULT_PLANES.copy().reshape(6, 12), O.DEFAULT_SPHERES.copy().reshape(3, 12)
    if name == "light_first":
        spheres = spheres[[2, 1, 0]].copy()
    elif name == "two_lights":
        spheres[1, 4:7] = np.float32([40.0, 30.0, 20.0]); spheres[1, 8:11] = 0.0; spheres[1, 11] = 1.0; spheres[1, 3] = np.float32(0.3)
    elif name == "no_light":
        spheres[2, 4:7] = 0.0; spheres[2, 8:11] = np.float32([0.6, 0.6, 0.6])
    elif name == "diffuse_sphere":
        spheres[0, 8:11] = np.float32([0.7, 0.5, 0.3]); spheres[0, 11] = 1.0
    elif name == "two_spheres":
        spheres = spheres[[1, 2]].copy()
    elif name == "five_spheres":   # (two more in front, clear of the others: tests/test_abi.py)
        spheres = np.concatenate([spheres, spheres[:2] + np.float32([0, 0, 2.2] + [0] * 9)])
    elif name == "overlapping_spheres":
        spheres[1, 0:3] = spheres[0, 0:3] + np.float32([0.9, 0.0, 0.3])
    else:
        assert name == "default"
    return planes, spheres


CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
import __graft_entry__ as e
import test_gpu_pool_diet3 as T
B = e.load_package().bindings
O = e.load_oracle()
assert B.build_id()["variant"] == %(variant)r, B.build_id()
out = {}
with B.Context(0) as ctx:
    for tier in %(tiers)r:
        mode = getattr(B, T.TIERS[tier][0])
        # (PT_NO_FAST_GUARD: five spheres would otherwise send a fast request to the careful tier)
        flags = B.PT_NO_FAST_GUARD if mode == B.PT_MATH_FAST else 0
        def render(name, q, planes=None, spheres=None, acc=None):
            ki = B.pathtrace_select_kernel(q, planes, spheres)
            # (a scene without a light is no closed box to the host — lights_inside_box — and goes to the round-synchronous kernels, whose
            #  code is shared with the sample-pool kernels: rendered and compared all the same)
            assert (ki.kernel == B.PT_KERNEL_POOL or name == "no_light") and ki.math_mode == mode, (tier, name, ki.kernel, ki.math_mode)
            try:   # (the status word is checked by the blocking call: a tripped loop bound comes back as an error)
                out[tier + "/" + name] = ctx.pathtrace(q, planes=planes, spheres=spheres, acc=acc)
            except B.McError as err:
                print("STATUS", tier, name, err.status, err)
                raise
            return out[tier + "/" + name]
        for name, (W, H, spp, depth) in T.SHAPES.items():
            render(name, B.pathtrace_params(W, H, spp, math_mode=mode, max_depth=depth))
        W, H, spp, depth = T.SHAPES["38x22x20"]
        part = render(T.RANGES[0], B.pathtrace_params(W, H, spp, math_mode=mode, sample_begin=0, sample_end=16))
        render(T.RANGES[1], B.pathtrace_params(W, H, spp, math_mode=mode, sample_begin=16, sample_end=spp), acc=part.copy())
        for name, row_begin in zip(T.TILES, (0, T.ROW_BLOCK)):
            render(name, B.pathtrace_params(W, H, spp, math_mode=mode, row_begin=row_begin, row_end=H, row_block=T.ROW_BLOCK,
                                            row_stride=T.ROW_STRIDE))
        for name in T.SCENES:
            planes, spheres = T.scene(O, name)
            if name == "overlapping_spheres":
                assert B.pathtrace_scene_class(planes, spheres) & B.PT_SCENE_SPHERES_DISJOINT == 0
            W, H, spp = T.SCENE_SHAPE
            render(name, B.pathtrace_params(W, H, spp, math_mode=mode, flags=flags), planes, spheres)
np.savez(%(dest)r, **out)
print("RENDERED_MC_OK", len(out))
"""


@pytest.fixture(scope="module")
def renders(tmp_path_factory):
    """({tier/case: image} of the shipped library, the same of the three parent builds) — one child process per library."""
    from conftest import ROOT
    pkg = os.path.join(ROOT, "vulkan-compute-tests_amd")
    tmp = tmp_path_factory.mktemp("diet3")

    def child(variant, lib, tiers):
        dest = str(tmp / f"{variant}.npz")
        code = CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), variant=variant, dest=dest, tiers=list(tiers))
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, MC_LIB_PATH=os.path.join(pkg, "lib", lib)))
        # every blocking call returned MC_OK (the status word stayed clear: no render tripped the loop bound)
        assert r.returncode == 0 and "STATUS" not in r.stdout and f"RENDERED_MC_OK {len(CASES) * len(tiers)}" in r.stdout, \
            r.stdout + r.stderr[-3000:]
        with np.load(dest) as z:
            return {k: z[k] for k in z.files}

    old = {}
    for tier, (_, tu) in TIERS.items():
        name = "diet3parent" if tier == "fast" else f"diet3parent_{tier}"
        subprocess.check_call(["make", "-s", "-j", "8", "-C", pkg, "exp", f"EXP_NAME={name}", f"EXP_TU={tu}",
                               "EXP_FLAGS=-DMC_PT_POOL_DIET3_PARENT"])
        old.update(child(f"exp_{name}", f"libmc_compute_exp_{name}.so", [tier]))
    return child("shipped", "libmc_compute.so", list(TIERS)), old


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("tier", list(TIERS))
def test_diet3_keeps_every_bit(renders, tier, case):
    shipped, old = renders[0][f"{tier}/{case}"], renders[1][f"{tier}/{case}"]
    assert shipped.shape == old.shape and shipped.dtype == np.float32
    assert np.isfinite(shipped).all()
    assert np.array_equal(bits(shipped), bits(old))


def test_every_render_returned_mc_ok(renders):
    """The fixture asserts it of each child; here: every case of every tier was rendered by both builds."""
    for images in renders:
        assert sorted(images) == sorted(f"{tier}/{case}" for tier in TIERS for case in CASES)


@pytest.mark.parametrize("tier", list(TIERS))
def test_interleaved_tiles_are_the_whole_image(renders, tier):
    """The rows a tile stores (row_block = 8 of every row_stride = 16 from its row_begin) are the whole image's, bit for bit: a wave owns
    the same pixels in every tiling, and its schedule depends on nothing else."""
    W, H, _, _ = SHAPES["38x22x20"]
    whole = renders[0][f"{tier}/38x22x20"]
    for name, row_begin in zip(TILES, (0, ROW_BLOCK)):
        rows = [r for r in range(row_begin, H) if (r - row_begin) % ROW_STRIDE < ROW_BLOCK]
        tile = renders[0][f"{tier}/{name}"]
        assert tile.shape[0] == len(rows)
        assert np.array_equal(bits(tile), bits(whole[rows]))


def test_strict_still_equals_the_oracle(renders):
    from conftest import ROOT
    sys.path.insert(0, ROOT)
    import __graft_entry__ as e
    O = e.load_oracle()
    for name in ("38x22x20", "16x8x48"):
        W, H, spp, depth = SHAPES[name]
        ref = O.pathtrace(W, H, spp, math_mode=O.MATH_MC, max_depth=depth)
        assert np.array_equal(bits(renders[0][f"strict/{name}"]), bits(ref))


def test_small_case_reaches_the_changed_code():
    """16 x 8 x 48 on the CPU, from the oracle's bounce counts.  In a closed box every ray hits, so a path ends by the roulette or at the
    depth limit only, and the bounces a render gains when the limit is raised from d to d + 1 are the paths still going after d."""
    from conftest import ROOT
    sys.path.insert(0, ROOT)
    import __graft_entry__ as e
    O = e.load_oracle()
    W, H, spp, depth = SHAPES["16x8x48"]

    def bounces(max_depth, spheres=O.DEFAULT_SPHERES):
        return O.pathtrace(W, H, spp, spheres=spheres, math_mode=O.MATH_MC, max_depth=max_depth, counts=True)[1]["bounces"]

    going = {d: bounces(d + 1) - bounces(d) for d in (6, 7, depth)}
    assert going[6] > 0              # lanes past depth 5: the carried mask selects the colour row divided by p
    assert going[6] > going[7] > 0   # the roulette ends paths, and not all of them
    assert going[depth] > 0          # paths are cut at the depth limit
    # The light's colour is 0, so p = 0 and the roulette ends EVERY path that hits it past depth 5.  With a white light (p = 1) those
    # paths go on and nothing else changes (a colour moves no ray): the bounces gained are paths the roulette ended on the emitter.
    white = O.DEFAULT_SPHERES.copy().reshape(3, 12)
    assert np.all(white[2, 4:7] > 0) and np.all(white[2, 8:11] == 0)
    white[2, 8:11] = 1.0
    assert bounces(depth, white) > bounces(depth)
    assert spp % 16 == 0 and W % 4 == 0 and H % 4 == 0   # full batches, no pixel outside a block: no stash entry is ever empty
