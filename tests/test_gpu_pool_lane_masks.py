"""The sample-pool kernels carry a lane's two one-bit facts as lane masks (csrc/pathtrace_pool.h): `alive` as a wave-uniform 64-bit value
in scalar registers, changed only by scalar and / or of compares' masks where all lanes pass — so the depth limit, the intersection, the
next bounce's random numbers and the roulette follow the bounce block instead of nesting in it — and `emissive`, once a 0.0f / 1.0f
factor, as a condition: the three emission sites add accmat * e in the lanes where it holds and leave out the multiplications by 1 and
the additions of +-0.  `key` is incremented in place, alpha = 1 is materialised once.  No
floating-point operation changes its operands or its order, so every image must keep its bits, in all three math tiers (the strict tier
takes the condition only: the mask form cost it scratch).  The earlier forms stay compilable for exactly this comparison
(-DMC_PT_POOL_FLOAT_STATE through `make exp`, one library per tier's translation unit): the shipped library and those three render
every case below in a child process each, and the storage buffers must be equal bit for bit, every pixel.  A render that trips the loop
bound sets the status word and fails its blocking call: every call must return MC_OK."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (W, H, spp, max_depth): a width that cuts the 2 x 2 wave tiles with a ragged last batch (the drain, where alive_m decides
# termination); one pixel (three of four pixel rows of every wave never alive); paths that end before and right after the first bounce
# (key at its limit, the emission condition read before it is ever cleared, lanes that die and refill in consecutive iterations)
SHAPES = {"33x9x37": (33, 9, 37, 12), "1x1x500": (1, 1, 500, 12), "40x24x33_depth1": (40, 24, 33, 1), "40x24x33_depth2": (40, 24, 33, 2)}
# the scenes of test_gpu_pool_valu_diet.py at 96 x 64 x 64.  emitting_glass and the mirror wall: a specular bounce followed by a hit of
# an emitter (the condition holds where it is used); two_lights: the roulette ends paths on an emitter after a diffuse bounce (it does not)
SCENES = ("two_lights", "diffuse_sphere_and_mirror_wall", "overlapping_spheres", "emitting_glass")
# the two sample ranges of 33x9x37, the second continuing the first's accumulator
RANGES = ("33x9_samples_0_16", "33x9_samples_16_37")
CASES = list(SHAPES) + list(SCENES) + list(RANGES)
TIERS = {"fast": ("PT_MATH_FAST", "pathtrace_fast"), "careful": ("PT_MATH_FAST_CAREFUL", "pathtrace_careful"),
         "strict": ("PT_MATH_STRICT", "pathtrace_strict")}

CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np
import __graft_entry__ as e
B = e.load_package().bindings
O = e.load_oracle()
assert B.build_id()["variant"] == %(variant)r, B.build_id()
SHAPES = %(shapes)r
out = {}
with B.Context(0) as ctx:
    for tier, mode_name in %(tiers)r:
        mode = getattr(B, mode_name)
        # (PT_NO_FAST_GUARD: a mirror wall or an enclosed light would otherwise send a fast request to the careful tier)
        flags = B.PT_NO_FAST_GUARD if mode == B.PT_MATH_FAST else 0
        def render(name, q, planes=None, spheres=None, acc=None):
            ki = B.pathtrace_select_kernel(q, planes, spheres)
            assert ki.kernel == B.PT_KERNEL_POOL and ki.math_mode == mode, (tier, name, ki.kernel, ki.math_mode)
            try:   # (the status word is checked by the blocking call: a tripped loop bound comes back as an error)
                out[tier + "/" + name] = ctx.pathtrace(q, planes=planes, spheres=spheres, acc=acc)
            except B.McError as err:
                print("STATUS", tier, name, err.status, err)
                raise
            return out[tier + "/" + name]
        for name, (W, H, spp, depth) in SHAPES.items():
            render(name, B.pathtrace_params(W, H, spp, math_mode=mode, max_depth=depth))
        for name in %(scenes)r:
            planes, spheres = O.DEFAULT_PLANES.copy().reshape(6, 12), O.DEFAULT_SPHERES.copy().reshape(3, 12)
            if name == "two_lights":
                spheres[1, 4:7] = np.float32([40.0, 30.0, 20.0]); spheres[1, 8:11] = 0.0; spheres[1, 11] = 1.0; spheres[1, 3] = np.float32(0.3)
            elif name == "diffuse_sphere_and_mirror_wall":
                spheres[0, 8:11] = np.float32([0.7, 0.5, 0.3]); spheres[0, 11] = 1.0
                planes[4, 11] = 2.0; planes[4, 8:11] = np.float32(0.9)
            elif name == "overlapping_spheres":
                spheres[1, 0:3] = spheres[0, 0:3] + np.float32([0.9, 0.0, 0.3])
                assert B.pathtrace_scene_class(planes, spheres) & B.PT_SCENE_SPHERES_DISJOINT == 0
            else:
                assert spheres[1, 11] == 3.0
                spheres[1, 4:7] = np.float32([3.0, 2.0, 1.0]); spheres[1, 3] = np.float32(0.5)   # (a light must clear the floor)
            render(name, B.pathtrace_params(96, 64, 64, math_mode=mode, flags=flags), planes, spheres)
        part = render("33x9_samples_0_16", B.pathtrace_params(33, 9, 37, math_mode=mode, sample_begin=0, sample_end=16))
        render("33x9_samples_16_37", B.pathtrace_params(33, 9, 37, math_mode=mode, sample_begin=16, sample_end=37), acc=part.copy())
np.savez(%(dest)r, **out)
print("RENDERED_MC_OK", len(out))
"""


@pytest.fixture(scope="module")
def renders(tmp_path_factory):
    """({tier/case: image} of the shipped library, the same of the three float-state builds) — one child process per library."""
    from conftest import ROOT
    pkg = os.path.join(ROOT, "vulkan-compute-tests_amd")
    tmp = tmp_path_factory.mktemp("lane_masks")

    def child(variant, lib, tiers):
        dest = str(tmp / f"{variant}.npz")
        code = CHILD % dict(root=ROOT, variant=variant, shapes=SHAPES, scenes=SCENES, dest=dest, tiers=[(t, TIERS[t][0]) for t in tiers])
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, MC_LIB_PATH=os.path.join(pkg, "lib", lib)))
        # every blocking call returned MC_OK (the status word stayed clear: no render tripped the loop bound)
        assert r.returncode == 0 and "STATUS" not in r.stdout and f"RENDERED_MC_OK {len(CASES) * len(tiers)}" in r.stdout, \
            r.stdout + r.stderr[-3000:]
        with np.load(dest) as z:
            return {k: z[k] for k in z.files}

    old = {}
    for tier, (_, tu) in TIERS.items():
        name = "floatstate" if tier == "fast" else f"floatstate_{tier}"
        subprocess.check_call(["make", "-s", "-j", "8", "-C", pkg, "exp", f"EXP_NAME={name}", f"EXP_TU={tu}",
                               "EXP_FLAGS=-DMC_PT_POOL_FLOAT_STATE"])
        old.update(child(f"exp_{name}", f"libmc_compute_exp_{name}.so", [tier]))
    return child("shipped", "libmc_compute.so", list(TIERS)), old


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("tier", list(TIERS))
def test_lane_masks_keep_every_bit(renders, tier, case):
    shipped, old = renders[0][f"{tier}/{case}"], renders[1][f"{tier}/{case}"]
    assert shipped.shape == old.shape and shipped.dtype == np.float32
    assert np.isfinite(shipped).all()
    assert np.array_equal(np.ascontiguousarray(shipped).view(np.uint32), np.ascontiguousarray(old).view(np.uint32))


def test_every_render_returned_mc_ok(renders):
    """The fixture asserts it of each child; here: every case of every tier was rendered by both builds."""
    for images in renders:
        assert sorted(images) == sorted(f"{tier}/{case}" for tier in TIERS for case in CASES)


def test_strict_still_equals_the_oracle(renders):
    from conftest import ROOT
    sys.path.insert(0, ROOT)
    import __graft_entry__ as e
    O = e.load_oracle()
    W, H, spp, depth = SHAPES["33x9x37"]
    ref = O.pathtrace(W, H, spp, math_mode=O.MATH_MC, max_depth=depth)
    got = renders[0]["strict/33x9x37"]
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(ref).view(np.uint32))
