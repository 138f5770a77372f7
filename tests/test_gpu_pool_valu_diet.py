"""The sample-pool kernels ask their loop predicates of lane masks they already hold (csrc/pathtrace_pool.h): the termination test
takes its two ballots only once the last batch has been produced, "is any diffuse lane on a sphere" reads the mask of the prologue's
own compare, and the emission of a path the roulette ends is added by the emitters' lanes alone instead of by every ended lane whenever
one of them had hit an emitter.  No floating-point operation changes except that last one, which leaves out additions of +-0 to a sum
that is never -0 — so every image must keep its bits, in all three math tiers.  The earlier forms stay compilable for exactly this
comparison (-DMC_PT_POOL_PARENT_FORMS through `make exp`, one library per tier's translation unit): the shipped library and those three
render every case below in a child process each, and the storage buffers must be equal bit for bit, every pixel."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (W, H, spp, max_depth) — the shapes of test_gpu_pool_trans_groups.py: a width that cuts the 2 x 2 wave tiles with a ragged last batch
# (the drain: the termination test's ballots); one pixel; paths that end before and right after the first bounce; several blocks
SHAPES = {"33x9x37": (33, 9, 37, 12), "1x1x500": (1, 1, 500, 12), "40x24x33_depth1": (40, 24, 33, 1), "40x24x33_depth2": (40, 24, 33, 2),
          "64x48x100": (64, 48, 100, 12)}
# that file's scenes — two lights, a diffuse non-emitting sphere (the general-basis bounce: the sphere mask is not empty) with a mirror
# wall, overlapping spheres — and a glass sphere that emits: the roulette then ends paths on an emitter that is not the diffuse light
SCENES = ("two_lights", "diffuse_sphere_and_mirror_wall", "overlapping_spheres", "emitting_glass")
# a later sample range of 33x9x37 (the stored accumulator, a drain with a ragged last batch), with the range before it
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
            out[tier + "/" + name] = ctx.pathtrace(q, planes=planes, spheres=spheres, acc=acc)
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
print("RENDERED", len(out))
"""


@pytest.fixture(scope="module")
def renders(tmp_path_factory):
    """({tier/case: image} of the shipped library, the same of the three parent-form builds) — one child process per library."""
    from conftest import ROOT
    pkg = os.path.join(ROOT, "vulkan-compute-tests_amd")
    tmp = tmp_path_factory.mktemp("valu_diet")

    def child(variant, lib, tiers):
        dest = str(tmp / f"{variant}.npz")
        code = CHILD % dict(root=ROOT, variant=variant, shapes=SHAPES, scenes=SCENES, dest=dest, tiers=[(t, TIERS[t][0]) for t in tiers])
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, MC_LIB_PATH=os.path.join(pkg, "lib", lib)))
        assert r.returncode == 0 and f"RENDERED {len(CASES) * len(tiers)}" in r.stdout, r.stdout + r.stderr[-3000:]
        with np.load(dest) as z:
            return {k: z[k] for k in z.files}

    parent = {}
    for tier, (_, tu) in TIERS.items():
        name = "parentforms" if tier == "fast" else f"parentforms_{tier}"
        subprocess.check_call(["make", "-s", "-j", "8", "-C", pkg, "exp", f"EXP_NAME={name}", f"EXP_TU={tu}",
                               "EXP_FLAGS=-DMC_PT_POOL_PARENT_FORMS"])
        parent.update(child(f"exp_{name}", f"libmc_compute_exp_{name}.so", [tier]))
    return child("shipped", "libmc_compute.so", list(TIERS)), parent


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("tier", list(TIERS))
def test_mask_predicates_keep_every_bit(renders, tier, case):
    shipped, parent = renders[0][f"{tier}/{case}"], renders[1][f"{tier}/{case}"]
    assert shipped.shape == parent.shape and shipped.dtype == np.float32
    assert np.isfinite(shipped).all()
    assert np.array_equal(np.ascontiguousarray(shipped).view(np.uint32), np.ascontiguousarray(parent).view(np.uint32))


def test_strict_still_equals_the_oracle(renders):
    from conftest import ROOT
    sys.path.insert(0, ROOT)
    import __graft_entry__ as e
    O = e.load_oracle()
    W, H, spp, depth = SHAPES["33x9x37"]
    ref = O.pathtrace(W, H, spp, math_mode=O.MATH_MC, max_depth=depth)
    got = renders[0]["strict/33x9x37"]
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(ref).view(np.uint32))
