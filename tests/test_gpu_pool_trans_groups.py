"""The fast sample-pool kernel issues the transcendentals of a bounce whose operands are known early as prioritised groups
(csrc/mc_math.h light_trans_group / bounce_trans_group: s_setprio 3, the transcendentals back to back, s_setprio 0): the light
sample's 1 / |xc| with the sine and cosine of its angle, and the cosine bounce's two square roots with its sine and cosine.  A group
holds the opcodes the compiler emitted before, on the same operands — only WHEN they are issued changes — so every image must keep
its bits.  The order before the groups stays compilable for exactly this comparison (-DMC_PT_TRANS_UNGROUPED through `make exp`): both
libraries render every case below in a child process of their own, and the storage buffers must be equal bit for bit, every pixel."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (W, H, spp, max_depth): a width that cuts the 2 x 2 wave tiles with a ragged last batch; one pixel; paths that end before and right
# after the first bounce group; several blocks
SHAPES = {"33x9x37": (33, 9, 37, 12), "1x1x500": (1, 1, 500, 12), "40x24x33_depth1": (40, 24, 33, 1), "40x24x33_depth2": (40, 24, 33, 2),
          "64x48x100": (64, 48, 100, 12)}
# the scenes of test_gpu_pool.py's variants: two lights (two light groups in an iteration), a diffuse non-emitting sphere (the
# general-basis bounce) with a mirror wall, overlapping spheres (the Disjoint = false instantiation)
SCENES = ("two_lights", "diffuse_sphere_and_mirror_wall", "overlapping_spheres")
CASES = list(SHAPES) + list(SCENES)

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
    for name, (W, H, spp, depth) in SHAPES.items():
        q = B.pathtrace_params(W, H, spp, math_mode=B.PT_MATH_FAST, max_depth=depth)
        ki = B.pathtrace_select_kernel(q)
        assert ki.kernel == B.PT_KERNEL_POOL and ki.math_mode == B.PT_MATH_FAST, name
        out[name] = ctx.pathtrace(q)
    for name in %(scenes)r:
        planes, spheres = O.DEFAULT_PLANES.copy().reshape(6, 12), O.DEFAULT_SPHERES.copy().reshape(3, 12)
        if name == "two_lights":
            spheres[1, 4:7] = np.float32([40.0, 30.0, 20.0]); spheres[1, 8:11] = 0.0; spheres[1, 11] = 1.0; spheres[1, 3] = np.float32(0.3)
        elif name == "diffuse_sphere_and_mirror_wall":
            spheres[0, 8:11] = np.float32([0.7, 0.5, 0.3]); spheres[0, 11] = 1.0
            planes[4, 11] = 2.0; planes[4, 8:11] = np.float32(0.9)
        else:
            spheres[1, 0:3] = spheres[0, 0:3] + np.float32([0.9, 0.0, 0.3])
            assert B.pathtrace_scene_class(planes, spheres) & B.PT_SCENE_SPHERES_DISJOINT == 0
        # (PT_NO_FAST_GUARD: the mirror wall would otherwise send a fast request to the careful tier, which has no groups)
        q = B.pathtrace_params(96, 64, 64, math_mode=B.PT_MATH_FAST, flags=B.PT_NO_FAST_GUARD)
        ki = B.pathtrace_select_kernel(q, planes, spheres)
        assert ki.kernel == B.PT_KERNEL_POOL and ki.math_mode == B.PT_MATH_FAST, name
        out[name] = ctx.pathtrace(q, planes=planes, spheres=spheres)
np.savez(%(dest)r, **out)
print("RENDERED", len(out))
"""


@pytest.fixture(scope="module")
def renders(tmp_path_factory):
    """{library: {case: image}} — the shipped library and the build with the groups compiled out, one child process each."""
    from conftest import ROOT
    pkg = os.path.join(ROOT, "vulkan-compute-tests_amd")
    subprocess.check_call(["make", "-s", "-j", "8", "-C", pkg, "exp", "EXP_NAME=ungrouped", "EXP_FLAGS=-DMC_PT_TRANS_UNGROUPED"])
    tmp = tmp_path_factory.mktemp("trans_groups")
    got = {}
    for variant, lib in (("shipped", "libmc_compute.so"), ("exp_ungrouped", "libmc_compute_exp_ungrouped.so")):
        dest = str(tmp / f"{variant}.npz")
        child = CHILD % dict(root=ROOT, variant=variant, shapes=SHAPES, scenes=SCENES, dest=dest)
        r = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, MC_LIB_PATH=os.path.join(pkg, "lib", lib)))
        assert r.returncode == 0 and f"RENDERED {len(CASES)}" in r.stdout, r.stdout + r.stderr[-3000:]
        with np.load(dest) as z:
            got[variant] = {k: z[k] for k in z.files}
    return got


@pytest.mark.parametrize("case", CASES)
def test_grouped_transcendentals_keep_every_bit(renders, case):
    grouped, ungrouped = renders["shipped"][case], renders["exp_ungrouped"][case]
    assert grouped.shape == ungrouped.shape and grouped.dtype == np.float32
    assert np.isfinite(grouped).all()
    assert np.array_equal(np.ascontiguousarray(grouped).view(np.uint32), np.ascontiguousarray(ungrouped).view(np.uint32))
