"""The path tracer's linear kernels (mc_pathtrace_render_device_async: every ray tests every object) against the BVH kernels
(mc_pathtrace_render_accel_device_async) on one context.

300 x 200 x 16 spp, strict and careful tier, scenes: lattices of 8, 64, 700 and 3500 spheres in the reference room, and a random room of
6000 spheres.  One process, device forms, HIP events around one launch, one warm launch of each variant, then the best of ROUNDS rounds
with the two variants alternating.  The host build of the tree and the first call (which uploads the object's device copy) are timed
apart, by wall clock.  Each strict pair of outputs is compared bit for bit, each careful pair too (reported, not required; the linear call renders a
careful request STRICT where a light touches a diffuse sphere, MC_PT_SCENE_LIGHT_ENCLOSED: the line says which tier it ran).
The last lines give the ratio per scene and the break-even sphere count (log-linear between the two scenes where the ratio crosses 1).
    On an MI355X:  python tools/pt_bvh_probe.py > profiles/pt_bvh_probe.txt"""
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import pt_bvh_ref as R  # noqa: E402

B = entry.load_package().bindings
ROUNDS = 5
W, H, SPP = 300, 200, 16


def event_ms(stream, launch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    launch()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def scenes():
    for n in (8, 64, 700, 3500):
        yield f"lattice {n}", R.ROOM.copy(), R.lattice(n)
    yield ("random room 6000",) + R.random_scene(np.random.default_rng(6000), 6, 6000, 4)


def main():
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# path tracer, linear against BVH: device {name}, {cus} CUs; shader clock under load {ctx.measure_clock():.0f} MHz; build {B.build_id()}")
    print(f"# {W} x {H} x {SPP} spp, max_depth 12; device forms, HIP events, one warm launch each, best of {ROUNDS} alternating rounds (worst in brackets)", flush=True)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    out_lin = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    out_bvh = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    ratios = {"strict": [], "careful": []}
    for label, planes, spheres in scenes():
        t0 = time.perf_counter()
        accel = B.PathtraceAccel(planes, spheres)
        build_ms = (time.perf_counter() - t0) * 1e3
        info = accel.info()
        print(f"{label}: {spheres.shape[0]} spheres, {planes.shape[0]} planes; tree: {info['nodes']} nodes, depth {info['depth']}, {info['leaves']} leaves, "
              f"{info['unboxed']} unboxed, {info['bytes']} bytes; host build {build_ms:.3f} ms", flush=True)
        first = True
        for tier, mode in (("strict", B.PT_MATH_STRICT), ("careful", B.PT_MATH_FAST_CAREFUL)):
            p = B.pathtrace_params(W, H, SPP, math_mode=mode)
            k_lin, k_bvh = B.pathtrace_select_kernel(p, planes, spheres), accel.select_kernel(p)
            lin = lambda: ctx.pathtrace_device(p, out_lin.data_ptr(), planes=planes, spheres=spheres, stream=s)   # noqa: E731
            bvh = lambda: ctx.pathtrace_accel_device(accel, p, out_bvh.data_ptr(), stream=s)                       # noqa: E731
            with torch.cuda.stream(stream):
                t0 = time.perf_counter()
                bvh()
                stream.synchronize()
                first_ms = (time.perf_counter() - t0) * 1e3
                lin()
                stream.synchronize()
                t = {"linear": [], "bvh": []}
                for _ in range(ROUNDS):
                    t["linear"].append(event_ms(stream, lin))
                    t["bvh"].append(event_ms(stream, bvh))
            same = bool(torch.equal(out_lin.view(torch.int32), out_bvh.view(torch.int32)))
            lo_l, lo_b = min(t["linear"]), min(t["bvh"])
            ratios[tier].append((spheres.shape[0], lo_l / lo_b))
            if first:
                print(f"    first BVH call (upload of the device copy + code object load + render): {first_ms:.3f} ms wall")
                first = False
            ran = {B.PT_MATH_STRICT: "strict", B.PT_MATH_FAST: "fast", B.PT_MATH_FAST_CAREFUL: "careful"}[k_lin.math_mode]
            print(f"    {tier:8s} linear ({B.PT_KERNEL_NAMES[k_lin.kernel]}, S = {k_lin.lanes_per_pixel}, runs {ran}) {lo_l:10.3f} ms ({max(t['linear']):10.3f})   "
                  f"bvh (S = {k_bvh.lanes_per_pixel}) {lo_b:9.3f} ms ({max(t['bvh']):9.3f})   linear / bvh = {lo_l / lo_b:7.2f}   outputs bit-equal: {same}",
                  flush=True)
        accel.close()
    for tier, rs in ratios.items():
        line = ", ".join(f"{n}: {r:.2f}" for n, r in rs)
        even = "not crossed in the range measured"
        for (n0, r0), (n1, r1) in zip(rs, rs[1:]):
            if (r0 - 1.0) * (r1 - 1.0) <= 0.0 and r0 != r1:
                even = f"about {math.exp(math.log(n0) + (math.log(n1) - math.log(n0)) * (1.0 - r0) / (r1 - r0)):.0f} spheres (between {n0} and {n1})"
                break
        if all(r > 1.0 for _, r in rs):
            even = f"below {rs[0][0]} spheres (the BVH is ahead on every scene measured)"
        print(f"# {tier}: linear / bvh by sphere count: {line}; break-even: {even}")
    print(f"# shader clock under load at the end {ctx.measure_clock():.0f} MHz", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
