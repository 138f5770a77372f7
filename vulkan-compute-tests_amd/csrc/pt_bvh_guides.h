// Path-tracer denoiser guides through the sphere BVH (include/mc_compute.h, mc_pathtrace_accel_guides).
//
// One body for the host and the device; nothing of HIP is needed to include this file (tools/pt_accel_guides_host_check.cpp compiles it
// with g++).  pt_guides_bvh_kernel (pt_bvh_guides.hip) and mc_pathtrace_accel_guides (pt_bvh_host.cpp) run guide_pixel_bvh below: the
// centre ray and the tail of ptd::guide_pixel (pt_denoise.h) with bvh::intersect_bvh<IeeeOps> (pt_bvh.h) between them in place of the
// linear loop.  The walk returns the loop's (id, t) for every ray, so the two vec4s are mc_pathtrace_guides' for the tables the object was
// made from, bit for bit.  IeeeOps in every math mode: the guides are strict whatever the render's tier is.  Requires -ffp-contract=off.
#pragma once
#include "pt_bvh.h"
#include "pt_denoise.h"

namespace mc {
namespace ptd {

// v.rec: the records, planes then spheres; slots 0 .. 3 of each are read (the tables' own values in the host and in the device copy).
MC_PTD_FN void guide_pixel_bvh(const Camera& cam, uint32_t W, uint32_t H, uint32_t gx, uint32_t gy, const bvh::View& v, vec4& normal_t,
                               vec4& position_id) {
    f3 o, d;
    guide_ray(cam, W, H, gx, gy, o, d);
    float t;
    const int32_t id = bvh::intersect_bvh<bvh::IeeeOps>(v, bvh::f3{o.x, o.y, o.z}, bvh::f3{d.x, d.y, d.z}, t);   // -1: a miss, t >= 1e20
    guide_tail(o, d, t, id, v.rec, v.n_planes, normal_t, position_id);
}

inline void guides_bvh_host(uint32_t W, uint32_t H, const bvh::View& v, vec4* normal_t, vec4* position_id) {
    const Camera cam = camera();
    for (uint32_t gy = 0; gy < H; gy++)
        for (uint32_t gx = 0; gx < W; gx++) {
            const size_t gid = (size_t)(H - 1u - gy) * W + gx;
            guide_pixel_bvh(cam, W, H, gx, gy, v, normal_t[gid], position_id[gid]);
        }
}

}  // namespace ptd
}  // namespace mc
