// Path-tracer denoiser for gfx950 (MI355X): the guide planes of the first hit through the sphere BVH of an mc_pathtrace_accel.  Contract in
// include/mc_compute.h (mc_pathtrace_accel_guides); scheme and measurements in DESIGN.md §3.24.  The arithmetic is pt_bvh_guides.h, the
// same source mc_pathtrace_accel_guides runs on the host.  Built like pt_denoise.hip: no contraction, IEEE divide and square root.
//
// pt_guides_bvh_kernel keeps pt_guides_kernel's mapping: a lane owns ONE pixel; a wave covers 64 adjacent pixels of a storage row, a block
// (64 x 4) four adjacent rows, blockIdx.y strides over the rows; two 16-B vector stores per pixel, 1 KiB contiguous per wave.  The planes
// and the unboxed list are read with wave-uniform indices; the walk is per lane and stackless (pt_bvh.h): a node is two 16-B vector loads, a
// leaf sphere one 16-B and one 4-B vector load.  Centre rays of adjacent pixels walk nearly the same nodes, so a wave's loads of one step
// mostly fall on one or two cache lines.  No LDS, no atomics, no private array, no scratch, no synchronisation.  The tree is the
// object's cached device copy: nothing is uploaded per call.
#include "pt_bvh_device.h"
#include "pt_bvh_guides.h"
#include "pt_denoise_host.h"

namespace mc {

namespace {

using ptd::vec4;
using namespace ptdh;

__global__ void __launch_bounds__(256) pt_guides_bvh_kernel(ptd::Camera cam, uint32_t W, uint32_t H, bvh::View view, vec4* __restrict__ normal_t,
                                                            vec4* __restrict__ position_id) {
    const uint32_t gx = blockIdx.x * 64u + threadIdx.x;
    if (gx >= W) return;
    for (uint32_t row = blockIdx.y * 4u + threadIdx.y; row < H; row += gridDim.y * 4u) {   // (storage row: pixel row H - 1 - row)
        vec4 nt, pid;
        ptd::guide_pixel_bvh(cam, W, H, gx, H - 1u - row, view, nt, pid);
        const size_t gid = (size_t)row * W + gx;
        normal_t[gid] = nt;
        position_id[gid] = pid;
    }
}

}  // namespace

int pt_accel_guides_check(const mc_pathtrace_accel* a, const char* who) {
    if (!a) return refuse(who, "a NULL pointer");
    if (!pt_accel_live(a)) return refuse(who, "not a live mc_pathtrace_accel (destroyed already?)");
    return MC_OK;
}

int pt_accel_guides_launch(mc_context* ctx, const mc_pathtrace_accel* a, uint32_t W, uint32_t H, void* d_normal_t, void* d_position_id,
                           const char* who, hipStream_t s) {
    if (int rc = pt_accel_guides_check(a, who)) return rc;
    if (!W || !H) return refuse(who, "width and height must be above 0");
    if (!d_normal_t || !d_position_id) return refuse(who, "an output plane is NULL");
    if (misaligned(d_normal_t) || misaligned(d_position_id)) return refuse(who, "the planes must be aligned to 16 bytes");
    const size_t bytes = (size_t)W * H * 16;
    if (overlaps(d_normal_t, bytes, d_position_id, bytes)) return refuse(who, "the two output planes overlap");
    if (!ctx) return refuse(who, "the context is NULL");
    bvh::View view{};
    if (int rc = pt_accel_device_view(ctx, a, s, view)) return rc;
    hipLaunchKernelGGL(pt_guides_bvh_kernel, plane_grid(W, H), dim3(64, 4), 0, s, ptd::camera(), W, H, view, (vec4*)d_normal_t, (vec4*)d_position_id);
    MC_HIP_TRY(hipGetLastError());
    return ctx->note_launch(s);   // the kernel reads the cached device copy
}

}  // namespace mc

extern "C" {

int mc_pathtrace_accel_guides_device_async(mc_context* ctx, const mc_pathtrace_accel* a, uint32_t width, uint32_t height, void* d_normal_t,
                                           void* d_position_id, void* stream) {
    const char* who = "mc_pathtrace_accel_guides_device_async";
    // (the context is asked for last among the checks; the device is made current only once they have passed)
    if (int rc = mc::pt_accel_guides_check(a, who)) return rc;
    if (!width || !height) return mc::ptdh::refuse(who, "width and height must be above 0");
    if (!d_normal_t || !d_position_id) return mc::ptdh::refuse(who, "an output plane is NULL");
    if (!ctx) return mc::ptdh::refuse(who, "the context is NULL");
    MC_HIP_TRY(hipSetDevice(ctx->device));
    return mc::pt_accel_guides_launch(ctx, a, width, height, d_normal_t, d_position_id, who, stream ? (hipStream_t)stream : ctx->stream);
}

}  // extern "C"
