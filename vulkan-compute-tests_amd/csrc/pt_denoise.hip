// Path-tracer denoiser for gfx950 (MI355X): the guide planes of the first hit and the edge-avoiding a-trous filter they steer.  The
// project's own addition (the reference writes the noisy image); contract in include/mc_compute.h, restated in tests/pt_denoise_ref.py;
// scheme and measurements in DESIGN.md §3.17.  The arithmetic is pt_denoise.h, the same source mc_pathtrace_guides and mc_pathtrace_denoise
// run on the host.  Built like the strict path tracer: no contraction, IEEE divide and square root (hipcc's default for HIP).
//
// Both kernels: a lane owns ONE pixel; a wave covers 64 adjacent pixels of a storage row, a block (64 x 4) four adjacent rows, blockIdx.y
// strides over the rows.  Vector loads and stores only, no LDS, no atomics, no synchronisation, no scratch.
//  * pt_guides_kernel: the centre ray against every record, read from memory with wave-uniform indices (one scalar load per record
//    and wave, as the path tracer's generic kernel for large scenes reads them); two 16-B stores per pixel, 1 KiB contiguous per wave.
//  * pt_denoise_pass_kernel: ONE pass of the filter.  The centre's colour, normal and position / id stay in registers; each of the 25 taps
//    reads the neighbour's position / id first and its colour and normal only where the ids agree and the neighbour lies in the image.  A
//    tap row of a wave is one contiguous 64-pixel segment of each plane whatever the step (coalesced 1-KiB loads); adjacent lanes' and
//    adjacent rows' taps overlap, so of the 25 x 48 B a pixel requests all but the compulsory 48 B come out of the vector cache and the L2.
//    Every step takes this one path (steps 1 and 2 could stage a tile with its halo in LDS; not done).
//    The passes are separate launches: a pass reads what the previous one wrote at a distance of up to 2 * 2^i pixels.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "pt_denoise.h"
#include "pt_denoise_host.h"

namespace mc {

namespace {

using ptd::vec4;
using namespace ptdh;

__global__ void __launch_bounds__(256) pt_guides_kernel(ptd::Camera cam, uint32_t W, uint32_t H, const float* __restrict__ rec, uint32_t n_planes,
                                                        uint32_t n_spheres, vec4* __restrict__ normal_t, vec4* __restrict__ position_id) {
    const uint32_t gx = blockIdx.x * 64u + threadIdx.x;
    if (gx >= W) return;
    for (uint32_t row = blockIdx.y * 4u + threadIdx.y; row < H; row += gridDim.y * 4u) {   // (storage row: pixel row H - 1 - row)
        vec4 nt, pid;
        ptd::guide_pixel(cam, W, H, gx, H - 1u - row, rec, n_planes, n_spheres, nt, pid);
        const size_t gid = (size_t)row * W + gx;
        normal_t[gid] = nt;
        position_id[gid] = pid;
    }
}

__global__ void __launch_bounds__(256) pt_denoise_pass_kernel(const vec4* __restrict__ in, const vec4* __restrict__ normal_t,
                                                              const vec4* __restrict__ position_id, vec4* __restrict__ out, uint32_t W, uint32_t H,
                                                              uint32_t step, float kc, float kn, float kx) {
    const uint32_t x = blockIdx.x * 64u + threadIdx.x;
    if (x >= W) return;
    for (uint32_t y = blockIdx.y * 4u + threadIdx.y; y < H; y += gridDim.y * 4u) {
        const size_t p = (size_t)y * W + x;
        out[p] = ptd::filter_pixel(W, H, x, y, step, kc, kn, kx, in, normal_t, position_id, in[p], normal_t[p], position_id[p]);
    }
}

std::vector<float> scene_records(const float* planes, uint32_t n_planes, const float* spheres, uint32_t n_spheres) {
    std::vector<float> rec(12 * ((size_t)n_planes + n_spheres));
    if (n_planes) std::memcpy(rec.data(), planes, sizeof(float) * 12 * n_planes);
    if (n_spheres) std::memcpy(rec.data() + 12 * (size_t)n_planes, spheres, sizeof(float) * 12 * n_spheres);
    return rec;
}

}  // namespace

int pt_denoise_check_params(const mc_pathtrace_denoise_params* d, const char* who) {
    if (!d) return refuse(who, "the denoise parameters are NULL");
    if (!d->width || !d->height) return refuse(who, "width and height must be above 0");
    if (d->passes < 1u || d->passes > ptd::kMaxPasses) return refuse(who, "passes = " + std::to_string(d->passes) + " is outside 1 .. 8");
    const float s2 = d->sigma_colour * d->sigma_colour;
    if (!(d->sigma_colour > 0.0f) || !std::isfinite(d->sigma_colour) || !(s2 > 0.0f) || !std::isfinite(s2))
        return refuse(who, "sigma_colour must be finite and above 0, and so must its fp32 square");
    if (!(d->k_normal >= 0.0f) || !std::isfinite(d->k_normal)) return refuse(who, "k_normal must be finite and not negative");
    if (!(d->k_position >= 0.0f) || !std::isfinite(d->k_position)) return refuse(who, "k_position must be finite and not negative");
    if (d->flags) return refuse(who, "flags must be 0");
    return MC_OK;
}

int pt_guides_check_scene(const float* planes, uint32_t n_planes, const float* spheres, uint32_t n_spheres, const char* who) {
    if ((!planes && n_planes) || (!spheres && n_spheres)) return refuse(who, "a scene table is NULL although its count is not 0");
    if ((size_t)n_planes + n_spheres > (1u << 20)) {
        set_error_detail(std::string(who) + ": more than 2^20 objects");
        return MC_ERR_UNSUPPORTED;
    }
    return MC_OK;
}

size_t pt_guides_records_bytes(uint32_t n_planes, uint32_t n_spheres) {
    const size_t bytes = (((size_t)n_planes + n_spheres) * 48 + 255) & ~(size_t)255;
    return bytes ? bytes : 256;   // (an empty scene: every pixel a miss; the launch still gets a pointer)
}

int pt_guides_launch(mc_context* ctx, uint32_t W, uint32_t H, const float* planes, uint32_t n_planes, const float* spheres, uint32_t n_spheres,
                     void* d_records, void* d_normal_t, void* d_position_id, const char* who, hipStream_t s) {
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    if (!W || !H) return refuse(who, "width and height must be above 0");
    if (int rc = pt_guides_check_scene(planes, n_planes, spheres, n_spheres, who)) return rc;
    if (!d_records || !d_normal_t || !d_position_id) return refuse(who, "an output plane is NULL");
    if (misaligned(d_normal_t) || misaligned(d_position_id) || misaligned(d_records)) return refuse(who, "the planes must be aligned to 16 bytes");
    const size_t bytes = (size_t)W * H * 16;
    if (overlaps(d_normal_t, bytes, d_position_id, bytes)) return refuse(who, "the two output planes overlap");
    const std::vector<float> rec = scene_records(planes, n_planes, spheres, n_spheres);
    if (!rec.empty()) {
        MC_HIP_TRY(hipMemcpyAsync(d_records, rec.data(), rec.size() * sizeof(float), hipMemcpyHostToDevice, s));
        MC_HIP_TRY(hipStreamSynchronize(s));   // pageable source `rec` (a local): staged before the call returns
    }
    hipLaunchKernelGGL(pt_guides_kernel, plane_grid(W, H), dim3(64, 4), 0, s, ptd::camera(), W, H, (const float*)d_records, n_planes, n_spheres,
                       (vec4*)d_normal_t, (vec4*)d_position_id);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

int pt_denoise_launch(mc_context* ctx, const mc_pathtrace_denoise_params* d, const void* d_rgba, const void* d_normal_t, const void* d_position_id,
                      void* d_out, void* d_tmp0, void* d_tmp1, const char* who, hipStream_t s) {
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    if (int rc = pt_denoise_check_params(d, who)) return rc;
    if (!d_rgba || !d_normal_t || !d_position_id || !d_out || !d_tmp0 || !d_tmp1) return refuse(who, "a plane is NULL");
    if (misaligned(d_rgba) || misaligned(d_normal_t) || misaligned(d_position_id) || misaligned(d_out) || misaligned(d_tmp0) || misaligned(d_tmp1))
        return refuse(who, "the planes must be aligned to 16 bytes");
    const uint32_t W = d->width, H = d->height;
    const size_t bytes = (size_t)W * H * 16;
    if (overlaps(d_out, bytes, d_normal_t, bytes) || overlaps(d_out, bytes, d_position_id, bytes) || overlaps(d_rgba, bytes, d_normal_t, bytes) ||
        overlaps(d_rgba, bytes, d_position_id, bytes) || (d_out != d_rgba && overlaps(d_out, bytes, d_rgba, bytes)))
        return refuse(who, "the output overlaps a guide plane, or the input without being the input (d_out == d_rgba is the in-place form)");
    // pass i reads the previous pass's plane and writes tmp[i & 1], the last one the output; a single pass in place goes through tmp0
    void* const tmp[2] = {d_tmp0, d_tmp1};
    const void* src = d_rgba;
    const bool copy_back = d->passes == 1u && d_out == d_rgba;
    for (uint32_t i = 0; i < d->passes; i++) {
        void* dst = (i + 1u == d->passes && !copy_back) ? d_out : tmp[i & 1u];
        hipLaunchKernelGGL(pt_denoise_pass_kernel, plane_grid(W, H), dim3(64, 4), 0, s, (const vec4*)src, (const vec4*)d_normal_t,
                           (const vec4*)d_position_id, (vec4*)dst, W, H, 1u << i, ptd::colour_weight(i, d->sigma_colour), d->k_normal, d->k_position);
        MC_HIP_TRY(hipGetLastError());
        src = dst;
    }
    if (copy_back) MC_HIP_TRY(hipMemcpyAsync(d_out, src, bytes, hipMemcpyDeviceToDevice, s));
    return MC_OK;
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_pathtrace_denoise_default_params(uint32_t width, uint32_t height, mc_pathtrace_denoise_params* d) {
    if (!d) return MC_ERR_INVALID_ARGUMENT;
    std::memset(d, 0, sizeof(*d));
    d->width = width; d->height = height;
    d->passes = 5;
    d->sigma_colour = 128.0f;
    d->k_normal = 8.0f;
    d->k_position = 4.0f;
    return MC_OK;
}

int mc_pathtrace_guides(uint32_t width, uint32_t height, const float* planes, uint32_t n_planes, const float* spheres, uint32_t n_spheres,
                        float* out_normal_t, float* out_position_id) {
    const char* who = "mc_pathtrace_guides";
    if (!width || !height) return refuse(who, "width and height must be above 0");
    if (int rc = pt_guides_check_scene(planes, n_planes, spheres, n_spheres, who)) return rc;
    if (!out_normal_t || !out_position_id) return refuse(who, "an output plane is NULL");
    const size_t npix = (size_t)width * height;
    const std::vector<float> rec = scene_records(planes, n_planes, spheres, n_spheres);
    AlignedOut nt(out_normal_t, npix), pid(out_position_id, npix);
    ptd::guides_host(width, height, rec.data(), n_planes, n_spheres, nt.ptr(), pid.ptr());
    nt.finish();
    pid.finish();
    return MC_OK;
}

int mc_pathtrace_guides_device_async(mc_context* ctx, uint32_t width, uint32_t height, const float* planes, uint32_t n_planes, const float* spheres,
                                     uint32_t n_spheres, void* d_normal_t, void* d_position_id, void* stream) {
    const char* who = "mc_pathtrace_guides_device_async";
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    if (int rc = pt_guides_check_scene(planes, n_planes, spheres, n_spheres, who)) return rc;
    MC_HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = ctx->scratch_iters.reserve(pt_guides_records_bytes(n_planes, n_spheres))) return rc;
    return pt_guides_launch(ctx, width, height, planes, n_planes, spheres, n_spheres, ctx->scratch_iters.ptr, d_normal_t, d_position_id, who,
                            stream ? (hipStream_t)stream : ctx->stream);
}

int mc_pathtrace_denoise(const mc_pathtrace_denoise_params* d, const float* rgba, const float* normal_t, const float* position_id, float* out) {
    const char* who = "mc_pathtrace_denoise";
    if (int rc = pt_denoise_check_params(d, who)) return rc;
    if (!rgba || !normal_t || !position_id || !out) return refuse(who, "a plane is NULL");
    const size_t npix = (size_t)d->width * d->height;
    std::vector<vec4> s_rgba, s_nt, s_pid;
    const vec4* a_rgba = aligned_in(rgba, npix, s_rgba);
    const vec4* a_nt = aligned_in(normal_t, npix, s_nt);
    const vec4* a_pid = aligned_in(position_id, npix, s_pid);
    AlignedOut o(out, npix);
    ptd::denoise_host(d->width, d->height, d->passes, d->sigma_colour, d->k_normal, d->k_position, a_rgba, a_nt, a_pid, o.ptr());
    o.finish();
    return MC_OK;
}

int mc_pathtrace_denoise_device_async(mc_context* ctx, const mc_pathtrace_denoise_params* d, const void* d_rgba, const void* d_normal_t,
                                      const void* d_position_id, void* d_out, void* stream) {
    const char* who = "mc_pathtrace_denoise_device_async";
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    if (int rc = pt_denoise_check_params(d, who)) return rc;
    if (!d_rgba || !d_normal_t || !d_position_id || !d_out) return refuse(who, "a plane is NULL");
    MC_HIP_TRY(hipSetDevice(ctx->device));
    const size_t plane = (size_t)d->width * d->height * 16;
    if (int rc = ctx->scratch_iters.reserve(2 * plane)) return rc;
    char* base = static_cast<char*>(ctx->scratch_iters.ptr);
    return pt_denoise_launch(ctx, d, d_rgba, d_normal_t, d_position_id, d_out, base, base + plane, who, stream ? (hipStream_t)stream : ctx->stream);
}

}  // extern "C"
