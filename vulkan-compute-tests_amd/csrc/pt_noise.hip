// Path-tracer denoiser for gfx950 (MI355X): the measured noise plane and the a-trous filter whose colour tolerance it steers.  Contract in
// include/mc_compute.h, restated in tests/pt_noise_ref.py; scheme and measurements in DESIGN.md §3.19.  The arithmetic is pt_noise.h (and
// pt_denoise.h's filter_pixel), the same source mc_pathtrace_noise and mc_pathtrace_denoise_adaptive run on the host.  Built like
// pt_denoise.hip: no contraction, IEEE divide.
//
// Three kernels in the launch shape of pt_denoise.hip's (a lane owns ONE pixel, a wave 64 adjacent pixels of a storage row, a block of
// 64 x 4 four adjacent rows, blockIdx.y strides over the rows); vector loads and stores only, no LDS, no atomics, no synchronisation.
//  * pt_noise_v_kernel: two 16-B loads and one 4-B store per pixel; three strict pow(x, 0.45) between them.
//  * pt_noise_window_kernel: up to (2 r + 1)^2 4-B loads per pixel of the plane the first kernel wrote.  A tap row of a wave is one
//    contiguous 256-B segment, adjacent lanes' and adjacent rows' taps overlap: all but the compulsory 4 B come out of the vector cache.
//    radius is a run-time value (0 .. 4); the two loops are not unrolled.
//  * pt_denoise_adaptive_pass_kernel: pt_denoise_pass_kernel with one more 4-B load per pixel, the centre's V, and one division for
//    its colour weight; the 25 taps are the same function.
#include <cmath>
#include <vector>

#include "pt_denoise_host.h"
#include "pt_noise.h"

namespace mc {

namespace {

using ptd::vec4;
using namespace ptdh;

__global__ void __launch_bounds__(256) pt_noise_v_kernel(const vec4* __restrict__ half, const vec4* __restrict__ full, float* __restrict__ v,
                                                         uint32_t W, uint32_t H, float scale) {
    const uint32_t x = blockIdx.x * 64u + threadIdx.x;
    if (x >= W) return;
    for (uint32_t y = blockIdx.y * 4u + threadIdx.y; y < H; y += gridDim.y * 4u) {
        const size_t p = (size_t)y * W + x;
        v[p] = ptd::noise_pixel(half[p], scale, full[p]);
    }
}

__global__ void __launch_bounds__(256) pt_noise_window_kernel(const float* __restrict__ v, float* __restrict__ variance, uint32_t W, uint32_t H,
                                                              int radius) {
    const uint32_t x = blockIdx.x * 64u + threadIdx.x;
    if (x >= W) return;
    for (uint32_t y = blockIdx.y * 4u + threadIdx.y; y < H; y += gridDim.y * 4u) variance[(size_t)y * W + x] = ptd::noise_window(W, H, x, y, radius, v);
}

__global__ void __launch_bounds__(256) pt_denoise_adaptive_pass_kernel(const vec4* __restrict__ in, const vec4* __restrict__ normal_t,
                                                                       const vec4* __restrict__ position_id, const float* __restrict__ variance,
                                                                       vec4* __restrict__ out, uint32_t W, uint32_t H, uint32_t step, float scale4,
                                                                       float k2, float kn, float kx) {
    const uint32_t x = blockIdx.x * 64u + threadIdx.x;
    if (x >= W) return;
    for (uint32_t y = blockIdx.y * 4u + threadIdx.y; y < H; y += gridDim.y * 4u) {
        const size_t p = (size_t)y * W + x;
        const float kc = ptd::colour_weight_adaptive(scale4, k2, variance[p]);
        out[p] = ptd::filter_pixel(W, H, x, y, step, kc, kn, kx, in, normal_t, position_id, in[p], normal_t[p], position_id[p]);
    }
}

bool misaligned4(const void* p) { return reinterpret_cast<uintptr_t>(p) % 4u != 0u; }

}  // namespace

int pt_noise_check(uint32_t radius, const char* who) {
    if (radius > ptd::kMaxNoiseRadius) return refuse(who, "radius = " + std::to_string(radius) + " is above 4");
    return MC_OK;
}

int pt_noise_check_k(float k_noise, const char* who) {
    if (!(k_noise > 0.0f) || !std::isfinite(k_noise) || !std::isfinite(k_noise * k_noise))
        return refuse(who, "k_noise must be finite and above 0, and its fp32 square finite");
    return MC_OK;
}

int pt_noise_launch(mc_context* ctx, uint32_t W, uint32_t H, const void* d_half, float scale, const void* d_full, uint32_t radius, void* d_variance,
                    void* d_v, const char* who, hipStream_t s) {
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    if (!W || !H) return refuse(who, "width and height must be above 0");
    if (int rc = pt_noise_check(radius, who)) return rc;
    if (!d_half || !d_full || !d_variance || !d_v) return refuse(who, "a plane is NULL");
    if (misaligned(d_half) || misaligned(d_full)) return refuse(who, "the vec4 planes must be aligned to 16 bytes");
    if (misaligned4(d_variance) || misaligned4(d_v)) return refuse(who, "the variance plane must be aligned to 4 bytes");
    const size_t npix = (size_t)W * H;
    if (overlaps(d_variance, npix * 4, d_half, npix * 16) || overlaps(d_variance, npix * 4, d_full, npix * 16))
        return refuse(who, "the variance plane overlaps an input plane");
    hipLaunchKernelGGL(pt_noise_v_kernel, plane_grid(W, H), dim3(64, 4), 0, s, (const vec4*)d_half, (const vec4*)d_full, (float*)d_v, W, H, scale);
    MC_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(pt_noise_window_kernel, plane_grid(W, H), dim3(64, 4), 0, s, (const float*)d_v, (float*)d_variance, W, H, (int)radius);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

int pt_denoise_adaptive_launch(mc_context* ctx, const mc_pathtrace_denoise_params* d, float k_noise, const void* d_rgba, const void* d_normal_t,
                               const void* d_position_id, const void* d_variance, void* d_out, void* d_tmp0, void* d_tmp1, const char* who,
                               hipStream_t s) {
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    if (int rc = pt_denoise_check_params(d, who)) return rc;
    if (int rc = pt_noise_check_k(k_noise, who)) return rc;
    if (!d_rgba || !d_normal_t || !d_position_id || !d_variance || !d_out || !d_tmp0 || !d_tmp1) return refuse(who, "a plane is NULL");
    if (misaligned(d_rgba) || misaligned(d_normal_t) || misaligned(d_position_id) || misaligned(d_out) || misaligned(d_tmp0) || misaligned(d_tmp1))
        return refuse(who, "the vec4 planes must be aligned to 16 bytes");
    if (misaligned4(d_variance)) return refuse(who, "the variance plane must be aligned to 4 bytes");
    const uint32_t W = d->width, H = d->height;
    const size_t bytes = (size_t)W * H * 16;
    if (overlaps(d_out, bytes, d_normal_t, bytes) || overlaps(d_out, bytes, d_position_id, bytes) || overlaps(d_out, bytes, d_variance, bytes / 4) ||
        overlaps(d_rgba, bytes, d_normal_t, bytes) || overlaps(d_rgba, bytes, d_position_id, bytes) || overlaps(d_rgba, bytes, d_variance, bytes / 4) ||
        (d_out != d_rgba && overlaps(d_out, bytes, d_rgba, bytes)))
        return refuse(who, "the output overlaps a guide or variance plane, or the input without being the input (d_out == d_rgba is the in-place form)");
    // the passes travel as pt_denoise_launch's do: tmp[i & 1], the last one the output, a single pass in place through tmp0 and a copy
    void* const tmp[2] = {d_tmp0, d_tmp1};
    const void* src = d_rgba;
    const bool copy_back = d->passes == 1u && d_out == d_rgba;
    const float k2 = k_noise * k_noise;
    for (uint32_t i = 0; i < d->passes; i++) {
        void* dst = (i + 1u == d->passes && !copy_back) ? d_out : tmp[i & 1u];
        hipLaunchKernelGGL(pt_denoise_adaptive_pass_kernel, plane_grid(W, H), dim3(64, 4), 0, s, (const vec4*)src, (const vec4*)d_normal_t,
                           (const vec4*)d_position_id, (const float*)d_variance, (vec4*)dst, W, H, 1u << i, (float)(1u << (2u * i)), k2, d->k_normal,
                           d->k_position);
        MC_HIP_TRY(hipGetLastError());
        src = dst;
    }
    if (copy_back) MC_HIP_TRY(hipMemcpyAsync(d_out, src, bytes, hipMemcpyDeviceToDevice, s));
    return MC_OK;
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_pathtrace_noise_default_params(float* k_noise, uint32_t* radius) {
    if (!k_noise || !radius) return MC_ERR_INVALID_ARGUMENT;
    *k_noise = 4.0f;
    *radius = 3u;
    return MC_OK;
}

int mc_pathtrace_noise(uint32_t width, uint32_t height, const float* half, float scale, const float* full, uint32_t radius, float* out_variance) {
    const char* who = "mc_pathtrace_noise";
    if (!width || !height) return refuse(who, "width and height must be above 0");
    if (int rc = pt_noise_check(radius, who)) return rc;
    if (!half || !full || !out_variance) return refuse(who, "a plane is NULL");
    const size_t npix = (size_t)width * height;
    std::vector<vec4> s_half, s_full;
    ptd::noise_host(width, height, aligned_in(half, npix, s_half), scale, aligned_in(full, npix, s_full), radius, out_variance);
    return MC_OK;
}

int mc_pathtrace_noise_device_async(mc_context* ctx, uint32_t width, uint32_t height, const void* d_half, float scale, const void* d_full,
                                    uint32_t radius, void* d_variance, void* stream) {
    const char* who = "mc_pathtrace_noise_device_async";
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    if (!width || !height) return refuse(who, "width and height must be above 0");
    if (int rc = pt_noise_check(radius, who)) return rc;
    MC_HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = ctx->scratch_iters.reserve(pt_noise_plane_bytes((size_t)width * height))) return rc;
    return pt_noise_launch(ctx, width, height, d_half, scale, d_full, radius, d_variance, ctx->scratch_iters.ptr, who,
                           stream ? (hipStream_t)stream : ctx->stream);
}

int mc_pathtrace_denoise_adaptive(const mc_pathtrace_denoise_params* d, float k_noise, const float* rgba, const float* normal_t,
                                  const float* position_id, const float* variance, float* out) {
    const char* who = "mc_pathtrace_denoise_adaptive";
    if (int rc = pt_denoise_check_params(d, who)) return rc;
    if (int rc = pt_noise_check_k(k_noise, who)) return rc;
    if (!rgba || !normal_t || !position_id || !variance || !out) return refuse(who, "a plane is NULL");
    const size_t npix = (size_t)d->width * d->height;
    std::vector<vec4> s_rgba, s_nt, s_pid;
    const vec4* a_rgba = aligned_in(rgba, npix, s_rgba);
    const vec4* a_nt = aligned_in(normal_t, npix, s_nt);
    const vec4* a_pid = aligned_in(position_id, npix, s_pid);
    AlignedOut o(out, npix);
    ptd::denoise_adaptive_host(d->width, d->height, d->passes, k_noise, d->k_normal, d->k_position, a_rgba, a_nt, a_pid, variance, o.ptr());
    o.finish();
    return MC_OK;
}

int mc_pathtrace_denoise_adaptive_device_async(mc_context* ctx, const mc_pathtrace_denoise_params* d, float k_noise, const void* d_rgba,
                                               const void* d_normal_t, const void* d_position_id, const void* d_variance, void* d_out, void* stream) {
    const char* who = "mc_pathtrace_denoise_adaptive_device_async";
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    if (int rc = pt_denoise_check_params(d, who)) return rc;
    if (int rc = pt_noise_check_k(k_noise, who)) return rc;
    if (!d_rgba || !d_normal_t || !d_position_id || !d_variance || !d_out) return refuse(who, "a plane is NULL");
    MC_HIP_TRY(hipSetDevice(ctx->device));
    const size_t plane = (size_t)d->width * d->height * 16;
    if (int rc = ctx->scratch_iters.reserve(2 * plane)) return rc;
    char* base = static_cast<char*>(ctx->scratch_iters.ptr);
    return pt_denoise_adaptive_launch(ctx, d, k_noise, d_rgba, d_normal_t, d_position_id, d_variance, d_out, base, base + plane, who,
                                      stream ? (hipStream_t)stream : ctx->stream);
}

}  // extern "C"
