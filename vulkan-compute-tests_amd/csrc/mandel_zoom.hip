// Zoom sequences of the Mandelbrot image for gfx950 (MI355X): a frame composed from the two keyframes that bracket it.  The project's own
// addition (the reference renders one still); contract in include/mc_compute.h, restated in tests/mandel_zoom_ref.py; scheme and
// measurements in DESIGN.md §3.16.  The arithmetic is mandel_zoom.h, the same source mc_mandelbrot_zoom_compose runs on the host.
//
// A memory-bound resample: four gathers of a texel's rgb (the compiler issues 12-B loads: alpha is never read) and one 16-B (and / or
// one 4-B) store per pixel, no dependence on depth, precision or colouring.
//  * a lane owns ONE output pixel; a wave covers 64 adjacent pixels of a row, a block (64 x 4) four adjacent rows, blockIdx.y strides
//    over the rows.  The frame magnifies the wide keyframe by 1 / r in [1, 2] and minifies the deep one by 2 r in [1, 2], so adjacent lanes
//    read adjacent or identical texels: a wave's four gathers touch at most 2 KiB of two rows each, and the second row is the next row's
//    first.  A wave's store is 1 KiB contiguous (256 B for the bytes).
//  * the column's share of the geometry (X, the source test's column half, x0, x1, fx for both keyframes) is computed once per lane,
//    before the row loop; the row's once per row and lane, not per tap: it is uniform over a wave but runs in the vector unit, a few
//    fp64 operations beside four gathers.
//  * which keyframe a pixel reads is decided per pixel; both branches are the same four loads from another base, so the choice is a
//    select of pointer and taps, not a branch.
// No LDS, no atomics, no synchronisation; vector loads and stores only.
#include <algorithm>
#include <cmath>
#include <cstdio>

#include "mandel_zoom.h"
#include "mandel_zoom_host.h"

namespace mc {

namespace {

// wide, deep (or null): W x H vec4.  out_rgba (vec4) / out_u8 (packed RGBA8): W x H; either may be null.
__global__ void __launch_bounds__(256) mandel_zoom_kernel(const float4* __restrict__ wide, const float4* __restrict__ deep,
                                                          float4* __restrict__ out_rgba, uint32_t* __restrict__ out_u8, uint32_t W,
                                                          uint32_t H, double r) {
    const uint32_t gx = blockIdx.x * 64u + threadIdx.x;
    if (gx >= W) return;
    const bool have_deep = deep != nullptr;
    const zoom::Axis ax = zoom::axis(gx, W, r, have_deep);
    for (uint32_t gy = blockIdx.y * 4u + threadIdx.y; gy < H; gy += gridDim.y * 4u) {
        const zoom::Axis ay = zoom::axis(gy, H, r, have_deep);   // (uniform over the wave: threadIdx.y is)
        const bool from_deep = ax.in_deep && ay.in_deep;
        const float4* __restrict__ src = from_deep ? deep : wide;
        const zoom::Tap tx = from_deep ? ax.deep : ax.wide, ty = from_deep ? ay.deep : ay.wide;
        const float4* __restrict__ row0 = src + (size_t)ty.i0 * W;
        const float4* __restrict__ row1 = src + (size_t)ty.i1 * W;
        const float4 a00 = row0[tx.i0], a01 = row0[tx.i1], a10 = row1[tx.i0], a11 = row1[tx.i1];
        float v[4];
        zoom::bilinear(&a00.x, &a01.x, &a10.x, &a11.x, tx.f, ty.f, v);
        const size_t o = (size_t)gy * W + gx;
        if (out_rgba) out_rgba[o] = make_float4(v[0], v[1], v[2], v[3]);
        if (out_u8) out_u8[o] = zoom::rgba8_of(v);
    }
}

// The filtered frame (MC_MANDEL_ZOOM_FILTER_AREA): mandel_zoom_kernel's mapping, a lane owns one output pixel and a wave
// 64 adjacent pixels of a row.  A deep-sourced pixel gathers the nine texels of its box (three rows, three adjacent or identical columns:
// adjacent lanes step by r2 in [1, 2] texels, so a wave's nine gathers touch at most 2 KiB + 32 B of each of three rows and the three
// column gathers of a row share their lines), a wide-sourced pixel the bilinear four.  The column's share (axis_area: both taps and the
// box) is computed once per lane before the row loop.  A wave diverges only where it straddles the deep keyframe's rectangle.
__global__ void __launch_bounds__(256) mandel_zoom_area_kernel(const float4* __restrict__ wide, const float4* __restrict__ deep,
                                                               float4* __restrict__ out_rgba, uint32_t* __restrict__ out_u8, uint32_t W,
                                                               uint32_t H, double r) {
    const uint32_t gx = blockIdx.x * 64u + threadIdx.x;
    if (gx >= W) return;
    const bool have_deep = deep != nullptr;
    const zoom::AxisArea ax = zoom::axis_area(gx, W, r, have_deep);
    for (uint32_t gy = blockIdx.y * 4u + threadIdx.y; gy < H; gy += gridDim.y * 4u) {
        const zoom::AxisArea ay = zoom::axis_area(gy, H, r, have_deep);   // (uniform over the wave: threadIdx.y is)
        float v[4];
        zoom::pixel_area(ax, ay, W, (const float*)wide, (const float*)deep, v);
        const size_t o = (size_t)gy * W + gx;
        if (out_rgba) out_rgba[o] = make_float4(v[0], v[1], v[2], v[3]);
        if (out_u8) out_u8[o] = zoom::rgba8_of(v);
    }
}

}  // namespace

int zoom_check_filter(uint32_t filter, const char* who) {
    if (filter == MC_MANDEL_ZOOM_FILTER_BILINEAR || filter == MC_MANDEL_ZOOM_FILTER_AREA) return MC_OK;
    set_error_detail(std::string(who) + ": filter = " + std::to_string(filter) +
                     " is neither MC_MANDEL_ZOOM_FILTER_BILINEAR (0) nor MC_MANDEL_ZOOM_FILTER_AREA (1)");
    return MC_ERR_INVALID_ARGUMENT;
}

int zoom_check_ratio(double r, const char* who) {
    if (r >= 0.5 && r <= 1.0) return MC_OK;   // (a NaN fails both)
    char buf[160];
    std::snprintf(buf, sizeof buf, "%s: r = %.17g is outside [0.5, 1] (the frame's scale over the wide keyframe's)", who, r);
    set_error_detail(buf);
    return MC_ERR_INVALID_ARGUMENT;
}

namespace {

// What both launchers check before anything runs: the arguments, r, alignment and overlap.
int zoom_check_args(mc_context* ctx, uint32_t W, uint32_t H, const void* d_wide, const void* d_deep, double r, const void* d_rgba_f32,
                    const void* d_rgba8, const char* who) {
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    if (!d_wide) {
        set_error_detail(std::string(who) + ": the wide keyframe is NULL");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (!W || !H) {
        set_error_detail(std::string(who) + ": width and height must be above 0");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (!d_rgba_f32 && !d_rgba8) {
        set_error_detail(std::string(who) + ": at least one output must be given");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (int rc = zoom_check_ratio(r, who)) return rc;
    if (reinterpret_cast<uintptr_t>(d_wide) % 16u || reinterpret_cast<uintptr_t>(d_deep) % 16u || reinterpret_cast<uintptr_t>(d_rgba_f32) % 16u ||
        reinterpret_cast<uintptr_t>(d_rgba8) % 4u) {
        set_error_detail(std::string(who) + ": the keyframes and the vec4 output must be aligned to 16 bytes, the RGBA8 output to 4");
        return MC_ERR_INVALID_ARGUMENT;
    }
    const size_t npix = (size_t)W * H;
    if (zoom_overlaps(d_rgba_f32, npix * 16, d_wide, npix * 16) || zoom_overlaps(d_rgba_f32, npix * 16, d_deep, npix * 16) ||
        zoom_overlaps(d_rgba8, npix * 4, d_wide, npix * 16) || zoom_overlaps(d_rgba8, npix * 4, d_deep, npix * 16) ||
        zoom_overlaps(d_rgba8, npix * 4, d_rgba_f32, npix * 16)) {
        set_error_detail(std::string(who) + ": an output overlaps a keyframe or the other output (a pixel reads its neighbours' texels: "
                         "the frame cannot be composed in place)");
        return MC_ERR_INVALID_ARGUMENT;
    }
    return MC_OK;
}

}  // namespace

int mandelbrot_zoom_launch(mc_context* ctx, uint32_t W, uint32_t H, const void* d_wide, const void* d_deep, double r, void* d_rgba_f32,
                           void* d_rgba8, const char* who, hipStream_t s) {
    if (int rc = zoom_check_args(ctx, W, H, d_wide, d_deep, r, d_rgba_f32, d_rgba8, who)) return rc;
    const dim3 grid((W + 63u) / 64u, std::min<uint32_t>((H + 3u) / 4u, 65535u)), block(64, 4);
    hipLaunchKernelGGL(mandel_zoom_kernel, grid, block, 0, s, (const float4*)d_wide, (const float4*)d_deep, (float4*)d_rgba_f32,
                       (uint32_t*)d_rgba8, W, H, r);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

int mandelbrot_zoom_filtered_launch(mc_context* ctx, uint32_t W, uint32_t H, const void* d_wide, const void* d_deep, double r, uint32_t filter,
                                    void* d_rgba_f32, void* d_rgba8, const char* who, hipStream_t s) {
    if (int rc = zoom_check_args(ctx, W, H, d_wide, d_deep, r, d_rgba_f32, d_rgba8, who)) return rc;
    if (int rc = zoom_check_filter(filter, who)) return rc;
    if (filter == MC_MANDEL_ZOOM_FILTER_BILINEAR) return mandelbrot_zoom_launch(ctx, W, H, d_wide, d_deep, r, d_rgba_f32, d_rgba8, who, s);
    const dim3 grid((W + 63u) / 64u, std::min<uint32_t>((H + 3u) / 4u, 65535u)), block(64, 4);
    hipLaunchKernelGGL(mandel_zoom_area_kernel, grid, block, 0, s, (const float4*)d_wide, (const float4*)d_deep, (float4*)d_rgba_f32,
                       (uint32_t*)d_rgba8, W, H, r);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

}  // namespace mc

using namespace mc;

extern "C" int mc_mandelbrot_zoom_ratio(uint32_t step, uint32_t steps_per_octave, double* r) {
    if (!r) return MC_ERR_INVALID_ARGUMENT;
    if (!steps_per_octave || step > steps_per_octave) {
        set_error_detail("mc_mandelbrot_zoom_ratio: step " + std::to_string(step) + " of " + std::to_string(steps_per_octave) +
                         " steps per octave (0 <= step <= steps_per_octave, steps_per_octave >= 1)");
        return MC_ERR_INVALID_ARGUMENT;
    }
    // (the two ends are exact whatever the libm: a keyframe's own frame must be that keyframe's bits)
    *r = step == 0u ? 1.0 : step == steps_per_octave ? 0.5 : std::exp2(-(double)step / (double)steps_per_octave);
    return MC_OK;
}

namespace {

int zoom_compose_host_call(const char* who, uint32_t width, uint32_t height, const float* wide, const float* deep, double r, uint32_t filter,
                           float* out_rgba_f32, uint8_t* out_rgba8) {
    if (!wide) {
        set_error_detail(std::string(who) + ": the wide keyframe is NULL");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (!width || !height) {
        set_error_detail(std::string(who) + ": width and height must be above 0");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (!out_rgba_f32 && !out_rgba8) {
        set_error_detail(std::string(who) + ": at least one output must be given");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (int rc = zoom_check_ratio(r, who)) return rc;
    if (int rc = zoom_check_filter(filter, who)) return rc;
    if (filter == MC_MANDEL_ZOOM_FILTER_AREA) zoom::compose_area_host(width, height, wide, deep, r, out_rgba_f32, out_rgba8);
    else zoom::compose_host(width, height, wide, deep, r, out_rgba_f32, out_rgba8);
    return MC_OK;
}

}  // namespace

extern "C" {

int mc_mandelbrot_zoom_compose(uint32_t width, uint32_t height, const float* wide, const float* deep, double r, float* out_rgba_f32,
                               uint8_t* out_rgba8) {
    return zoom_compose_host_call("mc_mandelbrot_zoom_compose", width, height, wide, deep, r, MC_MANDEL_ZOOM_FILTER_BILINEAR, out_rgba_f32,
                                  out_rgba8);
}

int mc_mandelbrot_zoom_compose_filtered(uint32_t width, uint32_t height, const float* wide, const float* deep, double r, uint32_t filter,
                                        float* out_rgba_f32, uint8_t* out_rgba8) {
    return zoom_compose_host_call("mc_mandelbrot_zoom_compose_filtered", width, height, wide, deep, r, filter, out_rgba_f32, out_rgba8);
}

int mc_mandelbrot_zoom_compose_device_async(mc_context* ctx, uint32_t width, uint32_t height, const void* d_wide, const void* d_deep, double r,
                                            void* d_rgba_f32, void* d_rgba8, void* stream) {
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    MC_HIP_TRY(hipSetDevice(ctx->device));
    return mandelbrot_zoom_launch(ctx, width, height, d_wide, d_deep, r, d_rgba_f32, d_rgba8, "mc_mandelbrot_zoom_compose_device_async",
                                  stream ? (hipStream_t)stream : ctx->stream);
}

int mc_mandelbrot_zoom_compose_filtered_device_async(mc_context* ctx, uint32_t width, uint32_t height, const void* d_wide, const void* d_deep,
                                                     double r, uint32_t filter, void* d_rgba_f32, void* d_rgba8, void* stream) {
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    MC_HIP_TRY(hipSetDevice(ctx->device));
    return mandelbrot_zoom_filtered_launch(ctx, width, height, d_wide, d_deep, r, filter, d_rgba_f32, d_rgba8,
                                           "mc_mandelbrot_zoom_compose_filtered_device_async", stream ? (hipStream_t)stream : ctx->stream);
}

}  // extern "C"
