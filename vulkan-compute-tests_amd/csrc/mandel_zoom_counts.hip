// Zoom sequences of the Mandelbrot image from COUNT keyframes for gfx950 (MI355X): a frame composed from the two count planes that bracket
// it, coloured through ONE map that moves with the zoom.  The project's own addition; contract in include/mc_compute.h, restated in
// tests/mandel_zoom_counts_ref.py; scheme and measurements in DESIGN.md §3.22.  The arithmetic is mandel_zoom_counts.h, the same source
// mc_mandelbrot_zoom_compose_counts runs on the host.
//
// The compose kernel keeps mandel_zoom_kernel's mapping: a lane owns ONE output pixel, a wave 64 adjacent pixels of a row, a block (64 x 4)
// four adjacent rows, blockIdx.y strides over the rows; the column's share of the geometry is computed once per lane, the keyframe is
// chosen by a select of pointer and taps.  A tap is a 4-B load and then dependent gathers from tables that stay in L2 (16 B x (M + 1)):
// the four count loads are issued together, then the gathers of all four taps together (zoom_counts::tap_colours forms every index before
// it loads): one rgb gather per tap for plain and equalised, two for smooth, an 8-B pair and then the two for smooth equalised.
// The table kernel builds the frame's table from the two keyframes' maps, one thread per entry.
// No LDS, no atomics, no synchronisation; vector loads and stores only.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "mandel_distance_host.h"
#include "mandel_equalise.h"
#include "mandel_resolve_smooth_host.h"
#include "mandel_smooth_equalise_host.h"
#include "mandel_zoom_counts.h"
#include "mandel_zoom_counts_host.h"

namespace mc {

namespace {

// wide, deep (or null): W x H uint32_t.  out_rgba (vec4) / out_u8 (packed RGBA8): W x H; either may be null.
template <int kMode>
__global__ void __launch_bounds__(256) mandel_zoom_counts_kernel(const uint32_t* __restrict__ wide, const uint32_t* __restrict__ deep,
                                                                 const float* __restrict__ table, const uint32_t* __restrict__ pairs,
                                                                 float4* __restrict__ out_rgba, uint32_t* __restrict__ out_u8, uint32_t W,
                                                                 uint32_t H, uint32_t M, double r) {
    const uint32_t gx = blockIdx.x * 64u + threadIdx.x;
    if (gx >= W) return;
    const bool have_deep = deep != nullptr;
    const zoom::Axis ax = zoom::axis(gx, W, r, have_deep);
    for (uint32_t gy = blockIdx.y * 4u + threadIdx.y; gy < H; gy += gridDim.y * 4u) {
        const zoom::Axis ay = zoom::axis(gy, H, r, have_deep);   // (uniform over the wave: threadIdx.y is)
        float v[4];
        zoom_counts::pixel<kMode>(ax, ay, W, M, wide, deep, table, pairs, v);
        const size_t o = (size_t)gy * W + gx;
        if (out_rgba) out_rgba[o] = make_float4(v[0], v[1], v[2], v[3]);
        if (out_u8) out_u8[o] = zoom::rgba8_of(v);
    }
}

// Equalised: out4[j] = lut[blend(map_wide[j], map_deep[j])], j <= M.  SmoothEqualised: out2[j] = (knot_j, knot_{j+1} - knot_j), j < M.
// A blended entry above the table's top (maps the sequence did not build itself) is taken as the top.
template <int kMode>
__global__ void __launch_bounds__(256) mandel_zoom_table_kernel(const uint32_t* __restrict__ map_wide, const uint32_t* __restrict__ map_deep,
                                                                const float4* __restrict__ lut, float4* __restrict__ out4,
                                                                uint2* __restrict__ out2, uint32_t M, uint32_t step, uint32_t steps) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (kMode == zoom_counts::Equalised) {
        if (j > M) return;
        const uint32_t m = zoom_counts::blend(map_wide[j], map_deep[j], step, steps);
        out4[j] = lut[m < M ? m : M];
    } else {
        if (j >= M) return;
        const uint32_t top = 256u * M;
        uint32_t k0 = zoom_counts::blend(map_wide[j], map_deep[j], step, steps);
        uint32_t k1 = zoom_counts::blend(map_wide[j + 1u], map_deep[j + 1u], step, steps);
        k0 = k0 < top ? k0 : top;
        k1 = k1 < top ? k1 : top;
        out2[j] = make_uint2(k0, k1 > k0 ? k1 - k0 : 0u);
    }
}

// The filtered frame (MC_MANDEL_ZOOM_FILTER_AREA): the same mapping.  A deep-sourced pixel loads the nine counts of its box
// together, then the gathers of all nine taps together (zoom_counts::tap_colours9), then zoom::area; a wide-sourced pixel is the four-tap
// pixel of the kernel above.
template <int kMode>
__global__ void __launch_bounds__(256) mandel_zoom_counts_area_kernel(const uint32_t* __restrict__ wide, const uint32_t* __restrict__ deep,
                                                                      const float* __restrict__ table, const uint32_t* __restrict__ pairs,
                                                                      float4* __restrict__ out_rgba, uint32_t* __restrict__ out_u8,
                                                                      uint32_t W, uint32_t H, uint32_t M, double r) {
    const uint32_t gx = blockIdx.x * 64u + threadIdx.x;
    if (gx >= W) return;
    const bool have_deep = deep != nullptr;
    const zoom::AxisArea ax = zoom::axis_area(gx, W, r, have_deep);
    for (uint32_t gy = blockIdx.y * 4u + threadIdx.y; gy < H; gy += gridDim.y * 4u) {
        const zoom::AxisArea ay = zoom::axis_area(gy, H, r, have_deep);   // (uniform over the wave: threadIdx.y is)
        float v[4];
        zoom_counts::pixel_area<kMode>(ax, ay, W, M, wide, deep, table, pairs, v);
        const size_t o = (size_t)gy * W + gx;
        if (out_rgba) out_rgba[o] = make_float4(v[0], v[1], v[2], v[3]);
        if (out_u8) out_u8[o] = zoom::rgba8_of(v);
    }
}

int refuse(const char* who, const std::string& what) {
    set_error_detail(std::string(who) + ": " + what);
    return MC_ERR_INVALID_ARGUMENT;
}

}  // namespace

int zoom_counts_mode(const mc_mandelbrot_params* p, const char* who, int* mode) {
    if (!p || !mode) return MC_ERR_INVALID_ARGUMENT;
    if (!p->width || !p->height) return refuse(who, "width and height must be above 0");
    if (!p->max_iter || p->max_iter == 0xffffffffu) return refuse(who, "max_iter must be above 0 and below 2^32 - 1 (the tables have max_iter + 1 entries)");
    if (!whole_image(p) || p->row_block) return refuse(who, "a count keyframe is a whole image (row_begin = 0, row_end = height, no interleave)");
    if (p->flags & MC_MANDEL_ITERS_U16) return refuse(who, "MC_MANDEL_ITERS_U16: a count keyframe is a plane of uint32_t");
    if (p->flags & MC_MANDEL_COLOUR_DISTANCE)
        return refuse(who, "MC_MANDEL_COLOUR_DISTANCE shades by a stencil over a whole smooth plane: a count keyframe cannot carry it (the vec4 "
                           "sequence, mc_mandelbrot_zoom_push, does)");
    if (int rc = smooth_samples_refuse_flag(p, who)) return rc;
    if ((p->flags & MC_MANDEL_SUPERSAMPLE_ADAPTIVE) || ((p->flags >> 8) & 15u) > 1u)
        return refuse(who, "MC_MANDEL_SUPERSAMPLE / MC_MANDEL_SUPERSAMPLE_ADAPTIVE: a supersampled pixel has no single count (the vec4 sequence, "
                           "mc_mandelbrot_zoom_push, takes such keyframes)");
    if (p->flags & MC_MANDEL_FMA) return refuse(who, "MC_MANDEL_FMA (the contraction switch measures the plain fp32 render only)");
    const uint32_t colour = p->flags & (uint32_t)(MC_MANDEL_COLOUR_EQUALISED | MC_MANDEL_COLOUR_SMOOTH | MC_MANDEL_COLOUR_SMOOTH_EQUALISED);
    if (colour & (colour - 1u))
        return refuse(who, "more than one colouring (exactly one of plain, MC_MANDEL_COLOUR_EQUALISED, MC_MANDEL_COLOUR_SMOOTH, "
                           "MC_MANDEL_COLOUR_SMOOTH_EQUALISED)");
    *mode = colour == MC_MANDEL_COLOUR_EQUALISED          ? zoom_counts::Equalised
            : colour == MC_MANDEL_COLOUR_SMOOTH           ? zoom_counts::Smooth
            : colour == MC_MANDEL_COLOUR_SMOOTH_EQUALISED ? zoom_counts::SmoothEqualised
                                                          : zoom_counts::Plain;
    if (*mode >= zoom_counts::Smooth && p->max_iter > kSmoothMaxIter)
        return refuse(who, "the smooth colourings need max_iter <= 2^24 - 1 (the smooth plane is 24.8 fixed point)");
    return MC_OK;
}

int zoom_counts_check_args(uint32_t W, uint32_t H, const void* d_wide, const void* d_deep, double r, const void* d_rgba_f32, const void* d_rgba8,
                           const char* who) {
    if (!d_wide) return refuse(who, "the wide keyframe is NULL");
    if (!W || !H) return refuse(who, "width and height must be above 0");
    if (!d_rgba_f32 && !d_rgba8) return refuse(who, "at least one output must be given");
    if (int rc = zoom_check_ratio(r, who)) return rc;
    if (reinterpret_cast<uintptr_t>(d_wide) % 4u || reinterpret_cast<uintptr_t>(d_deep) % 4u || reinterpret_cast<uintptr_t>(d_rgba_f32) % 16u ||
        reinterpret_cast<uintptr_t>(d_rgba8) % 4u)
        return refuse(who, "the keyframes and the RGBA8 output must be aligned to 4 bytes, the vec4 output to 16");
    const size_t npix = (size_t)W * H;
    if (zoom_overlaps(d_rgba_f32, npix * 16, d_wide, npix * 4) || zoom_overlaps(d_rgba_f32, npix * 16, d_deep, npix * 4) ||
        zoom_overlaps(d_rgba8, npix * 4, d_wide, npix * 4) || zoom_overlaps(d_rgba8, npix * 4, d_deep, npix * 4) ||
        zoom_overlaps(d_rgba8, npix * 4, d_rgba_f32, npix * 16))
        return refuse(who, "an output overlaps a keyframe or the other output (a pixel reads its neighbours' counts: the frame cannot be "
                           "composed in place)");
    return MC_OK;
}

int mandelbrot_zoom_counts_launch(mc_context* ctx, uint32_t W, uint32_t H, uint32_t max_iter, int mode, const void* d_wide, const void* d_deep,
                                  const void* d_table, const void* d_pairs, double r, void* d_rgba_f32, void* d_rgba8, const char* who,
                                  hipStream_t s) {
    if (!ctx || !d_table || !max_iter || (mode == zoom_counts::SmoothEqualised && !d_pairs)) return MC_ERR_INVALID_ARGUMENT;
    if (int rc = zoom_counts_check_args(W, H, d_wide, d_deep, r, d_rgba_f32, d_rgba8, who)) return rc;
    const dim3 grid((W + 63u) / 64u, std::min<uint32_t>((H + 3u) / 4u, 65535u)), block(64, 4);
#define MC_ZOOM_COUNTS_LAUNCH(kMode)                                                                                                       \
    hipLaunchKernelGGL(mandel_zoom_counts_kernel<kMode>, grid, block, 0, s, (const uint32_t*)d_wide, (const uint32_t*)d_deep,                \
                       (const float*)d_table, (const uint32_t*)d_pairs, (float4*)d_rgba_f32, (uint32_t*)d_rgba8, W, H, max_iter, r)
    switch (mode) {
        case zoom_counts::Plain: MC_ZOOM_COUNTS_LAUNCH(zoom_counts::Plain); break;
        case zoom_counts::Equalised: MC_ZOOM_COUNTS_LAUNCH(zoom_counts::Equalised); break;
        case zoom_counts::Smooth: MC_ZOOM_COUNTS_LAUNCH(zoom_counts::Smooth); break;
        case zoom_counts::SmoothEqualised: MC_ZOOM_COUNTS_LAUNCH(zoom_counts::SmoothEqualised); break;
        default: return MC_ERR_INVALID_ARGUMENT;
    }
#undef MC_ZOOM_COUNTS_LAUNCH
    MC_HIP_TRY(hipGetLastError());
    return ctx->note_launch(s);   // (reads the cached colour, composed or pair table)
}

int mandelbrot_zoom_table_launch(mc_context* ctx, uint32_t max_iter, int mode, const void* d_map_wide, const void* d_map_deep, uint32_t step,
                                 uint32_t steps_per_octave, const void* d_lut, void* d_out, hipStream_t s) {
    if (!ctx || !max_iter || max_iter == 0xffffffffu || !d_map_wide || !d_map_deep || !d_out || !steps_per_octave || step > steps_per_octave)
        return MC_ERR_INVALID_ARGUMENT;
    const uint32_t* mw = (const uint32_t*)d_map_wide;
    const uint32_t* md = (const uint32_t*)d_map_deep;
    if (mode == zoom_counts::Equalised) {
        if (!d_lut) return MC_ERR_INVALID_ARGUMENT;
        const uint32_t blocks = (uint32_t)(((uint64_t)max_iter + 1u + 255u) / 256u);
        hipLaunchKernelGGL(mandel_zoom_table_kernel<zoom_counts::Equalised>, dim3(blocks), dim3(256), 0, s, mw, md, (const float4*)d_lut,
                           (float4*)d_out, (uint2*)nullptr, max_iter, step, steps_per_octave);
    } else if (mode == zoom_counts::SmoothEqualised) {
        const uint32_t blocks = (uint32_t)(((uint64_t)max_iter + 255u) / 256u);
        hipLaunchKernelGGL(mandel_zoom_table_kernel<zoom_counts::SmoothEqualised>, dim3(blocks), dim3(256), 0, s, mw, md, (const float4*)nullptr,
                           (float4*)nullptr, (uint2*)d_out, max_iter, step, steps_per_octave);
    } else {
        return MC_ERR_INVALID_ARGUMENT;
    }
    MC_HIP_TRY(hipGetLastError());
    return ctx->note_launch(s);   // (reads the cached colour table)
}

int mandelbrot_zoom_counts_filtered_launch(mc_context* ctx, uint32_t W, uint32_t H, uint32_t max_iter, int mode, const void* d_wide,
                                           const void* d_deep, const void* d_table, const void* d_pairs, double r, uint32_t filter,
                                           void* d_rgba_f32, void* d_rgba8, const char* who, hipStream_t s) {
    if (!ctx || !d_table || !max_iter || (mode == zoom_counts::SmoothEqualised && !d_pairs)) return MC_ERR_INVALID_ARGUMENT;
    if (int rc = zoom_counts_check_args(W, H, d_wide, d_deep, r, d_rgba_f32, d_rgba8, who)) return rc;
    if (int rc = zoom_check_filter(filter, who)) return rc;
    if (filter == MC_MANDEL_ZOOM_FILTER_BILINEAR)
        return mandelbrot_zoom_counts_launch(ctx, W, H, max_iter, mode, d_wide, d_deep, d_table, d_pairs, r, d_rgba_f32, d_rgba8, who, s);
    const dim3 grid((W + 63u) / 64u, std::min<uint32_t>((H + 3u) / 4u, 65535u)), block(64, 4);
#define MC_ZOOM_COUNTS_AREA_LAUNCH(kMode)                                                                                                  \
    hipLaunchKernelGGL(mandel_zoom_counts_area_kernel<kMode>, grid, block, 0, s, (const uint32_t*)d_wide, (const uint32_t*)d_deep,           \
                       (const float*)d_table, (const uint32_t*)d_pairs, (float4*)d_rgba_f32, (uint32_t*)d_rgba8, W, H, max_iter, r)
    switch (mode) {
        case zoom_counts::Plain: MC_ZOOM_COUNTS_AREA_LAUNCH(zoom_counts::Plain); break;
        case zoom_counts::Equalised: MC_ZOOM_COUNTS_AREA_LAUNCH(zoom_counts::Equalised); break;
        case zoom_counts::Smooth: MC_ZOOM_COUNTS_AREA_LAUNCH(zoom_counts::Smooth); break;
        case zoom_counts::SmoothEqualised: MC_ZOOM_COUNTS_AREA_LAUNCH(zoom_counts::SmoothEqualised); break;
        default: return MC_ERR_INVALID_ARGUMENT;
    }
#undef MC_ZOOM_COUNTS_AREA_LAUNCH
    MC_HIP_TRY(hipGetLastError());
    return ctx->note_launch(s);   // (reads the cached colour, composed or pair table)
}

}  // namespace mc

using namespace mc;

namespace {

// A caller's map against the colouring: none for plain and smooth, one for the two equalised colourings; a rank map's entries at most
// max_iter (as mc_mandelbrot_recolour_device_async checks), a knot map as mc_mandelbrot_smooth_remap checks its own.
int check_map(const mc_mandelbrot_params* p, int mode, const uint32_t* map, const char* who) {
    const bool wanted = mode == zoom_counts::Equalised || mode == zoom_counts::SmoothEqualised;
    if (!wanted && map) return refuse(who, "a map was given, but the plain and the smooth colouring take none");
    if (wanted && !map) return refuse(who, "the equalised colourings need a map of max_iter + 1 entries (mc_mandelbrot_equalise_map, "
                                           "mc_mandelbrot_smooth_equalise_map or mc_mandelbrot_zoom_blend_map)");
    if (mode == zoom_counts::Equalised) {
        for (uint64_t j = 0; j <= p->max_iter; j++)
            if (map[j] > p->max_iter) return refuse(who, "a map entry exceeds max_iter");
    }
    if (mode == zoom_counts::SmoothEqualised) return smooth_equalise_check_knots(p->max_iter, map, who);
    return MC_OK;
}

int compose_counts_host_call(const char* who, const mc_mandelbrot_params* p, const uint32_t* wide, const uint32_t* deep, const uint32_t* map,
                             double r, uint32_t filter, float* out_rgba_f32, uint8_t* out_rgba8);
int compose_counts_device_call(const char* who, mc_context* ctx, const mc_mandelbrot_params* p, const void* d_wide, const void* d_deep,
                               const uint32_t* map, double r, uint32_t filter, void* d_rgba_f32, void* d_rgba8, void* stream);

}  // namespace

extern "C" {

int mc_mandelbrot_zoom_blend_map(uint32_t entries, const uint32_t* map_wide, const uint32_t* map_deep, uint32_t step, uint32_t steps_per_octave,
                                 uint32_t* out) {
    const char* who = "mc_mandelbrot_zoom_blend_map";
    if (entries && (!map_wide || !map_deep || !out)) return MC_ERR_INVALID_ARGUMENT;
    if (!steps_per_octave || step > steps_per_octave)
        return refuse(who, "step " + std::to_string(step) + " of " + std::to_string(steps_per_octave) +
                               " steps per octave (0 <= step <= steps_per_octave, steps_per_octave >= 1)");
    for (uint32_t j = 0; j < entries; j++)
        if (map_wide[j] > zoom_counts::kBlendMax || map_deep[j] > zoom_counts::kBlendMax)
            return refuse(who, "entry " + std::to_string(j) + " is above 256 * (2^24 - 1)");
    for (uint32_t j = 0; j < entries; j++) out[j] = zoom_counts::blend(map_wide[j], map_deep[j], step, steps_per_octave);
    return MC_OK;
}

int mc_mandelbrot_zoom_compose_counts(const mc_mandelbrot_params* p, const uint32_t* wide, const uint32_t* deep, const uint32_t* map, double r,
                                      float* out_rgba_f32, uint8_t* out_rgba8) {
    return compose_counts_host_call("mc_mandelbrot_zoom_compose_counts", p, wide, deep, map, r, MC_MANDEL_ZOOM_FILTER_BILINEAR, out_rgba_f32,
                                    out_rgba8);
}

int mc_mandelbrot_zoom_compose_counts_filtered(const mc_mandelbrot_params* p, const uint32_t* wide, const uint32_t* deep, const uint32_t* map,
                                               double r, uint32_t filter, float* out_rgba_f32, uint8_t* out_rgba8) {
    return compose_counts_host_call("mc_mandelbrot_zoom_compose_counts_filtered", p, wide, deep, map, r, filter, out_rgba_f32, out_rgba8);
}

int mc_mandelbrot_zoom_compose_counts_device_async(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_wide, const void* d_deep,
                                                   const uint32_t* map, double r, void* d_rgba_f32, void* d_rgba8, void* stream) {
    return compose_counts_device_call("mc_mandelbrot_zoom_compose_counts_device_async", ctx, p, d_wide, d_deep, map, r,
                                      MC_MANDEL_ZOOM_FILTER_BILINEAR, d_rgba_f32, d_rgba8, stream);
}

int mc_mandelbrot_zoom_compose_counts_filtered_device_async(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_wide,
                                                            const void* d_deep, const uint32_t* map, double r, uint32_t filter,
                                                            void* d_rgba_f32, void* d_rgba8, void* stream) {
    return compose_counts_device_call("mc_mandelbrot_zoom_compose_counts_filtered_device_async", ctx, p, d_wide, d_deep, map, r, filter,
                                      d_rgba_f32, d_rgba8, stream);
}

}  // extern "C"

namespace {

int compose_counts_host_call(const char* who, const mc_mandelbrot_params* p, const uint32_t* wide, const uint32_t* deep, const uint32_t* map,
                             double r, uint32_t filter, float* out_rgba_f32, uint8_t* out_rgba8) {
    int mode = 0;
    if (int rc = zoom_counts_mode(p, who, &mode)) return rc;
    if (!wide) return refuse(who, "the wide keyframe is NULL");
    if (!out_rgba_f32 && !out_rgba8) return refuse(who, "at least one output must be given");
    if (int rc = zoom_check_ratio(r, who)) return rc;
    if (int rc = check_map(p, mode, map, who)) return rc;
    if (int rc = zoom_check_filter(filter, who)) return rc;
    const uint32_t M = p->max_iter;
    const size_t npix = (size_t)p->width * p->height;
    if (mode >= zoom_counts::Smooth)
        for (const uint32_t* plane : {wide, deep})
            for (size_t i = 0; plane && i < npix; i++)
                if (plane[i] > 256u * M)
                    return refuse(who, std::string(plane == wide ? "wide" : "deep") + "[" + std::to_string(i) + "] = " + std::to_string(plane[i]) +
                                           " is above 256 * max_iter");
    std::vector<float> lut(((size_t)M + 1) * 4);
    mandelbrot_build_lut(M, p->k_color, lut.data());
    if (filter == MC_MANDEL_ZOOM_FILTER_AREA)
        zoom_counts::compose_counts_area_host(p->width, p->height, M, mode, wide, deep, lut.data(), map, r, out_rgba_f32, out_rgba8);
    else
        zoom_counts::compose_counts_host(p->width, p->height, M, mode, wide, deep, lut.data(), map, r, out_rgba_f32, out_rgba8);
    return MC_OK;
}

int compose_counts_device_call(const char* who, mc_context* ctx, const mc_mandelbrot_params* p, const void* d_wide, const void* d_deep,
                               const uint32_t* map, double r, uint32_t filter, void* d_rgba_f32, void* d_rgba8, void* stream) {
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    int mode = 0;
    if (int rc = zoom_counts_mode(p, who, &mode)) return rc;
    if (int rc = zoom_counts_check_args(p->width, p->height, d_wide, d_deep, r, d_rgba_f32, d_rgba8, who)) return rc;
    if (int rc = check_map(p, mode, map, who)) return rc;
    if (int rc = zoom_check_filter(filter, who)) return rc;
    MC_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const void* table = nullptr;
    const void* pairs = nullptr;
    if (mode == zoom_counts::Equalised) {
        if (int rc = mandelbrot_composed_table(ctx, p, map, who, s, &table)) return rc;
    } else {
        if (int rc = mandelbrot_lut_device(ctx, p, s, &table)) return rc;
        if (mode == zoom_counts::SmoothEqualised)
            if (int rc = smooth_equalise_pairs_device(ctx, p->max_iter, map, s, &pairs)) return rc;
    }
    return mandelbrot_zoom_counts_filtered_launch(ctx, p->width, p->height, p->max_iter, mode, d_wide, d_deep, table, pairs, r, filter, d_rgba_f32,
                                                  d_rgba8, who, s);
}

}  // namespace
