// Distance shading of the Mandelbrot image for gfx950 (MI355X): the stencil over the smooth-count plane.  The project's own addition
// (the reference colours by the integer count); contract in include/mc_compute.h, restated in tests/mandel_distance_ref.py; scheme and
// measurements in DESIGN.md §3.15.  The arithmetic is mandel_distance.h, the same source mc_mandelbrot_distance_plane / _colour run.
//
// A memory-bound 5-point stencil: 4 B read and 16 (+ 4) B written per pixel, two 16-B gathers from the L2-resident colour table (the
// smooth colour's a and b), as mandel_recolour_kernel's one.
//  * a lane owns FOUR adjacent pixels of one row; a wave covers 256 pixels of a row, a block (64 x 4) four adjacent rows, so a row read
//    as one lane's "below" is the next wave's centre and comes from the cache.
//  * the centre row's four counts, and those of the rows above and below, are one aligned 16-B vector each where the address allows.  A
//    row does not always start on a 16-B boundary (W not a multiple of four, a caller's offset pointer): such groups are read as two 8-B
//    vectors where those are aligned, else value by value, and so is a row's last, partial group.
//  * the left neighbour of a lane's first pixel and the right neighbour of its last are two 4-B loads of words the neighbouring lanes
//    load as part of their vectors: cache hits, no cross-lane traffic, nothing special at a wave's edge.
//  * the output is the compact rows [row_begin, row_end) of the request: the stencil reads the whole image's plane and the image's
//    borders, not the band's, decide where a difference is one-sided.
// No LDS, no atomics, no synchronisation; vector loads and stores only.
#include <algorithm>
#include <cmath>
#include <vector>

#include "mandel_distance.h"
#include "mandel_distance_host.h"
#include "mandel_resolve_smooth_host.h"
#include "mandel_smooth_equalise_host.h"

namespace mc {

namespace {

constexpr uint32_t kPx = 4u;   // pixels per lane

// Four counts at p into c; only the first `valid` exist (the rest read as 0 and belong to no pixel).
__device__ __forceinline__ void load_counts4(const uint32_t* __restrict__ p, uint32_t valid, uint32_t (&c)[kPx]) {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
    if (valid == kPx && (addr & 15u) == 0u) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        c[0] = q.x; c[1] = q.y; c[2] = q.z; c[3] = q.w;
    } else if (valid == kPx && (addr & 7u) == 0u) {
        const uint2 a = reinterpret_cast<const uint2*>(p)[0], b = reinterpret_cast<const uint2*>(p)[1];
        c[0] = a.x; c[1] = a.y; c[2] = b.x; c[3] = b.y;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < kPx; j++) c[j] = j < valid ? p[j] : 0u;
    }
}

// One lane: kPx adjacent pixels of output row r (storage row row_begin + r); blockIdx.y strides over the rows, four to a block.
// q: the WHOLE image's plane, W x H.  out_d / out_rgba: rows x W, compact; either may be null.  lut: (max_iter + 1) vec4.
__global__ void __launch_bounds__(256) mandel_distance_kernel(const uint32_t* __restrict__ q, const float4* __restrict__ lut,
                                                              float* __restrict__ out_d, float4* __restrict__ out_rgba, uint32_t W,
                                                              uint32_t H, uint32_t row_begin, uint32_t rows, uint32_t max_iter,
                                                              float threshold) {
    const uint32_t groups = (W + kPx - 1u) / kPx;
    const uint32_t g = blockIdx.x * 64u + threadIdx.x;
    if (g >= groups) return;
    const uint32_t x0 = g * kPx;
    const uint32_t npx = W - x0 < kPx ? W - x0 : kPx;
    const uint32_t interior = 256u * max_iter;
    for (uint32_t r = blockIdx.y * 4u + threadIdx.y; r < rows; r += gridDim.y * 4u) {
        const uint32_t y = row_begin + r;
        const bool has_u = y > 0u, has_d = y + 1u < H, has_l = x0 > 0u, has_r = x0 + npx < W;
        const uint32_t* __restrict__ row = q + (size_t)y * W + x0;
        uint32_t c[kPx], up[kPx] = {0u, 0u, 0u, 0u}, dn[kPx] = {0u, 0u, 0u, 0u};
        load_counts4(row, npx, c);
        if (has_u) load_counts4(row - W, npx, up);
        if (has_d) load_counts4(row + W, npx, dn);
        const uint32_t left = has_l ? row[-1] : 0u;
        const uint32_t right = has_r ? row[npx] : 0u;
        float D[kPx];
#pragma unroll
        for (uint32_t k = 0; k < kPx; k++) {
            const bool hl = k > 0u || has_l, hr = k + 1u < npx || has_r;
            const uint32_t l = k > 0u ? c[k > 0u ? k - 1u : 0u] : left;
            const uint32_t rr = k + 1u < kPx && k + 1u < npx ? c[k + 1u < kPx ? k + 1u : 0u] : right;
            D[k] = distance::distance_px(interior, c[k], l, rr, up[k], dn[k], hl, hr, has_u, has_d);
        }
        const size_t o = (size_t)r * W + x0;
        if (out_d) {
            float* __restrict__ d = out_d + o;
            if (npx == kPx && (reinterpret_cast<uintptr_t>(d) & 15u) == 0u) {
                *reinterpret_cast<float4*>(d) = make_float4(D[0], D[1], D[2], D[3]);
            } else {
#pragma unroll
                for (uint32_t k = 0; k < kPx; k++)
                    if (k < npx) d[k] = D[k];
            }
        }
        if (out_rgba) {
#pragma unroll
            for (uint32_t k = 0; k < kPx; k++)
                if (k < npx) {
                    float v[4];
                    distance::distance_colour(c[k], D[k], threshold, max_iter, reinterpret_cast<const float*>(lut), v);
                    out_rgba[o + k] = make_float4(v[0], v[1], v[2], v[3]);
                }
        }
    }
}

int refuse_threshold(const char* who) {
    set_error_detail(std::string(who) + ": MC_MANDEL_COLOUR_DISTANCE: threshold_px must be finite and above 0");
    return MC_ERR_INVALID_ARGUMENT;
}

}  // namespace

int mandelbrot_distance_launch(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_smooth, float threshold_px, void* d_distance,
                               void* d_rgba, const char* who, hipStream_t s) {
    if (!ctx || !p || !d_smooth || (!d_distance && !d_rgba) || !p->height || !p->max_iter || !rows_ok(p)) return MC_ERR_INVALID_ARGUMENT;
    if (int rc = smooth_samples_refuse_flag(p, who)) return rc;
    if (int rc = smooth_equalised_refuse_flag(p, who)) return rc;
    if (!distance_flag(p)) {
        set_error_detail(std::string(who) + ": the params must carry MC_MANDEL_COLOUR_DISTANCE");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (int rc = distance_refuse_combination(p, who)) return rc;
    if (p->row_stride || p->row_block) {
        set_error_detail(std::string(who) + ": MC_MANDEL_COLOUR_DISTANCE: the outputs are contiguous rows [row_begin, row_end); interleaved "
                         "tiles are not offered (band the output with row_begin / row_end)");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (!std::isfinite(threshold_px) || !(threshold_px > 0.0f)) return refuse_threshold(who);
    if (reinterpret_cast<uintptr_t>(d_smooth) % 4u || reinterpret_cast<uintptr_t>(d_distance) % 4u || reinterpret_cast<uintptr_t>(d_rgba) % 16u)
        return MC_ERR_INVALID_ARGUMENT;
    const void* lut = nullptr;
    if (d_rgba)
        if (int rc = mandelbrot_lut_device(ctx, p, s, &lut)) return rc;
    const uint32_t W = p->width, rows = p->row_end - p->row_begin;
    const uint32_t groups = (W + kPx - 1u) / kPx;
    const dim3 grid((groups + 63u) / 64u, std::min<uint32_t>((rows + 3u) / 4u, 65535u)), block(64, 4);
    hipLaunchKernelGGL(mandel_distance_kernel, grid, block, 0, s, (const uint32_t*)d_smooth, (const float4*)lut, (float*)d_distance,
                       (float4*)d_rgba, W, p->height, p->row_begin, rows, p->max_iter, threshold_px);
    MC_HIP_TRY(hipGetLastError());
    return ctx->note_launch(s);   // (reads a cached colour table)
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_mandelbrot_distance_device_async(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_smooth, float threshold_px,
                                        void* d_distance_f32, void* d_rgba_f32, void* stream) {
    if (!ctx || !p || !d_smooth || (!d_distance_f32 && !d_rgba_f32)) return MC_ERR_INVALID_ARGUMENT;
    MC_HIP_TRY(hipSetDevice(ctx->device));
    return mandelbrot_distance_launch(ctx, p, d_smooth, threshold_px, d_distance_f32, d_rgba_f32, "mc_mandelbrot_distance_device_async",
                                      stream ? (hipStream_t)stream : ctx->stream);
}

int mc_mandelbrot_distance_plane(uint32_t width, uint32_t height, uint32_t max_iter, const uint32_t* q, float* out_distance) {
    if (!width || !height || !max_iter || max_iter > smooth::kMaxIter || !q || !out_distance) return MC_ERR_INVALID_ARGUMENT;
    const size_t n = (size_t)width * height;
    for (size_t i = 0; i < n; i++)
        if (q[i] > 256u * max_iter) {
            set_error_detail("mc_mandelbrot_distance_plane: q[" + std::to_string(i) + "] = " + std::to_string(q[i]) + " is above 256 * max_iter");
            return MC_ERR_INVALID_ARGUMENT;
        }
    for (uint32_t y = 0; y < height; y++)
        for (uint32_t x = 0; x < width; x++) out_distance[(size_t)y * width + x] = distance::distance_at(q, width, height, max_iter, y, x);
    return MC_OK;
}

int mc_mandelbrot_distance_colour(uint32_t max_iter, const float k_color[4], const uint32_t* q, const float* distance, uint64_t count,
                                  float threshold_px, float* out_rgba_f32) {
    if (!max_iter || max_iter > smooth::kMaxIter || !k_color || !count || !q || !distance || !out_rgba_f32) return MC_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(threshold_px) || !(threshold_px > 0.0f)) return refuse_threshold("mc_mandelbrot_distance_colour");
    for (uint64_t i = 0; i < count; i++)
        if (q[i] > 256u * max_iter) {
            set_error_detail("mc_mandelbrot_distance_colour: q[" + std::to_string(i) + "] = " + std::to_string(q[i]) + " is above 256 * max_iter");
            return MC_ERR_INVALID_ARGUMENT;
        }
    std::vector<float> lut(((size_t)max_iter + 1) * 4);
    mandelbrot_build_lut(max_iter, k_color, lut.data());
    for (uint64_t i = 0; i < count; i++) distance::distance_colour(q[i], distance[i], threshold_px, max_iter, lut.data(), out_rgba_f32 + 4 * i);
    return MC_OK;
}

}  // extern "C"
