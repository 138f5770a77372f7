// s x s supersampling of the smooth Mandelbrot colourings for gfx950 (MI355X): the resolve over fractional counts, from a plane of
// smooth sample counts to one vec4 per pixel.  The project's own addition; contract in include/mc_compute.h, restated in
// tests/mandel_smooth_supersample_ref.py; scheme and measurements in DESIGN.md §3.25.  The arithmetic is mandel_resolve_smooth.h, the
// same source the host call runs.
//
// The scheme is mandel_resolve.hip's: the sample plane is what the smooth render of the s*W x s*H image writes for the same tile
// (mc_mandelbrot_supersample_params), one dense (rows * s) x (s * W) array of uint32_t, and
//  * a lane owns WHOLE pixels (two at s = 2, one otherwise), so the contract's tree is a fixed expression per lane;
//  * per sample row a lane reads up to 16 B of q as one aligned vector (s = 8: two), as 8-B vectors where only those are aligned, value
//    by value otherwise and in a row's last, partial group; the choice is uniform over a row's full groups;
//  * per sample the lane issues, for the ranked form, one aligned 8-B gather from the pair table and the 40-bit product, then the smooth
//    colour's two 16-B gathers from the L2-resident colour table and the lerp.  q is clamped to 256 M before any index is formed.
//  * a sample costs two or three gathers where the integer resolve costs one, so the sample rows go in chunks of TWO (eight or sixteen
//    samples in flight per lane): tree(r_0 .. r_{2k-1}) is the tree of the chunk sums r_0 + r_1, r_2 + r_3, ...
// No LDS, no atomics, no scratch; vector loads and stores only.
#include <algorithm>
#include <vector>

#include "mandel_distance_host.h"
#include "mandel_equalise.h"
#include "mandel_resolve_smooth.h"
#include "mandel_resolve_smooth_host.h"

namespace mc {

namespace {

using resolve_smooth::Knot;
using resolve_smooth::Rgba;

struct PairsDevice {
    const uint2* __restrict__ p;
    __device__ __forceinline__ Knot operator()(uint32_t j) const {
        const uint2 v = p[j];
        return Knot{v.x, v.y};
    }
};
struct LutDevice {
    const float4* __restrict__ p;
    __device__ __forceinline__ Rgba operator()(uint32_t i) const {
        const float4 v = p[i];
        return Rgba{v.x, v.y, v.z, v.w};
    }
};

// N smooth counts at p into c; only the first `valid` exist (the rest read as 0 and belong to no pixel).
template <int N>
__device__ __forceinline__ void load_smooth(const uint32_t* __restrict__ p, uint32_t valid, uint32_t (&c)[N]) {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
    if (valid == (uint32_t)N && (addr & 15u) == 0u) {
#pragma unroll
        for (int v = 0; v < N / 4; v++) {
            const uint4 q = reinterpret_cast<const uint4*>(p)[v];
            c[4 * v] = q.x; c[4 * v + 1] = q.y; c[4 * v + 2] = q.z; c[4 * v + 3] = q.w;
        }
    } else if (valid == (uint32_t)N && (addr & 7u) == 0u) {
#pragma unroll
        for (int v = 0; v < N / 2; v++) {
            const uint2 q = reinterpret_cast<const uint2*>(p)[v];
            c[2 * v] = q.x; c[2 * v + 1] = q.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < N; j++) c[j] = (uint32_t)j < valid ? p[j] : 0u;
    }
}

// Pixels per lane: 16 B of a sample row's counts, at least one pixel (mandel_resolve.hip's ResolveGroup for uint32_t).
template <int S>
struct SmoothGroup {
    static constexpr int kPixels = S == 2 ? 2 : 1;
};

// One lane: kPixels adjacent pixels of one compact pixel row; blockIdx.y strides over the rows.  pairs: max_iter (knot, step) entries
// (Ranked only); lut: (max_iter + 1) vec4.
template <int S, bool Ranked>
__global__ void __launch_bounds__(256) mandel_resolve_smooth_kernel(const uint32_t* __restrict__ samples, const uint2* __restrict__ pairs,
                                                                    const float4* __restrict__ lut, float4* __restrict__ rgba, uint32_t W,
                                                                    uint32_t rows, uint32_t max_iter) {
    constexpr int kPixels = SmoothGroup<S>::kPixels;
    constexpr int kElems = kPixels * S;   // counts per lane and sample row: 4, 4, 8
    constexpr int kChunk = 2;             // sample rows whose gathers are issued together
    constexpr int kChunks = S / kChunk;   // 1, 2, 4
    const uint32_t groups = (W + (uint32_t)kPixels - 1u) / (uint32_t)kPixels;
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= groups) return;
    const uint32_t x0 = g * (uint32_t)kPixels;
    const uint32_t npx = W - x0 < (uint32_t)kPixels ? W - x0 : (uint32_t)kPixels;
    const size_t pitch = (size_t)S * W;   // counts per sample row
    const float inv = 1.0f / (float)(S * S);
    const PairsDevice pd{pairs};
    const LutDevice ld{lut};
    for (uint32_t y = blockIdx.y; y < rows; y += gridDim.y) {
        const uint32_t* __restrict__ first = samples + (size_t)y * S * pitch + (size_t)x0 * S;
        // the sum of chunk h's two sample rows, per pixel
        auto chunk = [&](int h, Rgba (&p)[kPixels]) {
            Rgba r[kPixels][kChunk];
#pragma unroll
            for (int i = 0; i < kChunk; i++) {
                uint32_t c[kElems];
                load_smooth<kElems>(first + (size_t)(h * kChunk + i) * pitch, npx * (uint32_t)S, c);
#pragma unroll
                for (int k = 0; k < kPixels; k++) {
                    Rgba a[S];
#pragma unroll
                    for (int j = 0; j < S; j++) a[j] = resolve_smooth::sample_colour<Ranked>(c[k * S + j], max_iter, pd, ld);
                    r[k][i] = resolve_smooth::tree<S>(a);
                }
            }
#pragma unroll
            for (int k = 0; k < kPixels; k++) p[k] = resolve_smooth::tree<kChunk>(r[k]);
        };
        // tree(r_0 .. r_{S-1}) over the chunk sums: one chunk (s = 2), p_0 + p_1 (s = 4), (p_0 + p_1) + (p_2 + p_3) (s = 8); the loops are
        // kept rolled so that no more than one chunk's gathers are in flight
        Rgba t[kPixels];
        if constexpr (kChunks == 1) {
            chunk(0, t);
        } else {
#pragma unroll 1
            for (int hi = 0; hi < kChunks / 2; hi++) {
                Rgba u[kPixels];
#pragma unroll 1
                for (int lo = 0; lo < 2; lo++) {
                    Rgba p[kPixels];
                    chunk(2 * hi + lo, p);
#pragma unroll
                    for (int k = 0; k < kPixels; k++) u[k] = lo == 0 ? p[k] : resolve_smooth::add(u[k], p[k]);
                }
#pragma unroll
                for (int k = 0; k < kPixels; k++) t[k] = hi == 0 ? u[k] : resolve_smooth::add(t[k], u[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < kPixels; k++)
            if ((uint32_t)k < npx) {
                const Rgba o = resolve_smooth::scale(t[k], inv);
                rgba[(size_t)y * W + x0 + (uint32_t)k] = make_float4(o.r, o.g, o.b, o.a);
            }
    }
}

template <int S, bool Ranked>
void resolve_smooth_launch(const void* d_smooth, const void* pairs, const void* lut, void* d_rgba, uint32_t W, uint32_t rows,
                           uint32_t max_iter, hipStream_t s) {
    constexpr uint32_t kPixels = (uint32_t)SmoothGroup<S>::kPixels;
    const uint32_t groups = (W + kPixels - 1u) / kPixels;
    const dim3 grid((groups + 255u) / 256u, std::min<uint32_t>(rows, 65535u)), block(256);
    hipLaunchKernelGGL((mandel_resolve_smooth_kernel<S, Ranked>), grid, block, 0, s, (const uint32_t*)d_smooth, (const uint2*)pairs,
                       (const float4*)lut, (float4*)d_rgba, W, rows, max_iter);
}

template <bool Ranked>
void resolve_smooth_launch(uint32_t f, const void* d_smooth, const void* pairs, const void* lut, void* d_rgba, uint32_t W, uint32_t rows,
                           uint32_t max_iter, hipStream_t s) {
    if (f == 2u) resolve_smooth_launch<2, Ranked>(d_smooth, pairs, lut, d_rgba, W, rows, max_iter, s);
    else if (f == 4u) resolve_smooth_launch<4, Ranked>(d_smooth, pairs, lut, d_rgba, W, rows, max_iter, s);
    else resolve_smooth_launch<8, Ranked>(d_smooth, pairs, lut, d_rgba, W, rows, max_iter, s);
}

}  // namespace

int mandelbrot_resolve_smooth_launch(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_smooth, const uint32_t* qmap, void* d_rgba,
                                     const char* who, hipStream_t s) {
    if (!ctx || !p || !d_smooth || !d_rgba || !p->max_iter || !rows_ok(p)) return MC_ERR_INVALID_ARGUMENT;
    if (int rc = adaptive_smooth_refuse_flag(p, who)) return rc;   // (this stage resolves a FULL sample plane)
    if (!smooth_samples_flag(p)) {
        set_error_detail(std::string(who) + ": the params must carry MC_MANDEL_SUPERSAMPLE_SMOOTH");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (int rc = smooth_samples_check(p, who)) return rc;
    const bool ranked = smooth_equalised_flag(p);
    if (ranked != (qmap != nullptr)) {
        set_error_detail(std::string(who) + ": MC_MANDEL_SUPERSAMPLE_SMOOTH: qmap is given exactly when the params carry "
                         "MC_MANDEL_COLOUR_SMOOTH_EQUALISED");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (p->row_stride && (!p->row_block || p->row_block > p->row_stride)) return MC_ERR_INVALID_ARGUMENT;
    const uint32_t f = (p->flags >> 8) & 15u, W = p->width, M = p->max_iter;
    if ((uint64_t)W * f > 0xffffffffull) return MC_ERR_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(d_smooth) % 4u || reinterpret_cast<uintptr_t>(d_rgba) % 16u) return MC_ERR_INVALID_ARGUMENT;
    const void* pairs = nullptr;
    if (ranked) {
        if (int rc = smooth_equalise_check_knots(M, qmap, who)) return rc;
        if (int rc = smooth_equalise_pairs_device(ctx, M, qmap, s, &pairs)) return rc;
    }
    const void* lut = nullptr;
    if (int rc = mandelbrot_lut_device(ctx, p, s, &lut)) return rc;
    const uint32_t rows = tile_rows(p->row_begin, p->row_end, p->row_stride ? p->row_block : 0u, p->row_stride);
    if (ranked) resolve_smooth_launch<true>(f, d_smooth, pairs, lut, d_rgba, W, rows, M, s);
    else resolve_smooth_launch<false>(f, d_smooth, pairs, lut, d_rgba, W, rows, M, s);
    MC_HIP_TRY(hipGetLastError());
    return ctx->note_launch(s);   // (reads the cached pair and colour tables)
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_mandelbrot_resolve_smooth_device_async(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_smooth, const uint32_t* qmap,
                                              void* d_rgba_f32, void* stream) {
    if (!ctx || !p || !d_smooth || !d_rgba_f32 || !p->max_iter) return MC_ERR_INVALID_ARGUMENT;
    MC_HIP_TRY(hipSetDevice(ctx->device));
    return mandelbrot_resolve_smooth_launch(ctx, p, d_smooth, qmap, d_rgba_f32, "mc_mandelbrot_resolve_smooth_device_async",
                                            stream ? (hipStream_t)stream : ctx->stream);
}

int mc_mandelbrot_resolve_smooth(uint32_t max_iter, const float k_color[4], uint32_t s, uint32_t width, uint32_t rows, const uint32_t* q,
                                 const uint32_t* qmap, float* out_rgba_f32) {
    if (!max_iter || max_iter > kSmoothMaxIter || !k_color || !width || !rows || !q || !out_rgba_f32) return MC_ERR_INVALID_ARGUMENT;
    if (s != 2u && s != 4u && s != 8u) {
        set_error_detail("mc_mandelbrot_resolve_smooth: the factor is 2, 4 or 8");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if ((uint64_t)width * s > 0xffffffffull || (uint64_t)rows * s > 0xffffffffull) return MC_ERR_INVALID_ARGUMENT;
    if (qmap)
        if (int rc = smooth_equalise_check_knots(max_iter, qmap, "mc_mandelbrot_resolve_smooth")) return rc;
    const uint64_t count = (uint64_t)width * rows * s * s;
    for (uint64_t i = 0; i < count; i++)
        if (q[i] > 256u * max_iter) {
            set_error_detail("mc_mandelbrot_resolve_smooth: q[" + std::to_string(i) + "] = " + std::to_string(q[i]) + " is above 256 * max_iter");
            return MC_ERR_INVALID_ARGUMENT;
        }
    std::vector<float> lut(((size_t)max_iter + 1) * 4);
    mandelbrot_build_lut(max_iter, k_color, lut.data());
    std::vector<uint32_t> pairs;
    if (qmap) {
        pairs.resize((size_t)max_iter * 2);
        smooth_equalise::compose_pairs(max_iter, qmap, pairs.data());
    }
    resolve_smooth::resolve_plane(s, max_iter, width, rows, q, qmap ? pairs.data() : nullptr, lut.data(), out_rgba_f32);
    return MC_OK;
}

}  // extern "C"
