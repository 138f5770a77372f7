// s x s supersampling of the Mandelbrot image for gfx950 (MI355X): the resolve step, from a plane of sample counts to one vec4 per pixel.
// The project's own addition (the reference takes one sample per pixel, at its corner: mandelbrot.comp:29-30); contract in
// include/mc_compute.h, restated in tests/mandel_supersample_ref.py; scheme and measurements in DESIGN.md §3.11.
//
// The sample plane is what the plain render of the s*W x s*H image writes for the same tile (mc_mandelbrot_supersample_params): compact
// pixel row y owns the compact sample rows s*y .. s*y + s - 1, contiguous or interleaved tiles alike, so the kernel sees one dense
// (rows * s) x (s * W) array of counts and nothing of the tiling.
//  * a lane owns WHOLE pixels: the contract's order of additions (adjacent pairs, level by level, first inside a sample row, then over the
//    rows) is a fixed expression tree per pixel and costs no cross-lane traffic.
//  * per sample row a lane reads up to 16 B of counts — one or two pixels (s = 8 / uint32_t: one pixel, two vectors; s = 2 / uint16_t: two
//    pixels, 8 B) — as one aligned vector where the address allows.  A sample row of s * W counts does not always start on a 16-B
//    boundary (odd W with s = 2, uint16_t counts, a caller's offset pointer): such rows are read as 8-B vectors where those are aligned,
//    else value by value, and so is a row's last, partial group.  The choice is per (lane, sample row) and uniform over a row's full groups.
//  * every count is one 16-B gather from the (possibly composed) colour table, the gather mandel_recolour_kernel does; the table is
//    L2-resident (800 KB at M = 50 000).  No LDS, no atomics, vector loads and stores only.
#include <algorithm>

#include "mandel_equalise.h"
#include "mandel_distance_host.h"
#include "mandel_resolve_smooth_host.h"
#include "mandel_smooth_equalise_host.h"
#include "mandel_smooth_host.h"

namespace mc {

namespace {

__device__ __forceinline__ float4 add4(const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// tree(a_0 .. a_{K-1}) of the contract, K a power of two: sums of adjacent pairs, level by level — the balanced binary tree.
template <int K>
__device__ __forceinline__ float4 tree(const float4* a) {
    if constexpr (K == 1) return a[0];
    else return add4(tree<K / 2>(a), tree<K / 2>(a + K / 2));
}

template <class T>
__device__ __forceinline__ uint32_t count_of(const uint32_t* w, int j);
template <>
__device__ __forceinline__ uint32_t count_of<uint32_t>(const uint32_t* w, int j) { return w[j]; }
template <>
__device__ __forceinline__ uint32_t count_of<uint16_t>(const uint32_t* w, int j) { return (j & 1) ? (w[j >> 1] >> 16) : (w[j >> 1] & 0xffffu); }

// N counts at p into c; only the first `valid` exist (the rest read as 0 and belong to no pixel).
template <class T, int N>
__device__ __forceinline__ void load_counts(const T* __restrict__ p, uint32_t valid, uint32_t (&c)[N]) {
    constexpr int kWords = N * (int)sizeof(T) / 4;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
    uint32_t w[kWords];
    if (kWords >= 4 && valid == (uint32_t)N && (addr & 15u) == 0u) {
#pragma unroll
        for (int v = 0; v < kWords / 4; v++) {
            const uint4 q = reinterpret_cast<const uint4*>(p)[v];
            w[4 * v] = q.x; w[4 * v + 1] = q.y; w[4 * v + 2] = q.z; w[4 * v + 3] = q.w;
        }
    } else if (valid == (uint32_t)N && (addr & 7u) == 0u) {
#pragma unroll
        for (int v = 0; v < kWords / 2; v++) {
            const uint2 q = reinterpret_cast<const uint2*>(p)[v];
            w[2 * v] = q.x; w[2 * v + 1] = q.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < N; j++) c[j] = (uint32_t)j < valid ? (uint32_t)p[j] : 0u;
        return;
    }
#pragma unroll
    for (int j = 0; j < N; j++) c[j] = count_of<T>(w, j);
}

// Pixels per lane: 16 B of a sample row's counts, at least one pixel and at most two (four pixels per lane — s = 2 / uint16_t — measured
// slower than two: its four 16-B stores per lane lie 64 B apart).
template <int S, class T>
struct ResolveGroup {
    static constexpr int kFit = 16 / (int)sizeof(T) / S;
    static constexpr int kPixels = kFit < 1 ? 1 : kFit > 2 ? 2 : kFit;
};

// One lane: kPixels adjacent pixels of one compact pixel row; blockIdx.y strides over the rows.  table: (max_iter + 1) vec4.
template <int S, class T>
__global__ void __launch_bounds__(256) mandel_resolve_kernel(const T* __restrict__ samples, const float4* __restrict__ table,
                                                             float4* __restrict__ rgba, uint32_t W, uint32_t rows, uint32_t max_iter) {
    constexpr int kPixels = ResolveGroup<S, T>::kPixels;
    constexpr int kElems = kPixels * S;   // counts per lane and sample row
    constexpr int kChunk = S < 4 ? S : 4;   // sample rows whose gathers are issued together
    const uint32_t groups = (W + (uint32_t)kPixels - 1u) / (uint32_t)kPixels;
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= groups) return;
    const uint32_t x0 = g * (uint32_t)kPixels;
    const uint32_t npx = W - x0 < (uint32_t)kPixels ? W - x0 : (uint32_t)kPixels;
    const size_t pitch = (size_t)S * W;   // counts per sample row
    const float inv = 1.0f / (float)(S * S);
    for (uint32_t y = blockIdx.y; y < rows; y += gridDim.y) {
        const T* __restrict__ first = samples + (size_t)y * S * pitch + (size_t)x0 * S;
        // rows in chunks of at most four, a chunk's gathers in flight together: tree(r_0 .. r_7) = tree(r_0 .. r_3) + tree(r_4 .. r_7), so
        // s = 8 adds its two chunk sums and holds 32 gathered vec4 at a time, not 64 (240 VGPRs and two waves per SIMD otherwise)
        float4 t[kPixels];
#pragma unroll 1
        for (int h = 0; h < S / kChunk; h++) {
            float4 r[kPixels][kChunk];
#pragma unroll
            for (int i = 0; i < kChunk; i++) {
                uint32_t c[kElems];
                load_counts<T, kElems>(first + (size_t)(h * kChunk + i) * pitch, npx * (uint32_t)S, c);
#pragma unroll
                for (int k = 0; k < kPixels; k++) {
                    float4 a[S];
#pragma unroll
                    for (int j = 0; j < S; j++) {
                        const uint32_t n = c[k * S + j];
                        a[j] = table[n > max_iter ? max_iter : n];   // the clamp of mandel_recolour_kernel
                    }
                    r[k][i] = tree<S>(a);
                }
            }
#pragma unroll
            for (int k = 0; k < kPixels; k++) {
                const float4 q = tree<kChunk>(r[k]);
                t[k] = h == 0 ? q : add4(t[k], q);
            }
        }
#pragma unroll
        for (int k = 0; k < kPixels; k++)
            if ((uint32_t)k < npx)
                rgba[(size_t)y * W + x0 + (uint32_t)k] = make_float4(t[k].x * inv, t[k].y * inv, t[k].z * inv, t[k].w * inv);
    }
}

template <int S, class T>
void resolve_launch(const void* d_samples, const void* table, void* d_rgba, uint32_t W, uint32_t rows, uint32_t max_iter, hipStream_t s) {
    constexpr uint32_t kPixels = (uint32_t)ResolveGroup<S, T>::kPixels;
    const uint32_t groups = (W + kPixels - 1u) / kPixels;
    const dim3 grid((groups + 255u) / 256u, std::min<uint32_t>(rows, 65535u)), block(256);
    hipLaunchKernelGGL((mandel_resolve_kernel<S, T>), grid, block, 0, s, (const T*)d_samples, (const float4*)table, (float4*)d_rgba, W, rows,
                       max_iter);
}

bool factor_ok(uint32_t s) { return s == 2u || s == 4u || s == 8u; }

int refuse_factor(const char* who, uint32_t s) {
    set_error_detail(std::string(who) + ": MC_MANDEL_SUPERSAMPLE(" + std::to_string(s) + "): the factor is 2, 4 or 8 (0 and 1: off)");
    return MC_ERR_INVALID_ARGUMENT;
}

}  // namespace

int mandelbrot_supersample_params(const mc_mandelbrot_params* p, mc_mandelbrot_params* q) {
    if (!p || !q) return MC_ERR_INVALID_ARGUMENT;
    uint32_t s = (p->flags >> 8) & 15u;
    if (s <= 1u) s = 1u;   // off: the sample grid is the image's own
    else if (!factor_ok(s)) return refuse_factor("mc_mandelbrot_supersample_params", s);
    const uint32_t in[6] = {p->width, p->height, p->row_begin, p->row_end, p->row_block, p->row_stride};
    for (uint32_t v : in)
        if ((uint64_t)v * s > 0xffffffffull) {
            set_error_detail("mc_mandelbrot_supersample_params: a width, height or row number times the factor exceeds 2^32 - 1");
            return MC_ERR_INVALID_ARGUMENT;
        }
    mc_mandelbrot_params out = *p;   // (p and q may be the same object)
    out.width = p->width * s; out.height = p->height * s;
    out.row_begin = p->row_begin * s; out.row_end = p->row_end * s;
    out.row_block = p->row_block * s; out.row_stride = p->row_stride * s;
    out.flags &= ~((uint32_t)MC_MANDEL_SUPERSAMPLE(15) | (uint32_t)MC_MANDEL_COLOUR_EQUALISED | (uint32_t)MC_MANDEL_SUPERSAMPLE_ADAPTIVE);
    if (out.flags & MC_MANDEL_SUPERSAMPLE_SMOOTH) {   // the samples are smooth counts: q renders the grid's q plane (mandel_resolve_smooth.hip)
        if (out.flags & MC_MANDEL_COLOUR_SMOOTH_EQUALISED)
            out.flags = (out.flags & ~(uint32_t)MC_MANDEL_COLOUR_SMOOTH_EQUALISED) | (uint32_t)MC_MANDEL_COLOUR_SMOOTH;
        out.flags &= ~(uint32_t)MC_MANDEL_SUPERSAMPLE_SMOOTH;
    }
    if (out.flags & MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE) {   // likewise: the list render's samples are the grid's smooth counts (mandel_refine_smooth.hip)
        if (out.flags & MC_MANDEL_COLOUR_SMOOTH_EQUALISED)
            out.flags = (out.flags & ~(uint32_t)MC_MANDEL_COLOUR_SMOOTH_EQUALISED) | (uint32_t)MC_MANDEL_COLOUR_SMOOTH;
        out.flags &= ~(uint32_t)MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE;
    }
    *q = out;
    return MC_OK;
}

int mandelbrot_resolve_launch(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_samples, uint32_t iters_bytes,
                              const uint32_t* map, void* d_rgba, hipStream_t s) {
    if (!ctx || !p || !d_samples || !d_rgba || !p->max_iter || !rows_ok(p)) return MC_ERR_INVALID_ARGUMENT;
    if (iters_bytes != 2u && iters_bytes != 4u) return MC_ERR_INVALID_ARGUMENT;
    if (iters_bytes == 2u && p->max_iter > 65535u) return MC_ERR_INVALID_ARGUMENT;
    if (p->row_stride && (!p->row_block || p->row_block > p->row_stride)) return MC_ERR_INVALID_ARGUMENT;
    const uint32_t f = (p->flags >> 8) & 15u;
    if (!factor_ok(f)) return refuse_factor("mc_mandelbrot_resolve_device_async", f);
    if ((uint64_t)p->width * f > 0xffffffffull) return MC_ERR_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(d_samples) % iters_bytes || reinterpret_cast<uintptr_t>(d_rgba) % 16u) return MC_ERR_INVALID_ARGUMENT;
    const void* table = nullptr;
    int rc = map ? mandelbrot_composed_table(ctx, p, map, "mc_mandelbrot_resolve_device_async", s, &table)
                 : mandelbrot_lut_device(ctx, p, s, &table);
    if (rc) return rc;
    const uint32_t W = p->width, M = p->max_iter;
    const uint32_t rows = tile_rows(p->row_begin, p->row_end, p->row_stride ? p->row_block : 0u, p->row_stride);
    if (iters_bytes == 4u) {
        if (f == 2u) resolve_launch<2, uint32_t>(d_samples, table, d_rgba, W, rows, M, s);
        else if (f == 4u) resolve_launch<4, uint32_t>(d_samples, table, d_rgba, W, rows, M, s);
        else resolve_launch<8, uint32_t>(d_samples, table, d_rgba, W, rows, M, s);
    } else {
        if (f == 2u) resolve_launch<2, uint16_t>(d_samples, table, d_rgba, W, rows, M, s);
        else if (f == 4u) resolve_launch<4, uint16_t>(d_samples, table, d_rgba, W, rows, M, s);
        else resolve_launch<8, uint16_t>(d_samples, table, d_rgba, W, rows, M, s);
    }
    MC_HIP_TRY(hipGetLastError());
    return ctx->note_launch(s);   // (reads a cached colour table)
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_mandelbrot_supersample_params(const mc_mandelbrot_params* p, mc_mandelbrot_params* q) { return mandelbrot_supersample_params(p, q); }

int mc_mandelbrot_resolve_device_async(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_samples, uint32_t iters_bytes,
                                       const uint32_t* map, void* d_rgba_f32, void* stream) {
    if (!ctx || !p || !d_samples || !d_rgba_f32 || !p->max_iter || (iters_bytes != 2u && iters_bytes != 4u)) return MC_ERR_INVALID_ARGUMENT;
    if (int rc = smooth_samples_refuse_flag(p, "mc_mandelbrot_resolve_device_async")) return rc;
    if (int rc = smooth_equalised_refuse_flag(p, "mc_mandelbrot_resolve_device_async")) return rc;
    if (int rc = smooth_refuse_flag(p, "mc_mandelbrot_resolve_device_async")) return rc;
    if (int rc = distance_refuse_flag(p, "mc_mandelbrot_resolve_device_async")) return rc;
    if (p->flags & MC_MANDEL_SUPERSAMPLE_ADAPTIVE) {
        set_error_detail("mc_mandelbrot_resolve_device_async: MC_MANDEL_SUPERSAMPLE_ADAPTIVE: this call resolves a FULL sample plane; the adaptive "
                         "render is mc_mandelbrot_render / mc_mandelbrot_render_rgba8 of a whole image");
        return MC_ERR_INVALID_ARGUMENT;
    }
    MC_HIP_TRY(hipSetDevice(ctx->device));
    return mandelbrot_resolve_launch(ctx, p, d_samples, iters_bytes, map, d_rgba_f32, stream ? (hipStream_t)stream : ctx->stream);
}

}  // extern "C"
