// Adaptive smooth supersampling of the Mandelbrot image for gfx950 (MI355X): the refine list over smooth counts and the whole-image chain
// around it.  The project's own addition; contract in include/mc_compute.h (MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE), restated in
// tests/mandel_adaptive_smooth_ref.py; scheme and measurements in DESIGN.md §3.28.
//
// A pixel gets its s x s smooth samples only where its plain smooth count (the anchor: sample (0, 0) of the pixel, which is the plain
// W x H smooth image's q bit for bit) is further than a threshold from one of its up to eight neighbours' (mandel_refine_smooth.h).
// The chain:
//   plain smooth render of W x H -> anchor plane q (+ the plain colours) -> [its smooth histogram, knot map and the plain ranked colours]
//   -> refine list (this file) -> list render: the six smooth list kernels (mandel_adaptive_smooth.h), which resolve a pixel's colour
//   between its s^2 lanes and overwrite the refined pixels.  No sample plane exists.
//  * the list: one lane per pixel, nine reads of the anchor plane, a wave ballot, the four waves' totals exchanged through LDS and ONE
//    vector atomic add per 256-lane block that has a refined pixel; each lane writes its index at its prefix position.  The list's ORDER
//    depends on the order the atomics arrive in; nothing downstream depends on it.
//  * mc_mandelbrot_refine_smooth, the rule on the host, is mandel_refine_smooth_host.cpp: a translation unit without HIP.
//  * the tables: the anchor pass reads the image's c / dc table, the list pass the grid's; the side record keeps the one that is not in
//    the context's slot and the two are swapped around the anchor pass, as mandel_refine.hip does.
#include <algorithm>
#include <vector>

#include "mandel_adaptive_smooth.h"
#include "mandel_adaptive_smooth_host.h"
#include "mandel_equalise.h"
#include "mandel_refine_smooth.h"
#include "mandel_resolve_smooth_host.h"
#include "mandel_side_record.h"

namespace mc {

namespace {

// One lane per pixel.  Every lane reaches both barriers (no early return); lanes past the plane are not refined.
__global__ void __launch_bounds__(256) mandel_refine_smooth_kernel(const uint32_t* __restrict__ plane, uint32_t W, uint32_t H, uint32_t top,
                                                                   uint32_t tau, uint32_t* __restrict__ list,
                                                                   uint32_t* __restrict__ counter) {
    __shared__ uint32_t wave_total[4];
    __shared__ uint32_t block_base;
    const uint64_t total = (uint64_t)W * H;
    const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    bool refined = false;
    if (idx < total) {
        const uint32_t y = (uint32_t)(idx / W), x = (uint32_t)(idx - (uint64_t)y * W);
        refined = refine_smooth::refined(plane, W, H, y, x, top, tau);
    }
    const uint64_t ballot = __ballot(refined);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0u) wave_total[wave] = (uint32_t)__popcll(ballot);
    __syncthreads();
    const uint32_t t0 = wave_total[0], t1 = wave_total[1], t2 = wave_total[2], t3 = wave_total[3];
    const uint32_t sum = ((t0 + t1) + t2) + t3;
    if (threadIdx.x == 0u && sum) block_base = atomicAdd(counter, sum);   // the block's ONE add
    __syncthreads();
    if (refined) {
        const uint32_t before = wave == 0u ? 0u : wave == 1u ? t0 : wave == 2u ? t0 + t1 : (t0 + t1) + t2;
        list[block_base + before + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull))] = (uint32_t)idx;
    }
}

// The context's state of the chain, a side record of the context (mandel_side_record.h).
struct AdaptiveSmoothState {
    DeviceBuffer list, counter;     // W * H indices; one uint32_t
    DeviceBuffer img_tab;           // the c / dc table slot that is NOT in ctx->ctab at the moment (the image's, between calls)
    std::vector<float> img_key;
    uint32_t count_host = 0;
};
SideRecords<AdaptiveSmoothState> g_as_states;

uint32_t log2_of(uint32_t s) { return s == 2u ? 1u : s == 4u ? 2u : 3u; }

// The plain smooth render of the image: the anchor pass.
mc_mandelbrot_params anchor_params(const mc_mandelbrot_params* p) {
    mc_mandelbrot_params q = *p;
    q.flags &= ~((uint32_t)MC_MANDEL_SUPERSAMPLE(15) | (uint32_t)MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE | (uint32_t)MC_MANDEL_COLOUR_SMOOTH_EQUALISED);
    q.flags |= (uint32_t)MC_MANDEL_COLOUR_SMOOTH;
    return q;
}

}  // namespace

int mandelbrot_refine_smooth_launch(const uint32_t* d_plane, uint32_t W, uint32_t H, uint32_t max_iter, uint32_t tau, uint32_t* d_list,
                                    uint32_t* d_counter, hipStream_t s) {
    const uint64_t total = (uint64_t)W * H;
    if (!d_plane || !d_list || !d_counter || !total || total > 0xffffffffull || !max_iter || max_iter > kSmoothMaxIter)
        return MC_ERR_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(d_plane) % 4u || reinterpret_cast<uintptr_t>(d_list) % 4u || reinterpret_cast<uintptr_t>(d_counter) % 4u)
        return MC_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(mandel_refine_smooth_kernel, dim3((uint32_t)((total + 255u) / 256u)), dim3(256), 0, s, d_plane, W, H, 256u * max_iter,
                       tau, d_list, d_counter);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

void adaptive_smooth_release(mc_context* ctx) {
    g_as_states.erase(ctx, [](AdaptiveSmoothState& st) {
        st.list.release();
        st.counter.release();
        st.img_tab.release();
    });
}

int mandelbrot_adaptive_smooth_reserve(mc_context* ctx, const mc_mandelbrot_params* p) {
    AdaptiveSmoothState* st = g_as_states.get(ctx);
    const size_t npix = std::max((size_t)p->width * p->height, (size_t)64);
    int rc;
    if ((rc = ctx->scratch_rgba.reserve(npix * 16))) return rc;
    if ((rc = ctx->scratch_iters.reserve(npix * 4))) return rc;
    if ((rc = st->list.reserve(npix * 4))) return rc;
    return st->counter.reserve(256);
}

int mandelbrot_adaptive_smooth_launch(mc_context* ctx, const mc_mandelbrot_params* p, uint32_t threshold, const char* who, hipStream_t s) {
    const uint32_t f = supersample_of(p), M = p->max_iter, W = p->width, H = p->height;
    const bool ranked = smooth_equalised_flag(p);
    const uint64_t npix = (uint64_t)W * H;
    mc_mandelbrot_params grid;
    int rc;
    if ((rc = mandelbrot_supersample_params(p, &grid))) return rc;
    const mc_mandelbrot_params plain = anchor_params(p);
    AdaptiveSmoothState* st = g_as_states.get(ctx);
    void* d_q = ctx->scratch_iters.ptr;
    void* d_rgba = ctx->scratch_rgba.ptr;
    // anchor pass on the image's table (the side record's slot), the context's slot keeping the grid's for the list pass; after the call
    // the context's slot holds the GRID's table (mandel_refine.hip states the price)
    std::swap(ctx->ctab, st->img_tab);
    std::swap(ctx->ctab_key, st->img_key);
    rc = mandelbrot_smooth_launch(ctx, &plain, ranked ? nullptr : d_rgba, nullptr, d_q, s);
    std::swap(ctx->ctab, st->img_tab);
    std::swap(ctx->ctab_key, st->img_key);
    if (rc) return rc;
    const void* pairs = nullptr;
    if (ranked) {   // the anchor plane's histogram: the plain ranked image's knot map, for refined and unrefined pixels alike
        const uint32_t* qmap = nullptr;
        if ((rc = mandelbrot_smooth_equalise_plane_map(ctx, M, d_q, npix, s, &qmap))) return rc;
        mc_mandelbrot_params pe = plain;
        pe.flags = (pe.flags & ~(uint32_t)MC_MANDEL_COLOUR_SMOOTH) | (uint32_t)MC_MANDEL_COLOUR_SMOOTH_EQUALISED;
        if ((rc = mandelbrot_smooth_remap_launch(ctx, &pe, d_q, qmap, nullptr, d_rgba, who, s))) return rc;
        if ((rc = smooth_equalise_pairs_device(ctx, M, qmap, s, &pairs))) return rc;   // (cached by the remap)
    }
    const void* lut = nullptr;
    if ((rc = mandelbrot_lut_device(ctx, p, s, &lut))) return rc;
    MC_HIP_TRY(hipMemsetAsync(st->counter.ptr, 0, 4, s));
    if ((rc = mandelbrot_refine_smooth_launch((const uint32_t*)d_q, W, H, M, threshold, (uint32_t*)st->list.ptr, (uint32_t*)st->counter.ptr, s))) return rc;
    // the list's length sizes the launch (and is the report): 4 bytes back
    MC_HIP_TRY(hipMemcpyAsync(&st->count_host, st->counter.ptr, 4, hipMemcpyDeviceToHost, s));
    MC_HIP_TRY(hipStreamSynchronize(s));
    const uint32_t count = st->count_host;
    if (count > npix) {
        set_error_detail("MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE: the refine list is longer than the image");
        return MC_ERR_HIP;
    }
    if (count) {   // (an empty list launches nothing: a zero-sized grid is an error)
        const SmoothSampleList sl = {{(const uint32_t*)st->list.ptr, count, W, log2_of(f), 1.0f / (float)(f * f), (const float4*)lut, (float4*)d_rgba},
                                     (const uint2*)pairs};
        if ((rc = mandelbrot_list_smooth_launch(ctx, &grid, sl, s, false))) return rc;
    }
    adaptive_report(ctx, count, npix);
    return MC_OK;
}

int mandelbrot_adaptive_smooth_warmup(mc_context* ctx, const mc_mandelbrot_params* p, hipStream_t s) {
    int rc = mandelbrot_adaptive_smooth_reserve(ctx, p);
    if (rc) return rc;
    AdaptiveSmoothState* st = g_as_states.get(ctx);
    const mc_mandelbrot_params plain = anchor_params(p);
    std::swap(ctx->ctab, st->img_tab);   // the image's table into the side record's slot (the anchor pass's)
    std::swap(ctx->ctab_key, st->img_key);
    rc = mandelbrot_warmup(ctx, &plain, ctx->scratch_iters.ptr, s);
    std::swap(ctx->ctab, st->img_tab);
    std::swap(ctx->ctab_key, st->img_key);
    if (rc) return rc;
    MC_HIP_TRY(hipMemsetAsync(ctx->scratch_iters.ptr, 0, 256, s));
    MC_HIP_TRY(hipMemsetAsync(st->counter.ptr, 0, 4, s));
    MC_HIP_TRY(hipMemsetAsync(st->list.ptr, 0, 4, s));   // entry 0: pixel 0
    if ((rc = mandelbrot_refine_smooth_launch((const uint32_t*)ctx->scratch_iters.ptr, 8, 8, p->max_iter, refine_smooth::kDefaultThreshold,
                            (uint32_t*)st->list.ptr, (uint32_t*)st->counter.ptr, s)))
        return rc;
    mc_mandelbrot_params grid;
    if ((rc = mandelbrot_supersample_params(p, &grid))) return rc;
    const void* lut = nullptr;
    if ((rc = mandelbrot_lut_device(ctx, p, s, &lut))) return rc;
    const void* pairs = nullptr;
    if (smooth_equalised_flag(p)) {   // the knots of a flat histogram: the pair table's device buffer at the request's size
        std::vector<uint32_t> identity((size_t)p->max_iter + 1);
        for (size_t j = 0; j < identity.size(); j++) identity[j] = 256u * (uint32_t)j;
        if ((rc = smooth_equalise_pairs_device(ctx, p->max_iter, identity.data(), s, &pairs))) return rc;
    }
    const uint32_t f = supersample_of(p);
    const SmoothSampleList sl = {{(const uint32_t*)st->list.ptr, 1u, p->width, log2_of(f), 1.0f / (float)(f * f), (const float4*)lut,
                                  (float4*)ctx->scratch_rgba.ptr},
                                 (const uint2*)pairs};
    return mandelbrot_list_smooth_launch(ctx, &grid, sl, s, true);
}

}  // namespace mc
