// Adaptive supersampling of the Mandelbrot image for gfx950 (MI355X): the refine list and the whole-image chain around it.
// The project's own addition; contract in include/mc_compute.h (MC_MANDEL_SUPERSAMPLE_ADAPTIVE), restated in
// tests/mandel_adaptive_ref.py; scheme and measurements in DESIGN.md §3.12.
//
// A pixel gets its s x s samples only where its plain count (the anchor: sample (0, 0) of the pixel, which is the plain W x H image's
// count bit for bit) differs from one of its up to eight neighbours'.  The chain:
//   plain render of W x H -> anchor plane (+ the plain colours) -> [histogram, map, composed table, recolour when equalised]
//   -> refine list (this file) -> list render: the six render kernels under the list mapping of mandel_adaptive.h, which resolve a
//   pixel's colour between its s^2 lanes and overwrite the refined pixels.  No sample plane exists.
//  * the list: one lane per pixel, nine reads of the anchor plane (2 or 4 B each, neighbouring lanes share the lines), a wave ballot, ONE
//    vector atomic add per wave that has a refined pixel, each lane writing its index at its prefix position.  The list's ORDER
//    depends on the order the atomics arrive in; nothing downstream depends on it (every entry writes its own pixel, from its own samples).
//  * the tables: the anchor pass reads the image's c / dc table, the list pass the grid's.  The context caches one; this file keeps the
//    other in its side record and swaps the two slots around the anchor pass, so that neither is rebuilt from call to call.
//  * the context's state lives in a side record (as mandel_histogram.hip's), not in mc_internal.h.
#include <algorithm>

#include "mandel_adaptive.h"
#include "mandel_adaptive_smooth_host.h"
#include "mandel_equalise.h"
#include "mandel_side_record.h"

namespace mc {

namespace {

// One lane per pixel: nine reads of the anchor plane, a wave ballot, one vector atomic add per wave that has a refined pixel, each lane
// writing its index at its prefix position.  (On K4's plane that is up to 614 400 adds to one address, which serialise: the pass takes
// 3.9 ms there, profiles/mandel_adaptive_probe.txt.  One add per block of several waves is the known remedy)
template <class T>
__global__ void __launch_bounds__(256) mandel_refine_kernel(const T* __restrict__ plane, uint32_t W, uint32_t H, uint32_t* __restrict__ list,
                                                            uint32_t* __restrict__ counter) {
    const uint64_t total = (uint64_t)W * H;
    const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    bool refined = false;
    if (idx < total) {
        const uint32_t y = (uint32_t)(idx / W), x = (uint32_t)(idx - (uint64_t)y * W);
        const T a = plane[idx];
        const uint32_t y0 = y ? y - 1u : 0u, y1 = y + 1u < H ? y + 1u : y;
        const uint32_t x0 = x ? x - 1u : 0u, x1 = x + 1u < W ? x + 1u : x;
        for (uint32_t yy = y0; yy <= y1; yy++)
            for (uint32_t xx = x0; xx <= x1; xx++) refined |= plane[(uint64_t)yy * W + xx] != a;
    }
    const uint64_t ballot = __ballot(refined);
    if (!ballot) return;   // wave-uniform
    const uint32_t lane = __lane_id();
    const uint32_t leader = (uint32_t)__ffsll((unsigned long long)ballot) - 1u;
    uint32_t base = 0u;
    if (lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(ballot));
    base = __shfl(base, (int)leader);
    if (refined) list[base + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull))] = (uint32_t)idx;
}

// The context's adaptive state, a side record of the context (mandel_side_record.h).
struct AdaptiveState {
    DeviceBuffer list, counter;     // W * H indices; one uint32_t
    DeviceBuffer img_tab;           // the c / dc table slot that is NOT in ctx->ctab at the moment (the image's, between calls)
    std::vector<float> img_key;
    uint32_t count_host = 0;
    bool reported = false;          // mc_context_last_refined
    uint64_t refined = 0, pixels = 0;
};
SideRecords<AdaptiveState> g_ad_states;

uint32_t log2_of(uint32_t s) { return s == 2u ? 1u : s == 4u ? 2u : 3u; }

void plain_params(const mc_mandelbrot_params* p, uint32_t iters_bytes, mc_mandelbrot_params* plain) {
    *plain = *p;
    plain->flags &= ~((uint32_t)MC_MANDEL_SUPERSAMPLE(15) | (uint32_t)MC_MANDEL_COLOUR_EQUALISED | (uint32_t)MC_MANDEL_SUPERSAMPLE_ADAPTIVE |
                      (uint32_t)MC_MANDEL_ITERS_U16);
    if (iters_bytes == 2u) plain->flags |= (uint32_t)MC_MANDEL_ITERS_U16;
}

}  // namespace

// What mc_context_last_refined reports: either adaptive chain's last successful render (mandel_refine_smooth.hip calls this too).
void adaptive_report(mc_context* ctx, uint64_t refined, uint64_t pixels) {
    AdaptiveState* st = g_ad_states.get(ctx);
    st->refined = refined;
    st->pixels = pixels;
    st->reported = true;
}

void adaptive_release(mc_context* ctx) {
    g_ad_states.erase(ctx, [](AdaptiveState& st) {
        st.list.release();
        st.counter.release();
        st.img_tab.release();
    });
}

int mandelbrot_refine_launch(mc_context* ctx, const void* d_plane, uint32_t iters_bytes, uint32_t W, uint32_t H, uint32_t* d_list,
                             uint32_t* d_counter, hipStream_t s) {
    if (!ctx || !d_plane || !d_list || !d_counter || !W || !H || (iters_bytes != 2u && iters_bytes != 4u)) {
        set_error_detail("MC_MANDEL_SUPERSAMPLE_ADAPTIVE: the refine list needs a context, a plane of 2- or 4-byte counts, a list and a counter");
        return MC_ERR_INVALID_ARGUMENT;
    }
    const uint64_t total = (uint64_t)W * H;
    if (total > 0xffffffffull) {
        set_error_detail("MC_MANDEL_SUPERSAMPLE_ADAPTIVE: the list's entries are uint32_t, width * height must stay below 2^32");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (reinterpret_cast<uintptr_t>(d_plane) % iters_bytes || reinterpret_cast<uintptr_t>(d_list) % 4u ||
        reinterpret_cast<uintptr_t>(d_counter) % 4u) {
        set_error_detail("MC_MANDEL_SUPERSAMPLE_ADAPTIVE: the refine list's plane, list or counter is not aligned to its element size");
        return MC_ERR_INVALID_ARGUMENT;
    }
    const dim3 grid((uint32_t)((total + 255u) / 256u)), block(256);
    if (iters_bytes == 2u) hipLaunchKernelGGL(mandel_refine_kernel<uint16_t>, grid, block, 0, s, (const uint16_t*)d_plane, W, H, d_list, d_counter);
    else hipLaunchKernelGGL(mandel_refine_kernel<uint32_t>, grid, block, 0, s, (const uint32_t*)d_plane, W, H, d_list, d_counter);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

int adaptive_check(const mc_mandelbrot_params* p, const char* who) {
    if (!p || !(p->flags & MC_MANDEL_SUPERSAMPLE_ADAPTIVE)) return MC_OK;
    if (!supersample_of(p)) {
        set_error_detail(std::string(who) + ": MC_MANDEL_SUPERSAMPLE_ADAPTIVE is valid only together with MC_MANDEL_SUPERSAMPLE(s), s = 2, 4 or 8");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (!whole_image(p)) {
        set_error_detail(std::string(who) + ": MC_MANDEL_SUPERSAMPLE_ADAPTIVE needs the whole image (row_begin = 0, row_end = height, no "
                         "interleave): a tile or band cannot see its neighbours' counts");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if ((uint64_t)p->width * p->height > 0xffffffffull) {
        set_error_detail(std::string(who) + ": MC_MANDEL_SUPERSAMPLE_ADAPTIVE: the list's entries are uint32_t, width * height must stay below 2^32");
        return MC_ERR_INVALID_ARGUMENT;
    }
    return MC_OK;
}

int mandelbrot_adaptive_reserve(mc_context* ctx, const mc_mandelbrot_params* p) {
    AdaptiveState* st = g_ad_states.get(ctx);
    const size_t npix = (size_t)p->width * p->height;
    int rc;
    if ((rc = ctx->scratch_iters.reserve(std::max(npix, (size_t)64) * (p->max_iter <= 65535u ? 2u : 4u)))) return rc;
    if ((rc = st->list.reserve(std::max(npix, (size_t)64) * 4))) return rc;
    return st->counter.reserve(256);
}

int mandelbrot_adaptive_launch(mc_context* ctx, const mc_mandelbrot_params* p, hipStream_t s) {
    const uint32_t f = supersample_of(p), M = p->max_iter, W = p->width, H = p->height;
    const bool equalised = (p->flags & MC_MANDEL_COLOUR_EQUALISED) != 0u;
    const uint32_t iters_bytes = M <= 65535u ? 2u : 4u;
    const uint64_t npix = (uint64_t)W * H;
    mc_mandelbrot_params grid, plain;
    int rc;
    if ((rc = mandelbrot_supersample_params(p, &grid))) return rc;
    plain_params(p, iters_bytes, &plain);
    AdaptiveState* st = g_ad_states.get(ctx);
    // anchor pass on the image's table (the side record's slot), the context's slot keeping the grid's for the list pass.  Nothing else
    // reads ctx->ctab between the two swaps (one thread per context, mandelbrot_launch only).  AFTER the call the context's slot holds
    // the GRID's table: a plain render of the same image that follows rebuilds its table once (the price of adding no second slot to
    // mc_internal.h, whose text the path tracer's build id covers).
    std::swap(ctx->ctab, st->img_tab);
    std::swap(ctx->ctab_key, st->img_key);
    rc = mandelbrot_launch(ctx, &plain, equalised ? nullptr : ctx->scratch_rgba.ptr, ctx->scratch_iters.ptr, s);
    std::swap(ctx->ctab, st->img_tab);
    std::swap(ctx->ctab_key, st->img_key);
    if (rc) return rc;
    const void* table = nullptr;
    if (equalised) {   // the anchor plane's histogram: the plain equalised image's map, for refined and unrefined pixels alike
        const uint32_t* map = nullptr;
        if ((rc = mandelbrot_equalise_plane_map(ctx, M, ctx->scratch_iters.ptr, iters_bytes, npix, s, &map))) return rc;
        if ((rc = mandelbrot_recolour_launch(ctx, &plain, ctx->scratch_iters.ptr, iters_bytes, map, ctx->scratch_rgba.ptr, s))) return rc;
        if ((rc = mandelbrot_composed_table(ctx, p, map, "MC_MANDEL_SUPERSAMPLE_ADAPTIVE", s, &table))) return rc;   // (cached by the recolouring)
    } else if ((rc = mandelbrot_lut_device(ctx, p, s, &table))) {
        return rc;
    }
    MC_HIP_TRY(hipMemsetAsync(st->counter.ptr, 0, 4, s));
    if ((rc = mandelbrot_refine_launch(ctx, ctx->scratch_iters.ptr, iters_bytes, W, H, (uint32_t*)st->list.ptr, (uint32_t*)st->counter.ptr, s)))
        return rc;
    // the list's length sizes the launch (and is the report): 4 bytes back
    MC_HIP_TRY(hipMemcpyAsync(&st->count_host, st->counter.ptr, 4, hipMemcpyDeviceToHost, s));
    MC_HIP_TRY(hipStreamSynchronize(s));
    const uint32_t count = st->count_host;
    if (count > npix) {
        set_error_detail("MC_MANDEL_SUPERSAMPLE_ADAPTIVE: the refine list is longer than the image");
        return MC_ERR_HIP;
    }
    if (count) {   // (an empty list launches nothing: a zero-sized grid is an error)
        const SampleList l = {(const uint32_t*)st->list.ptr, count, W, log2_of(f), 1.0f / (float)(f * f), (const float4*)table,
                              (float4*)ctx->scratch_rgba.ptr};
        if ((rc = mandelbrot_list_launch(ctx, &grid, l, s, false))) return rc;
    }
    adaptive_report(ctx, count, npix);
    return MC_OK;
}

int mandelbrot_adaptive_warmup(mc_context* ctx, const mc_mandelbrot_params* p, hipStream_t s) {
    // scratch_iters holds at least 64 uint32_t, scratch_rgba at least 64 vec4 (mc_context_warmup_mandelbrot); the grid's tables are in
    // place (the warm-up of the grid's plain render ran before this)
    int rc = mandelbrot_adaptive_reserve(ctx, p);
    if (rc) return rc;
    AdaptiveState* st = g_ad_states.get(ctx);
    const uint32_t iters_bytes = p->max_iter <= 65535u ? 2u : 4u;
    mc_mandelbrot_params plain;
    plain_params(p, 4u, &plain);
    std::swap(ctx->ctab, st->img_tab);   // the image's table into the side record's slot (the anchor pass's)
    std::swap(ctx->ctab_key, st->img_key);
    rc = mandelbrot_warmup(ctx, &plain, ctx->scratch_iters.ptr, s);
    std::swap(ctx->ctab, st->img_tab);
    std::swap(ctx->ctab_key, st->img_key);
    if (rc) return rc;
    MC_HIP_TRY(hipMemsetAsync(ctx->scratch_iters.ptr, 0, 256, s));
    MC_HIP_TRY(hipMemsetAsync(st->counter.ptr, 0, 4, s));
    MC_HIP_TRY(hipMemsetAsync(st->list.ptr, 0, 4, s));   // entry 0: pixel 0
    if ((rc = mandelbrot_refine_launch(ctx, ctx->scratch_iters.ptr, iters_bytes, 8, 8, (uint32_t*)st->list.ptr, (uint32_t*)st->counter.ptr, s)))
        return rc;
    mc_mandelbrot_params grid;
    if ((rc = mandelbrot_supersample_params(p, &grid))) return rc;
    const void* table = nullptr;
    if ((rc = mandelbrot_lut_device(ctx, p, s, &table))) return rc;
    const uint32_t f = supersample_of(p);
    const SampleList l = {(const uint32_t*)st->list.ptr, 1u, p->width, log2_of(f), 1.0f / (float)(f * f), (const float4*)table,
                          (float4*)ctx->scratch_rgba.ptr};
    return mandelbrot_list_launch(ctx, &grid, l, s, true);
}

}  // namespace mc

using namespace mc;

extern "C" int mc_context_last_refined(mc_context* ctx, uint64_t* refined, uint64_t* pixels) {
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    AdaptiveState* st = g_ad_states.get(ctx);
    if (!st->reported) {
        set_error_detail("mc_context_last_refined: no adaptive render has succeeded on this context");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (refined) *refined = st->refined;
    if (pixels) *pixels = st->pixels;
    return MC_OK;
}
