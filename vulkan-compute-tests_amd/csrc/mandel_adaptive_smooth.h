// Adaptive smooth supersampling (MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE, mandel_refine_smooth.hip): what the six list kernels over smooth
// samples share.  The list mapping is mandel_adaptive.h's (sample_lane); a lane's sample is a smooth count q (mandel_smooth.h), its colour
// resolve_smooth::sample_colour (mandel_resolve_smooth.h), a pixel's colour the butterfly of sample_resolve.  DESIGN.md §3.28.
#pragma once
#include "mandel_adaptive.h"
#include "mandel_resolve_smooth.h"

namespace mc {

// What a smooth list render gets beside its kernel's own arguments (which describe the SAMPLE GRID, as for SampleList).
struct SmoothSampleList {
    SampleList l;                       // l.table: the colour table itself, max_iter + 1 vec4 (never a composed one)
    const uint2* __restrict__ pairs;    // ranked: the pair table of §3.21, max_iter (knot, step) entries; null: unranked
};

#ifdef __HIPCC__
struct SmoothListPairs {
    const uint2* __restrict__ p;
    __device__ __forceinline__ resolve_smooth::Knot operator()(uint32_t j) const {
        const uint2 v = p[j];
        return resolve_smooth::Knot{v.x, v.y};
    }
};
struct SmoothListLut {
    const float4* __restrict__ p;
    __device__ __forceinline__ resolve_smooth::Rgba operator()(uint32_t i) const {
        const float4 v = p[i];
        return resolve_smooth::Rgba{v.x, v.y, v.z, v.w};
    }
};

// The lane's smooth count q into its sample colour (ranked or not: wave-uniform), then sample_resolve's butterfly over the flattened
// index i * s + j, which is §3.25's tree (rows of adjacent pairs, then the row sums); the pixel's first lane scales by 1 / s^2 and stores.
// Every lane of the wave takes part; sample_colour clamps q before any index is formed, so an empty entry's lanes gather inside the tables.
__device__ __forceinline__ void smooth_sample_resolve(const SmoothSampleList& sl, const SampleLane& ln, uint32_t q, uint32_t max_iter) {
    const SampleList& l = sl.l;
    const SmoothListPairs pd{sl.pairs};
    const SmoothListLut ld{l.table};
    const resolve_smooth::Rgba v = sl.pairs ? resolve_smooth::sample_colour<true>(q, max_iter, pd, ld)
                                            : resolve_smooth::sample_colour<false>(q, max_iter, pd, ld);
    float4 c = make_float4(v.r, v.g, v.b, v.a);
    const uint32_t group = 1u << (2u * l.log2s);
    for (uint32_t d = 1u; d < group; d <<= 1) {
        c.x = c.x + __shfl_xor(c.x, (int)d);
        c.y = c.y + __shfl_xor(c.y, (int)d);
        c.z = c.z + __shfl_xor(c.z, (int)d);
        c.w = c.w + __shfl_xor(c.w, (int)d);
    }
    if (ln.valid && (threadIdx.x & (group - 1u)) == 0u)
        l.out_rgba[ln.pixel] = make_float4(c.x * l.inv, c.y * l.inv, c.z * l.inv, c.w * l.inv);
}
#endif

// The smooth list render of `grid` (the plain smooth-render params of the sample grid, mc_mandelbrot_supersample_params): every
// precision's kernel under the list mapping; a zero count is the caller's to skip.  warm: one entry, at most 32 iterations.
int mandelbrot_list_smooth_launch(mc_context* ctx, const mc_mandelbrot_params* grid, const SmoothSampleList& sl, hipStream_t s, bool warm);

}  // namespace mc
