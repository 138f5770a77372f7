// Adaptive supersampling (MC_MANDEL_SUPERSAMPLE_ADAPTIVE, mandel_refine.hip): the refine list, the list mapping of the six render
// kernels and the entry points the rest of the library calls.  The contract is in include/mc_compute.h; DESIGN.md §3.12 has the scheme.
#pragma once
#include "mc_internal.h"

namespace mc {

// What a list render gets beside its kernel's own arguments (which describe the SAMPLE GRID: its W, H, max_iter and c / dc / u table;
// their output pointers are unused).  A wave takes 64 / s^2 entries of the list; lane l is sample (i, j) = ((l mod s^2) / s,
// (l mod s^2) mod s) of entry l / s^2, so a pixel's s^2 samples are adjacent lanes in the order of the flattened index i * s + j.
struct SampleList {
    const uint32_t* __restrict__ list;   // refined pixels of the IMAGE: y * img_w + x, in any order
    uint32_t count;                      // entries, > 0
    uint32_t img_w;                      // the image's width W (the grid's is s * W)
    uint32_t log2s;                      // 1, 2, 3: s = 2, 4, 8
    float inv;                           // 1 / s^2
    const float4* __restrict__ table;    // max_iter + 1 vec4: the colour table, or lut[map[.]] composed
    float4* __restrict__ out_rgba;       // the image's W x H vec4: the list's pixels are overwritten
};

#ifdef __HIPCC__
struct SampleLane {
    uint32_t gx, gy;   // the lane's sample on the grid
    uint32_t pixel;    // its pixel's index in the image
    bool valid;        // the entry exists (the last wave of a list may be partly empty: whole pixels only)
};

__device__ __forceinline__ SampleLane sample_lane(const SampleList& l) {
    const uint32_t lane = threadIdx.x;
    const uint32_t per = 64u >> (2u * l.log2s);   // entries per wave
    const uint32_t entry = blockIdx.x * per + (lane >> (2u * l.log2s));
    SampleLane r;
    r.valid = entry < l.count;
    r.pixel = l.list[r.valid ? entry : 0u];
    const uint32_t py = r.pixel / l.img_w, px = r.pixel - py * l.img_w;
    const uint32_t sub = lane & ((1u << (2u * l.log2s)) - 1u);
    r.gx = (px << l.log2s) + (sub & ((1u << l.log2s) - 1u));
    r.gy = (py << l.log2s) + (sub >> l.log2s);
    return r;
}

// The contract's tree over a pixel's samples = the adjacent-pair tree over the flattened index: log2(s^2) butterfly steps between lanes
// (IEEE addition commutes bit for bit, so both lanes of a pair hold the same sum).  Every lane of the wave takes part; the pixel's first
// lane scales by 1 / s^2 and stores.
__device__ __forceinline__ void sample_resolve(const SampleList& l, const SampleLane& ln, uint32_t n, uint32_t max_iter) {
    float4 c = l.table[n > max_iter ? max_iter : n];   // the clamp of mandel_recolour_kernel
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

// The list render of `grid` (the plain-render params of the sample grid, mc_mandelbrot_supersample_params): every precision's kernel under
// the list mapping; l.count == 0 is the caller's to skip.  warm: one entry, at most 32 iterations (mc_context_warmup_mandelbrot).
int mandelbrot_list_launch(mc_context* ctx, const mc_mandelbrot_params* grid, const SampleList& l, hipStream_t s, bool warm);

// Step 1: the indices y * W + x of the pixels of the W x H plane (iters_bytes 2: uint16_t, 4: uint32_t) that differ from one of their up
// to eight neighbours, appended to d_list (room for W * H entries) in no particular order; *d_counter (zeroed by the caller) ends as the
// list's length.
int mandelbrot_refine_launch(mc_context* ctx, const void* d_plane, uint32_t iters_bytes, uint32_t W, uint32_t H, uint32_t* d_list,
                             uint32_t* d_counter, hipStream_t s);
// MC_MANDEL_SUPERSAMPLE_ADAPTIVE needs MC_MANDEL_SUPERSAMPLE(s >= 2) and a whole image: MC_OK, or the refusal with its detail string.
int adaptive_check(const mc_mandelbrot_params* p, const char* who);
// The scratch the chain needs beyond scratch_rgba: the anchor plane in scratch_iters, the list and its counter in the side record.
int mandelbrot_adaptive_reserve(mc_context* ctx, const mc_mandelbrot_params* p);
// The whole-image chain on s into scratch_rgba: anchor plane (the plain W x H render), [its histogram, map and composed table,] the plain
// colours, the refine list, the list render over the refined pixels.  Synchronises s once or twice (the list's length; the histogram).
int mandelbrot_adaptive_launch(mc_context* ctx, const mc_mandelbrot_params* p, hipStream_t s);
// mc_context_warmup_mandelbrot with the bit: the refine and list kernels made resident, the side record's buffers allocated.
int mandelbrot_adaptive_warmup(mc_context* ctx, const mc_mandelbrot_params* p, hipStream_t s);
// mc_context_destroy: the context's list, counter and second c table, if any, are freed.
void adaptive_release(mc_context* ctx);

}  // namespace mc
