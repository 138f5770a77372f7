// MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE, host side: the bit's check and refusals and the chain's entry points, for the translation units
// with entry points that take mc_mandelbrot_params (multi.hip words its own refusal).  The refine rule is mandel_refine_smooth.h, the list
// kernels' shared part mandel_adaptive_smooth.h, the chain mandel_refine_smooth.hip.
#pragma once
#include <string>

#include "mc_internal.h"

namespace mc {

inline bool adaptive_smooth_flag(const mc_mandelbrot_params* p) { return p && (p->flags & MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE) != 0u; }

// From every call that does not honour the bit:
inline int adaptive_smooth_refuse_flag(const mc_mandelbrot_params* p, const char* who) {
    if (!adaptive_smooth_flag(p)) return MC_OK;
    set_error_detail(std::string(who) + ": MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE (smooth supersampling of the pixels whose smooth count is "
                     "further than a threshold from a neighbour's) is honoured by mc_mandelbrot_render, mc_mandelbrot_render_rgba8 and "
                     "mc_mandelbrot_render_adaptive_smooth for whole images");
    return MC_ERR_INVALID_ARGUMENT;
}

// What the bit needs and what it does not combine with: the calls that honour it and the warm-up.
inline int adaptive_smooth_check(const mc_mandelbrot_params* p, const char* who) {
    if (!adaptive_smooth_flag(p)) return MC_OK;
    const uint32_t f = (p->flags >> 8) & 15u;
    const bool smooth = (p->flags & MC_MANDEL_COLOUR_SMOOTH) != 0u, ranked = (p->flags & MC_MANDEL_COLOUR_SMOOTH_EQUALISED) != 0u;
    const char* what = (p->flags & MC_MANDEL_SUPERSAMPLE_ADAPTIVE) ? "does not combine with MC_MANDEL_SUPERSAMPLE_ADAPTIVE (that bit compares integer counts; this one is set without it)"
                       : (p->flags & MC_MANDEL_SUPERSAMPLE_SMOOTH) ? "does not combine with MC_MANDEL_SUPERSAMPLE_SMOOTH (that bit is the full resolve; this one is set without it)"
                       : (f != 2u && f != 4u && f != 8u)           ? "needs MC_MANDEL_SUPERSAMPLE(s) with s = 2, 4 or 8"
                       : (smooth == ranked)                        ? "needs exactly one of MC_MANDEL_COLOUR_SMOOTH and MC_MANDEL_COLOUR_SMOOTH_EQUALISED"
                       : (p->flags & MC_MANDEL_COLOUR_EQUALISED)   ? "does not combine with MC_MANDEL_COLOUR_EQUALISED (the rank map over fractional counts is MC_MANDEL_COLOUR_SMOOTH_EQUALISED)"
                       : (p->flags & MC_MANDEL_COLOUR_DISTANCE)    ? "does not combine with MC_MANDEL_COLOUR_DISTANCE (distance shading of supersampled planes does not exist)"
                       : (p->flags & MC_MANDEL_ITERS_U16)          ? "does not combine with MC_MANDEL_ITERS_U16 (the anchor plane is uint32_t smooth counts)"
                       : (p->flags & MC_MANDEL_FMA)                ? "does not combine with MC_MANDEL_FMA (the contraction switch has no smooth kernel)"
                       : p->max_iter > 0x00ffffffu                 ? "needs max_iter <= 2^24 - 1 (the smooth plane is 24.8 fixed point)"
                       : !whole_image(p)                           ? "needs the whole image (row_begin = 0, row_end = height, no interleave): a tile or band cannot see its neighbours' counts"
                       : (uint64_t)p->width * p->height > 0xffffffffull ? "needs width * height <= 2^32 - 1 (the list's entries are uint32_t)"
                                                                   : nullptr;
    if (!what) return MC_OK;
    set_error_detail(std::string(who) + ": MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE " + what);
    return MC_ERR_INVALID_ARGUMENT;
}

// mandel_refine_smooth.hip.  The scratch the chain needs: scratch_rgba (the image), the anchor plane in scratch_iters, the list, its
// counter and the image's c / dc table slot in the side record.
int mandelbrot_adaptive_smooth_reserve(mc_context* ctx, const mc_mandelbrot_params* p);
// The whole-image chain on s into scratch_rgba (p has passed adaptive_smooth_check): the anchor pass, [the anchor plane's histogram, knot
// map and the plain ranked colours,] the refine list, the list render over the refined pixels.  Synchronises s once or twice (the list's
// length; the histogram).  who: the entry point's name for the refusals of the stages it runs.
int mandelbrot_adaptive_smooth_launch(mc_context* ctx, const mc_mandelbrot_params* p, uint32_t threshold, const char* who, hipStream_t s);
// mc_context_warmup_mandelbrot with the bit (the grid's and the image's smooth render have been warmed up): the refine kernel and the
// list kernel of p's precision made resident, the side record's buffers allocated.
int mandelbrot_adaptive_smooth_warmup(mc_context* ctx, const mc_mandelbrot_params* p, hipStream_t s);
// The refine stage alone: the indices y * W + x of the refined pixels of the W x H smooth plane appended to d_list (room for W * H
// entries) in no particular order; *d_counter (zeroed by the caller) ends as the list's length.
int mandelbrot_refine_smooth_launch(const uint32_t* d_plane, uint32_t W, uint32_t H, uint32_t max_iter, uint32_t tau, uint32_t* d_list,
                                    uint32_t* d_counter, hipStream_t s);
// mc_context_destroy: the context's list, counter and table slot, if any, are freed.
void adaptive_smooth_release(mc_context* ctx);
// mandel_refine.hip: what mc_context_last_refined reports, set by either adaptive chain.
void adaptive_report(mc_context* ctx, uint64_t refined, uint64_t pixels);

}  // namespace mc
