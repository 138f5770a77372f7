// MC_MANDEL_SUPERSAMPLE_SMOOTH, host side: the resolve's launcher and the bit's refusals, for the translation units with entry points
// that take mc_mandelbrot_params (multi.hip words its own refusal).  The arithmetic is in mandel_resolve_smooth.h.
#pragma once
#include <string>

#include "mandel_adaptive_smooth_host.h"
#include "mandel_smooth_equalise_host.h"

namespace mc {

// mandel_resolve_smooth.hip: the colours of p's compact tile (p carries the bit, the factor and one smooth colouring) from the tile's
// compact sample rows of smooth counts at d_smooth.  qmap: a HOST table of max_iter + 1 knots, given exactly when p carries
// MC_MANDEL_COLOUR_SMOOTH_EQUALISED.  who: the entry point's name for the refusals.
int mandelbrot_resolve_smooth_launch(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_smooth, const uint32_t* qmap, void* d_rgba,
                                     const char* who, hipStream_t s);

inline bool smooth_samples_flag(const mc_mandelbrot_params* p) { return p && (p->flags & MC_MANDEL_SUPERSAMPLE_SMOOTH) != 0u; }

// From every call that does not honour the bit.  The same calls do not honour MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE either, and refuse it
// here by its own name (mandel_adaptive_smooth_host.h).
inline int smooth_samples_refuse_flag(const mc_mandelbrot_params* p, const char* who) {
    if (int rc = adaptive_smooth_refuse_flag(p, who)) return rc;
    if (!smooth_samples_flag(p)) return MC_OK;
    set_error_detail(std::string(who) + ": MC_MANDEL_SUPERSAMPLE_SMOOTH (supersampling resolved over smooth counts) is honoured by "
                     "mc_mandelbrot_render, mc_mandelbrot_render_rgba8 and mc_mandelbrot_resolve_smooth_device_async; by hand: "
                     "mc_mandelbrot_render_smooth_device_async of the grid of mc_mandelbrot_supersample_params for the q plane, then "
                     "mc_mandelbrot_resolve_smooth_device_async per tile");
    return MC_ERR_INVALID_ARGUMENT;
}

// What the bit needs and what it does not combine with: the calls that honour it, the resolve stage and the warm-up.
inline int smooth_samples_check(const mc_mandelbrot_params* p, const char* who) {
    if (!smooth_samples_flag(p)) return MC_OK;
    const uint32_t f = (p->flags >> 8) & 15u;
    const bool smooth = (p->flags & MC_MANDEL_COLOUR_SMOOTH) != 0u, ranked = (p->flags & MC_MANDEL_COLOUR_SMOOTH_EQUALISED) != 0u;
    const char* what = (f != 2u && f != 4u && f != 8u) ? "needs MC_MANDEL_SUPERSAMPLE(s) with s = 2, 4 or 8"
                       : (smooth == ranked)            ? "needs exactly one of MC_MANDEL_COLOUR_SMOOTH and MC_MANDEL_COLOUR_SMOOTH_EQUALISED"
                       : (p->flags & MC_MANDEL_SUPERSAMPLE_ADAPTIVE) ? "does not combine with MC_MANDEL_SUPERSAMPLE_ADAPTIVE (adaptive refinement compares integer counts)"
                       : (p->flags & MC_MANDEL_COLOUR_EQUALISED)     ? "does not combine with MC_MANDEL_COLOUR_EQUALISED (the rank map over fractional counts is MC_MANDEL_COLOUR_SMOOTH_EQUALISED)"
                       : (p->flags & MC_MANDEL_COLOUR_DISTANCE)      ? "does not combine with MC_MANDEL_COLOUR_DISTANCE (distance shading of supersampled planes does not exist)"
                       : (p->flags & MC_MANDEL_ITERS_U16)            ? "does not combine with MC_MANDEL_ITERS_U16 (the sample plane is uint32_t smooth counts)"
                       : (p->flags & MC_MANDEL_FMA)                  ? "does not combine with MC_MANDEL_FMA (the contraction switch has no smooth kernel)"
                       : p->max_iter > kSmoothMaxIter                ? "needs max_iter <= 2^24 - 1 (the smooth plane is 24.8 fixed point)"
                                                                     : nullptr;
    if (!what) return MC_OK;
    set_error_detail(std::string(who) + ": MC_MANDEL_SUPERSAMPLE_SMOOTH " + what);
    return MC_ERR_INVALID_ARGUMENT;
}

}  // namespace mc
