// MC_MANDEL_COLOUR_DISTANCE, host side: the stage's launcher and the flag's refusals, for the translation units with entry points that take
// mc_mandelbrot_params (api.hip, mandel_distance.hip, mandel_histogram.hip, mandel_resolve.hip; multi.hip words its own refusal).  The
// arithmetic is in mandel_distance.h.
#pragma once
#include <string>

#include "mandel_smooth_host.h"

namespace mc {

// mandel_distance.hip: D and / or the shaded colours of p's rows [row_begin, row_end), stored compactly, from the WHOLE image's q plane.
// who: the entry point's name for the refusals.
int mandelbrot_distance_launch(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_smooth, float threshold_px, void* d_distance,
                               void* d_rgba, const char* who, hipStream_t s);

inline bool distance_flag(const mc_mandelbrot_params* p) { return p && (p->flags & MC_MANDEL_COLOUR_DISTANCE) != 0u; }

// From a call that cannot see the whole image's smooth plane, or that builds colours from a plane of integer counts:
inline int distance_refuse_flag(const mc_mandelbrot_params* p, const char* who) {
    if (!distance_flag(p)) return MC_OK;
    set_error_detail(std::string(who) + ": MC_MANDEL_COLOUR_DISTANCE is a stencil over the WHOLE image's smooth plane: use mc_mandelbrot_render, "
                     "mc_mandelbrot_render_rgba8 or mc_mandelbrot_render_distance with row_begin = 0, row_end = height, no interleave; by hand: "
                     "mc_mandelbrot_render_smooth_device_async (MC_MANDEL_COLOUR_SMOOTH) for the q plane, then "
                     "mc_mandelbrot_distance_device_async per band");
    return MC_ERR_INVALID_ARGUMENT;
}

// What the flag does not combine with (it is a colouring of its own and implies the smooth count), and smooth's limit on max_iter: the
// calls that honour the flag, the stage and the warm-up.
inline int distance_refuse_combination(const mc_mandelbrot_params* p, const char* who) {
    if (!distance_flag(p)) return MC_OK;
    const char* other = (p->flags & MC_MANDEL_COLOUR_SMOOTH)          ? "MC_MANDEL_COLOUR_SMOOTH (the flag implies the smooth count and is set without it)"
                        : (p->flags & MC_MANDEL_COLOUR_EQUALISED)     ? "MC_MANDEL_COLOUR_EQUALISED (the rank map over fractional counts is MC_MANDEL_COLOUR_SMOOTH_EQUALISED, a colouring of its own)"
                        : (p->flags & MC_MANDEL_SUPERSAMPLE_ADAPTIVE) ? "MC_MANDEL_SUPERSAMPLE_ADAPTIVE (a resolve over fractional counts does not exist)"
                        : ((p->flags >> 8) & 15u) > 1u                ? "MC_MANDEL_SUPERSAMPLE (a resolve over fractional counts does not exist)"
                        : (p->flags & MC_MANDEL_FMA)                  ? "MC_MANDEL_FMA (the contraction switch has no smooth kernel)"
                                                                      : nullptr;
    if (other) {
        set_error_detail(std::string(who) + ": MC_MANDEL_COLOUR_DISTANCE does not combine with " + other);
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (p->max_iter > kSmoothMaxIter) {
        set_error_detail(std::string(who) + ": MC_MANDEL_COLOUR_DISTANCE needs max_iter <= 2^24 - 1 (the smooth plane is 24.8 fixed point)");
        return MC_ERR_INVALID_ARGUMENT;
    }
    return MC_OK;
}

}  // namespace mc
