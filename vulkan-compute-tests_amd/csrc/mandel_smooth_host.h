// MC_MANDEL_COLOUR_SMOOTH, host side: the launcher and the flag's refusals, for the translation units with entry points that take
// mc_mandelbrot_params (api.hip, mandelbrot.hip, mandel_histogram.hip, mandel_resolve.hip; multi.hip words its own refusal).  The
// arithmetic and the kernels' epilogue are in mandel_smooth.h.
#pragma once
#include <string>

#include "mc_internal.h"

namespace mc {

constexpr uint32_t kSmoothMaxIter = 0x00ffffffu;   // smooth::kMaxIter of mandel_smooth.h: 256 * max_iter fits the plane's uint32_t

// mandelbrot.hip: mandelbrot_launch with the smooth plane (p carries MC_MANDEL_COLOUR_SMOOTH; any of the three outputs may be null, not all).
int mandelbrot_smooth_launch(mc_context* ctx, const mc_mandelbrot_params* p, void* d_rgba, void* d_iters, void* d_smooth, hipStream_t s);

// What the flag does not combine with (the colourings and resolves that work on integer counts, the fp32 contraction switch), and its
// limit on max_iter: every render entry point and the launcher itself.
inline int smooth_refuse_combination(const mc_mandelbrot_params* p, const char* who) {
    if (!p || !(p->flags & MC_MANDEL_COLOUR_SMOOTH)) return MC_OK;
    const char* other = (p->flags & MC_MANDEL_COLOUR_EQUALISED)       ? "MC_MANDEL_COLOUR_EQUALISED (the rank map over fractional counts is MC_MANDEL_COLOUR_SMOOTH_EQUALISED, set on its own)"
                        : (p->flags & MC_MANDEL_SUPERSAMPLE_ADAPTIVE) ? "MC_MANDEL_SUPERSAMPLE_ADAPTIVE (adaptive refinement of fractional counts does not exist; the full resolve is MC_MANDEL_SUPERSAMPLE_SMOOTH)"
                        : ((p->flags >> 8) & 15u) > 1u                ? "MC_MANDEL_SUPERSAMPLE (the resolve over fractional counts is asked for by name: add MC_MANDEL_SUPERSAMPLE_SMOOTH)"
                        : (p->flags & MC_MANDEL_FMA)                  ? "MC_MANDEL_FMA (the contraction switch measures the plain fp32 kernel only)"
                                                                      : nullptr;
    if (other) {
        set_error_detail(std::string(who) + ": MC_MANDEL_COLOUR_SMOOTH does not combine with " + other);
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (p->max_iter > kSmoothMaxIter) {
        set_error_detail(std::string(who) + ": MC_MANDEL_COLOUR_SMOOTH needs max_iter <= 2^24 - 1 (the plane is 24.8 fixed point)");
        return MC_ERR_INVALID_ARGUMENT;
    }
    return MC_OK;
}
// From a call that builds colours from a plane of integer counts:
inline int smooth_refuse_flag(const mc_mandelbrot_params* p, const char* who) {
    if (!p || !(p->flags & MC_MANDEL_COLOUR_SMOOTH)) return MC_OK;
    set_error_detail(std::string(who) + ": MC_MANDEL_COLOUR_SMOOTH: the smooth colour needs the escape state, which a count plane does not "
                     "hold; render with mc_mandelbrot_render_smooth or any single-device render call");
    return MC_ERR_INVALID_ARGUMENT;
}

}  // namespace mc
