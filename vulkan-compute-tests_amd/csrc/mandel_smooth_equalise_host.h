// MC_MANDEL_COLOUR_SMOOTH_EQUALISED, host side: the stages' launchers and the flag's refusals, for the translation units with entry points
// that take mc_mandelbrot_params (api.hip, mandel_smooth_equalise.hip, mandel_distance.hip, mandel_histogram.hip, mandel_resolve.hip;
// multi.hip words its own refusal).  The arithmetic is in mandel_smooth_equalise.h.
#pragma once
#include <string>

#include "mandel_smooth_host.h"

namespace mc {

// mandel_smooth_equalise.hip.  ADDS the counts of min(q >> 8, max_iter) over n_pixels smooth counts at d_smooth to d_hist[max_iter + 1].
int mandelbrot_smooth_histogram_launch(mc_context* ctx, const void* d_smooth, uint64_t n_pixels, uint32_t max_iter, void* d_hist,
                                       hipStream_t s);
// q' (d_ranked) and / or its smooth colour (d_rgba) for the compact tile p describes; qmap is a HOST table of max_iter + 1 knots.
// who: the entry point's name for the refusals.
int mandelbrot_smooth_remap_launch(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_smooth, const uint32_t* qmap, void* d_ranked,
                                   void* d_rgba, const char* who, hipStream_t s);
// The whole-image chain behind the smooth render of the q plane into d_smooth on s: histogram, table to the host, knot map, remap into
// d_ranked and / or d_rgba.  Synchronises s once (the table round trip).
int mandelbrot_smooth_equalise_whole(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_smooth, void* d_ranked, void* d_rgba,
                                     const char* who, hipStream_t s);
// The knot map of the n smooth counts at d_smooth on s: the histogram into the side record's table, its round trip (s is synchronised once)
// and knot_map on the host.  *qmap: max_iter + 1 knots in the side record, valid until the context's next call of this kind.
int mandelbrot_smooth_equalise_plane_map(mc_context* ctx, uint32_t max_iter, const void* d_smooth, uint64_t n, hipStream_t s,
                                         const uint32_t** qmap);
// mc_context_warmup_mandelbrot with the flag: both kernels made resident on a 64-pixel plane at d_smooth, the side record's buffers
// allocated.
int mandelbrot_smooth_equalise_warmup(mc_context* ctx, const mc_mandelbrot_params* p, void* d_smooth, void* d_rgba, hipStream_t s);
// A caller's knot table (non-decreasing, the last entry 256 * max_iter) and its pair table as a cached device table of the context: what
// the remap stage checks and gathers from, for the count-keyframe compose (mandel_zoom_counts.hip), which gathers from the same table.
int smooth_equalise_check_knots(uint32_t max_iter, const uint32_t* qmap, const char* who);
int smooth_equalise_pairs_device(mc_context* ctx, uint32_t max_iter, const uint32_t* qmap, hipStream_t s, const void** d_pairs);
// mc_context_destroy: the context's histogram and knot table, if any, are freed.
void smooth_equalise_release(mc_context* ctx);

inline bool smooth_equalised_flag(const mc_mandelbrot_params* p) { return p && (p->flags & MC_MANDEL_COLOUR_SMOOTH_EQUALISED) != 0u; }

// From a call that cannot see the whole image's smooth plane, or that builds colours from a plane of integer counts:
inline int smooth_equalised_refuse_flag(const mc_mandelbrot_params* p, const char* who) {
    if (!smooth_equalised_flag(p)) return MC_OK;
    set_error_detail(std::string(who) + ": MC_MANDEL_COLOUR_SMOOTH_EQUALISED ranks the WHOLE image's smooth plane: use mc_mandelbrot_render, "
                     "mc_mandelbrot_render_rgba8 or mc_mandelbrot_render_smooth_equalised with row_begin = 0, row_end = height, no interleave; by "
                     "hand: mc_mandelbrot_render_smooth_device_async (MC_MANDEL_COLOUR_SMOOTH) for the q plane, "
                     "mc_mandelbrot_smooth_histogram_device_async over every tile, mc_mandelbrot_smooth_equalise_map, then "
                     "mc_mandelbrot_smooth_remap_device_async per tile");
    return MC_ERR_INVALID_ARGUMENT;
}

// What the flag does not combine with (it is a colouring of its own and implies the smooth count), and smooth's limit on max_iter: the
// calls that honour the flag, the stage and the warm-up.
inline int smooth_equalised_refuse_combination(const mc_mandelbrot_params* p, const char* who) {
    if (!smooth_equalised_flag(p)) return MC_OK;
    const char* other = (p->flags & MC_MANDEL_COLOUR_SMOOTH)          ? "MC_MANDEL_COLOUR_SMOOTH (the flag implies the smooth count and is set without it)"
                        : (p->flags & MC_MANDEL_COLOUR_EQUALISED)     ? "MC_MANDEL_COLOUR_EQUALISED (the flag is the rank map over fractional counts and is set without it)"
                        : (p->flags & MC_MANDEL_COLOUR_DISTANCE)      ? "MC_MANDEL_COLOUR_DISTANCE (two colourings of one smooth plane: choose one)"
                        : (p->flags & MC_MANDEL_SUPERSAMPLE_ADAPTIVE) ? "MC_MANDEL_SUPERSAMPLE_ADAPTIVE (adaptive refinement of fractional counts does not exist; the full resolve is MC_MANDEL_SUPERSAMPLE_SMOOTH)"
                        : ((p->flags >> 8) & 15u) > 1u                ? "MC_MANDEL_SUPERSAMPLE (the resolve over fractional counts is asked for by name: add MC_MANDEL_SUPERSAMPLE_SMOOTH)"
                        : (p->flags & MC_MANDEL_FMA)                  ? "MC_MANDEL_FMA (the contraction switch has no smooth kernel)"
                                                                      : nullptr;
    if (other) {
        set_error_detail(std::string(who) + ": MC_MANDEL_COLOUR_SMOOTH_EQUALISED does not combine with " + other);
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (p->max_iter > kSmoothMaxIter) {
        set_error_detail(std::string(who) + ": MC_MANDEL_COLOUR_SMOOTH_EQUALISED needs max_iter <= 2^24 - 1 (the smooth plane is 24.8 fixed point)");
        return MC_ERR_INVALID_ARGUMENT;
    }
    return MC_OK;
}

}  // namespace mc
