// Mandelbrot zoom sequences from count keyframes, host side: the params check the entry points share and the two launchers
// (mandel_zoom_counts.hip; the sequence object is api.hip's, beside the vec4 one).  The arithmetic is in mandel_zoom_counts.h.
#pragma once
#include <string>

#include "mandel_zoom_host.h"

namespace mc {

// The colouring of p as a zoom_counts::Mode, after the refusals every count-keyframe call shares: a whole image without interleave or
// MC_MANDEL_ITERS_U16, at most one colour bit, no distance shading, supersampling or contraction switch, max_iter within the colouring's
// limit.  who: the entry point's name for the refusal.
int zoom_counts_mode(const mc_mandelbrot_params* p, const char* who, int* mode);

// The frame at r from the W x H uint32_t keyframes d_wide and d_deep (or null) into d_rgba_f32 (vec4) and / or d_rgba8 (4 bytes per
// pixel), on s.  d_table: (max_iter + 1) vec4, the colour table or lut[map[.]]; d_pairs: max_iter (knot, step) entries for
// zoom_counts::SmoothEqualised, null otherwise.  zoom_counts_check_args is its check of the pointers (alignment 4 / 4 / 16 / 4, overlap)
// and of r, for a caller that builds tables before it launches.
int zoom_counts_check_args(uint32_t W, uint32_t H, const void* d_wide, const void* d_deep, double r, const void* d_rgba_f32, const void* d_rgba8,
                           const char* who);
int mandelbrot_zoom_counts_launch(mc_context* ctx, uint32_t W, uint32_t H, uint32_t max_iter, int mode, const void* d_wide, const void* d_deep,
                                  const void* d_table, const void* d_pairs, double r, void* d_rgba_f32, void* d_rgba8, const char* who,
                                  hipStream_t s);

// The filtered frame: mandelbrot_zoom_counts_launch's arguments and checks, then the filter's (zoom_check_filter).
// MC_MANDEL_ZOOM_FILTER_BILINEAR launches that call's kernel as it does; MC_MANDEL_ZOOM_FILTER_AREA the area kernel of the mode.
int mandelbrot_zoom_counts_filtered_launch(mc_context* ctx, uint32_t W, uint32_t H, uint32_t max_iter, int mode, const void* d_wide,
                                           const void* d_deep, const void* d_table, const void* d_pairs, double r, uint32_t filter,
                                           void* d_rgba_f32, void* d_rgba8, const char* who, hipStream_t s);

// The frame's table from the two keyframes' DEVICE maps (max_iter + 1 entries each), blended at step of steps_per_octave, one thread per
// entry, on s: lut[map_f[.]] ((max_iter + 1) vec4) for zoom_counts::Equalised, the (knot, step) pairs (max_iter uint2) for
// zoom_counts::SmoothEqualised.  d_lut: the context's colour table.
int mandelbrot_zoom_table_launch(mc_context* ctx, uint32_t max_iter, int mode, const void* d_map_wide, const void* d_map_deep, uint32_t step,
                                 uint32_t steps_per_octave, const void* d_lut, void* d_out, hipStream_t s);

}  // namespace mc
