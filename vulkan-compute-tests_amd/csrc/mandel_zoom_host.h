// Mandelbrot zoom sequences, host side: the compose stage's launcher and the argument checks the entry points share (mandel_zoom.hip; the
// sequence object is api.hip's, beside the blocking render whose chain it drives).  The arithmetic is in mandel_zoom.h.
#pragma once
#include <string>

#include "mc_internal.h"

namespace mc {

// r of a frame: in [0.5, 1], not NaN.  who: the entry point's name for the refusal.
int zoom_check_ratio(double r, const char* who);

// Do the byte ranges [a, a + na) and [b, b + nb) meet?  A null pointer meets nothing.
inline bool zoom_overlaps(const void* a, size_t na, const void* b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

// mandel_zoom.hip: the frame at r from the W x H vec4 keyframes d_wide and d_deep (or null) into d_rgba_f32 (vec4) and / or d_rgba8
// (4 bytes per pixel), on s.  Pointers are checked for alignment (16 bytes; d_rgba8: 4) and the outputs against every other buffer for
// overlap.
int mandelbrot_zoom_launch(mc_context* ctx, uint32_t W, uint32_t H, const void* d_wide, const void* d_deep, double r, void* d_rgba_f32,
                           void* d_rgba8, const char* who, hipStream_t s);

// filter of a filtered call: MC_MANDEL_ZOOM_FILTER_BILINEAR or MC_MANDEL_ZOOM_FILTER_AREA; any other value is refused with the value in
// the detail.  who: the entry point's name for the refusal.
int zoom_check_filter(uint32_t filter, const char* who);

// The filtered frame: mandelbrot_zoom_launch's arguments and checks, then the filter's.  MC_MANDEL_ZOOM_FILTER_BILINEAR launches
// mandelbrot_zoom_launch's kernel as that call does; MC_MANDEL_ZOOM_FILTER_AREA the area kernel (nine taps per deep-sourced pixel).
int mandelbrot_zoom_filtered_launch(mc_context* ctx, uint32_t W, uint32_t H, const void* d_wide, const void* d_deep, double r, uint32_t filter,
                                    void* d_rgba_f32, void* d_rgba8, const char* who, hipStream_t s);

}  // namespace mc
