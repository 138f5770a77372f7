// Histogram-equalised Mandelbrot colouring (MC_MANDEL_COLOUR_EQUALISED, mandel_histogram.hip): the entry points the rest of the
// library calls.  The contract is in include/mc_compute.h; DESIGN.md §3.10 has the scheme and its measurements.
#pragma once
#include "mc_internal.h"

namespace mc {

// The histogram's table: block-private LDS copies of RANGES of kHistRangeBins bins (64 KB), every block counting the values of its own
// range over its share of the plane and flushing once; beyond kHistMaxRanges ranges (max_iter >= 2^20) wave-combined atomics straight to
// the global table (DESIGN.md §3.10 has the measurements behind both constants).
constexpr uint32_t kHistRangeBins = 16384;
constexpr uint32_t kHistMaxRanges = 64;

// ADDS the counts of n_pixels values (iters_bytes 2: uint16_t, 4: uint32_t; values above max_iter count in bin max_iter) to
// d_hist[max_iter + 1].
int mandelbrot_histogram_launch(mc_context* ctx, const void* d_iters, uint32_t iters_bytes, uint64_t n_pixels, uint32_t max_iter,
                                void* d_hist, hipStream_t s);
// map[max_iter + 1] from hist[max_iter + 1] (host only).
int mandelbrot_equalise_map(uint32_t max_iter, const uint32_t* hist, uint32_t* map);
// d_rgba[i] = lut[map[min(n[i], max_iter)]] for the compact tile p describes; map is a HOST table.
int mandelbrot_recolour_launch(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_iters, uint32_t iters_bytes,
                               const uint32_t* map, void* d_rgba, hipStream_t s);
// The whole-image chain after the count plane has been rendered into d_iters (uint32_t) on s: histogram, table to the host, map,
// recolour into d_rgba.  Synchronises s once (the table round trip).
int mandelbrot_equalise_whole(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_iters, void* d_rgba, hipStream_t s);
// mc_context_warmup_mandelbrot with the flag: both kernels made resident (a 64-pixel plane), the side record's buffers allocated.
int mandelbrot_equalise_warmup(mc_context* ctx, const mc_mandelbrot_params* p, hipStream_t s);
// mc_context_destroy: the context's histogram and composed colour table, if any, are freed.
void equalise_release(mc_context* ctx);

}  // namespace mc
