// MC_PRECISION_PERTURB (mandel_perturb.hip): the entry points the rest of the library calls.
#pragma once
#include "mc_internal.h"

namespace mc {

// launch_impl (mandelbrot.hip) hands precision 3 over after its common checks: orbit / view / max_iter checks, the colour and dc tables,
// the launch.  warm = the cold-start warm-up's one-tile launch (mc_context_warmup_mandelbrot).
int perturb_launch(mc_context* ctx, const mc_mandelbrot_params* p, void* d_rgba, void* d_iters, hipStream_t s, bool warm);
// mc_context_destroy: the context's bound orbit, if any, is freed.
void perturb_release(mc_context* ctx);

}  // namespace mc
