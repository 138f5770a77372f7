// Path tracer, per-pixel sample budgets, host side: the launchers and the argument checks the entry points share (pt_budget.hip; the
// chain mc_pathtrace_render_budgeted is api.hip's, beside the blocking calls whose skeleton it uses).  The arithmetic is in pt_budget.h,
// the list render in pt_budget_kernel.h (launched through pathtrace.hip's planning: pathtrace_list_launch, mc_internal.h).
#pragma once
#include "pt_budget.h"
#include "pt_denoise_host.h"

namespace mc {

// max_level at most 8; target finite and above 0 with a finite fp32 square.
int pt_budget_check(float target, uint32_t max_level, const char* who);
// A size the uint32_t storage indices of a list can address: width and height above 0, at most 2^31 pixels.
int pt_budget_check_size(uint32_t W, uint32_t H, const char* who);

inline size_t pt_budget_round256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
constexpr size_t kBudgetCountsBytes = 256;   // the nine counts, then at +128 the nine cursors of the scatter pass

// The level plane (one byte per pixel) of the variance plane on s.
int pt_budget_levels_launch(mc_context* ctx, uint32_t W, uint32_t H, const void* d_variance, float target, uint32_t max_level, void* d_levels,
                            const char* who, hipStream_t s);
// The bucketed list (W * H uint32_t) and the nine counts on s; d_cursors: nine uint32_t of scratch.
int pt_budget_lists_launch(mc_context* ctx, uint32_t W, uint32_t H, const void* d_levels, uint32_t max_level, void* d_list, void* d_counts,
                           void* d_cursors, const char* who, hipStream_t s);
// The resolve from d_acc into d_out (which may be d_acc) on s.  d_levels == NULL: every pixel as level 0, i.e. encode_strict(2 acc), the
// chain's finished pilot (not offered by the entry point).
int pt_budget_resolve_launch(mc_context* ctx, uint32_t W, uint32_t H, const void* d_acc, const void* d_levels, void* d_out, const char* who,
                             hipStream_t s);
// mc_pathtrace_render_list_device_async after the context: every check of the list render, then pathtrace_list_launch.
int pt_budget_list_render(mc_context* ctx, const mc_pathtrace_params* p, const float* planes, uint32_t n_planes, const float* spheres,
                          uint32_t n_spheres, const void* d_list, uint32_t n_list, float prescale, void* d_acc, const char* who, hipStream_t s);

}  // namespace mc
