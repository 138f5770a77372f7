// Path tracer, per-pixel sample budgets: the level of a pixel from its measured noise and the resolve of a budgeted accumulator plane
// (include/mc_compute.h states the contract, at mc_pathtrace_budget_levels / mc_pathtrace_budget_resolve; DESIGN.md §3.20;
// tests/pt_budget_ref.py restates it in numpy).
//
// One body for the host and the device, as pt_noise.h, whose encode_strict the resolve runs unchanged: pt_budget_levels_kernel /
// pt_budget_resolve_kernel (pt_budget.hip) and mc_pathtrace_budget_levels / mc_pathtrace_budget_resolve run these same functions.  Every
// operation is ONE IEEE-754 fp32 operation in the order written.  Requires -ffp-contract=off.
//
// THE CONTRACT, levels (one float V_p per pixel in, one uint8_t per pixel out, storage order):  tau2 = target * target (once, on the host);
//   t = V_p;  l = 0;  while (l < max_level && t > tau2) { t = t * 0.5f;  l = l + 1; }      NaN: 0 (no comparison holds);  +inf: max_level.
//   The pixel's budget is n0 << l samples.  max_level is 0 .. 8.
// THE CONTRACT, resolve (acc: the linear accumulator plane the rounds leave; a pixel of level 0 still holds the pilot's plane, HALF of its
//   n0-sample accumulator, every other pixel its accumulator at its own divisor):
//   out[p].rgb = encode_strict(acc[p].rgb * (level[p] == 0 ? 2.0f : 1.0f));   out[p].w = acc[p].w.
#pragma once
#include "pt_noise.h"

namespace mc {
namespace ptd {

constexpr uint32_t kMaxBudgetLevel = 8;

MC_PTD_FN uint8_t budget_level(float variance, float tau2, uint32_t max_level) {
    float t = variance;
    uint32_t l = 0;
    while (l < max_level && t > tau2) {
        t = t * 0.5f;
        l = l + 1u;
    }
    return (uint8_t)l;
}

MC_PTD_FN vec4 budget_resolve(vec4 acc, uint32_t level) {
    const float m = level == 0u ? 2.0f : 1.0f;
    return vec4{encode_strict(acc.x * m), encode_strict(acc.y * m), encode_strict(acc.z * m), acc.w};
}

}  // namespace ptd
}  // namespace mc
