// Instantiates the MC_PT_MATH_FAST tier of the list-render kernels (pt_budget_kernel.h), built like pathtrace_fast.hip: the two-float
// primitives and the explicit-polynomial math are included FIRST, under the command line's -ffp-contract=off, then this translation unit
// — and only the path tracer code below — lets the compiler contract a*b+c (MC_PT_FAST_CONTRACT as there).
#include <hip/hip_runtime.h>

#include "mc_internal.h"
#include "ds_arith.h"
#include "mc_math.h"
#ifndef MC_PT_FAST_CONTRACT
#define MC_PT_FAST_CONTRACT 2
#endif
#if MC_PT_FAST_CONTRACT >= 1
#pragma clang fp contract(fast)
#endif
#if MC_PT_FAST_CONTRACT == 1
#define MC_PT_DECISION_FP _Pragma("clang fp contract(off)")
#endif
#include "pt_budget_kernel.h"

namespace mc { namespace pt {
template <> int launch_list_tier<1>(const PTArgs& a, const ListArgs& l, int kernel, int S, hipStream_t s) { return launch_list_tier_impl<1>(a, l, kernel, S, s); }
} }
