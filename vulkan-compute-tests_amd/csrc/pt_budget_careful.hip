// Instantiates the careful tier (Fast = 2, csrc/mc_math.h) of the list-render kernels (pt_budget_kernel.h), compiled WITHOUT contraction
// like pathtrace_careful.hip: division, square root and reciprocal square root rounded as the reference rounds them, hardware sine /
// cosine / exp / log.
#include "pt_budget_kernel.h"

namespace mc { namespace pt {
template <> int launch_list_tier<2>(const PTArgs& a, const ListArgs& l, int kernel, int S, hipStream_t s) { return launch_list_tier_impl<2>(a, l, kernel, S, s); }
} }
