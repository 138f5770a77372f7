// Instantiates the MC_PT_MATH_STRICT tier of the list-render kernels (pt_budget_kernel.h): IEEE divide / sqrt and the mc_math sin / cos /
// pow, no contraction (the command line's -ffp-contract=off, as pathtrace_strict.hip): every sample bit-identical to the CPU oracle's.
#include "pt_budget_kernel.h"

namespace mc { namespace pt {
template <> int launch_list_tier<0>(const PTArgs& a, const ListArgs& l, int kernel, int S, hipStream_t s) { return launch_list_tier_impl<0>(a, l, kernel, S, s); }
} }
