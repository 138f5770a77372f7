// Instantiates the MC_PT_MATH_STRICT tier of the BVH path tracer kernels (pt_bvh_kernel.h): IEEE divide / sqrt and the mc_math sin / cos /
// pow, no contraction (the command line's -ffp-contract=off, as pathtrace_strict.hip): bit-identical to the CPU oracle.
#include "pt_bvh_kernel.h"

namespace mc { namespace pt {
template <> int launch_bvh_tier<0>(const BvhArgs& k, int S, uint32_t tile_rows, hipStream_t s) { return launch_bvh_tier_impl<0>(k, S, tile_rows, s); }
template <> int launch_bvh_list_tier<0>(const BvhArgs& k, const BvhListArgs& l, int S, hipStream_t s) { return launch_bvh_list_tier_impl<0>(k, l, S, s); }
} }
