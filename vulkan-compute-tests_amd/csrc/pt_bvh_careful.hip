// Instantiates the careful tier (Fast = 2, csrc/mc_math.h) of the BVH path tracer kernels (pt_bvh_kernel.h), compiled WITHOUT contraction
// like pathtrace_careful.hip: division, square root and reciprocal square root rounded as the reference rounds them, hardware sine /
// cosine / exp / log.  An MC_PT_MATH_FAST request is rendered by this tier too: a scene worth a BVH has four or more spheres.
#include "pt_bvh_kernel.h"

namespace mc { namespace pt {
template <> int launch_bvh_tier<2>(const BvhArgs& k, int S, uint32_t tile_rows, hipStream_t s) { return launch_bvh_tier_impl<2>(k, S, tile_rows, s); }
template <> int launch_bvh_list_tier<2>(const BvhArgs& k, const BvhListArgs& l, int S, hipStream_t s) { return launch_bvh_list_tier_impl<2>(k, l, S, s); }
} }
