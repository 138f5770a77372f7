// Instantiates the MC_PT_MATH_STRICT path tracer kernels (IEEE divide/sqrt + mc_math sin/cos/pow:
// bit-identical to the CPU oracle).  Split from the fast instantiations so both compile in parallel.
#include "pathtrace_kernel.h"
#include "pathtrace_pool.h"

template int mc::pt::launch_tier<0>(const mc::pt::PTArgs&, int, int, int, uint32_t, hipStream_t);

#ifdef MC_PT_REGION_STATS
namespace mc { namespace pt { MC_PT_REGION_STATS_READER(region_stats_strict) } }   // (summed by mc_debug_pt_region_stats, pathtrace_fast.hip)
#endif
