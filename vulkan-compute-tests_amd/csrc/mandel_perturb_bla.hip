// MC_PRECISION_PERTURB_BLA: PERTURB's loop with bilinear skips (include/mc_compute.h states the contract).
//
// Each pixel runs a loop of its own, one trip at a time: a trip either SKIPS 2^K iterations by one entry (A, B) of the host's BLA table,
// d' = A d + B dc, or runs PERTURB's iteration exactly (escape and rebase tests included).  The escape-time framework of mandel_escape.h
// is not used: its fast block assumes m advances by one per iteration, which a skip breaks.
//  * the level: the largest k >= 1 that the alignment of m, the orbit's end, the iterations left and the radius R_k(m) allow.  The valid
//    levels form a prefix (R_k(m) never increases with k), so the kernel probes level 1 first (a lane whose offset has grown fails it:
//    one probe), then the highest level the three limits allow, then bisects between them.  A probe reads the whole entry (40 B), so
//    the skip has (A, B) in registers once the level is known.
//  * divergence: lanes that skip and lanes that step in the same trip run both branches under the exec mask; a lane's trip is one or
//    the other, so the restatement's per-pixel loop is exactly what each lane computes.  Before any rebase and while every lane takes
//    the same level, a wave shares m and every table read is wave-uniform (one cache line per probe).
//  * IEEE double in source order (-ffp-contract=off), fp64 denormals kept.
#include "mandel_adaptive_smooth.h"
#include "mandel_perturb.h"
#include "mandel_smooth.h"
#include "mc_internal.h"

namespace mc {

namespace {

// S(n) = sum over j >= 0 of floor(n / 2^j) = 2n - popcount(n): level k of the table starts at entry S(n) - S(n >> k), n = L - 2
__device__ __forceinline__ uint64_t level_sum(uint64_t n) { return 2u * n - (uint64_t)__popcll(n); }

#define MC_BLA_ON_ESCAPE(zx, zy)
__global__ void __launch_bounds__(64) mandel_perturb_bla_kernel(PerturbBlaArgs a) {
    const TileLane ln = tile_lane(a.t);
    const uint32_t gx = ln.gx, gy = ln.gy;
    const bool valid = ln.valid;
#include "mandel_perturb_bla_loop.h"
    tile_store(a.t, ln, a.count_trips ? trips : n);   // trips <= M: every trip but an escaping one advances i by at least one
}

// The same loop under the list mapping of mandel_adaptive.h: a describes the sample grid, a lane is one sample of a refined pixel, and
// the pixel's colour is resolved between the lanes of its samples (no count leaves the kernel).
__global__ void __launch_bounds__(64) mandel_perturb_bla_list_kernel(PerturbBlaArgs a, SampleList l) {
    const SampleLane ln = sample_lane(l);
    const uint32_t gx = ln.gx, gy = ln.gy;
    const bool valid = ln.valid;
#include "mandel_perturb_bla_loop.h"
    sample_resolve(l, ln, a.count_trips ? trips : n, a.t.max_iter);
}
#undef MC_BLA_ON_ESCAPE

// MC_MANDEL_COLOUR_SMOOTH: the loop's escaping z kept (the loop leaves at its one escape test), then the shared epilogue
// (mandel_smooth.h) with c = Z_1 + dc.
#define MC_BLA_ON_ESCAPE(zx, zy) ezx = zx; ezy = zy;
__global__ void __launch_bounds__(64) mandel_perturb_bla_smooth_kernel(PerturbBlaArgs a, uint32_t* __restrict__ out_smooth) {
    const TileLane ln = tile_lane(a.t);
    const uint32_t gx = ln.gx, gy = ln.gy;
    const bool valid = ln.valid;
    double ezx = 0.0, ezy = 0.0;
#include "mandel_perturb_bla_loop.h"
    const double2 c1 = Z[1];
    smooth_tile_store(a.t, ln, out_smooth, n, a.count_trips ? trips : n, ezx, ezy, c1.x + dcx, c1.y + dcy);
}

// MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE (mandel_adaptive_smooth.h): the smooth kernel's lane under the list mapping (a: the sample grid);
// q is of n, as the smooth plane's is.  (After every existing kernel, which keep their listings.)
__global__ void __launch_bounds__(64) mandel_perturb_bla_list_smooth_kernel(PerturbBlaArgs a, SmoothSampleList l) {
    const SampleLane ln = sample_lane(l.l);
    const uint32_t gx = ln.gx, gy = ln.gy;
    const bool valid = ln.valid;
    double ezx = 0.0, ezy = 0.0;
#include "mandel_perturb_bla_loop.h"
    (void)trips;
    const double2 c1 = Z[1];
    smooth_sample_resolve(l, ln, smooth::smooth_count(n, a.t.max_iter, ezx, ezy, c1.x + dcx, c1.y + dcy), a.t.max_iter);
}
#undef MC_BLA_ON_ESCAPE

}  // namespace

int perturb_bla_launch(const PerturbBlaArgs& a, dim3 grid, hipStream_t s, const SampleList* list, SmoothOut smooth,
                       const SmoothSampleList* slist) {
    if (slist) hipLaunchKernelGGL(mandel_perturb_bla_list_smooth_kernel, grid, dim3(64), 0, s, a, *slist);
    else if (smooth.on) hipLaunchKernelGGL(mandel_perturb_bla_smooth_kernel, grid, dim3(64), 0, s, a, smooth.q);
    else if (!list) hipLaunchKernelGGL(mandel_perturb_bla_kernel, grid, dim3(64), 0, s, a);
    else hipLaunchKernelGGL(mandel_perturb_bla_list_kernel, grid, dim3(64), 0, s, a, *list);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

}  // namespace mc
