// MC_PRECISION_PERTURB_BLA_DEEP: the rescaled loop of mandel_perturb_deep.hip with bilinear skips (include/mc_compute.h states the
// contract).
//
// A pixel's offset is delta = w * 2^S exactly (§3.7's state: w, S, the phase, m), and each trip either SKIPS 2^k iterations by one
// entry of the host's floatexp table or runs §3.7's rescaled iteration exactly (escape, rebase and the Z = 0 rule included).
//  * the level: the trip structure of mandel_perturb_bla.hip: level 1 first, then the top level the alignment, the orbit's end and the
//    iterations left allow, then bisection.  The radius test N1(w) 2^S < R is ldexp(N1(w), S - er) < r: exact (R's mantissa r is 0 or
//    in [0.5, 1), so a result that under- or overflows compares as the exact value would).
//  * a skip: P = A w at exponent ea + S, Q = B u at exponent eb + E, aligned with ldexp at the larger frexp exponent, added and
//    normalised; then the plain phase (S = 0, w = d) if |delta'|inf >= T, else the scaled phase with the normalised mantissas and their
//    exponent (delta' = 0: w = 0, S = E, as at the start).
//  * a table entry is one 64-byte record (5 mantissas, 3 exponents), so a probe is one record read.
//  * IEEE double in source order (-ffp-contract=off), fp64 denormals kept; ldexp = v_ldexp_f64, the exponent = v_frexp_exp_i32_f64.
#include "mandel_adaptive_smooth.h"
#include "mandel_perturb.h"
#include "mandel_smooth.h"
#include "mc_internal.h"

namespace mc {

namespace {

constexpr double kT = 0x1p-500;        // the phase threshold T
constexpr double kWinHi = 0x1p256;     // the renormalisation window of |w|inf
constexpr double kWinLo = 0x1p-256;

__device__ __forceinline__ double pow2(int k) { return __builtin_amdgcn_ldexp(1.0, k); }
__device__ __forceinline__ double ldexp2(double x, int k) { return __builtin_amdgcn_ldexp(x, k); }
__device__ __forceinline__ int frexp_exp(double x) { return __builtin_amdgcn_frexp_exp(x); }

// S(n) = sum over j >= 0 of floor(n / 2^j) = 2n - popcount(n): level k of the table starts at entry S(n) - S(n >> k), n = L - 2
__device__ __forceinline__ uint64_t level_sum(uint64_t n) { return 2u * n - (uint64_t)__popcll(n); }

#define MC_BLA_ON_ESCAPE(zx, zy)
__global__ void __launch_bounds__(64) mandel_perturb_bla_deep_kernel(PerturbBlaDeepArgs a) {
    const TileLane ln = tile_lane(a.t);
    const uint32_t gx = ln.gx, gy = ln.gy;
    const bool valid = ln.valid;
#include "mandel_perturb_bla_deep_loop.h"
    tile_store(a.t, ln, a.count_trips ? trips : n);   // trips <= M: every trip but an escaping one advances i by at least one
}

// The same loop under the list mapping of mandel_adaptive.h: a describes the sample grid, a lane is one sample of a refined pixel, and
// the pixel's colour is resolved between the lanes of its samples (no count leaves the kernel).
__global__ void __launch_bounds__(64) mandel_perturb_bla_deep_list_kernel(PerturbBlaDeepArgs a, SampleList l) {
    const SampleLane ln = sample_lane(l);
    const uint32_t gx = ln.gx, gy = ln.gy;
    const bool valid = ln.valid;
#include "mandel_perturb_bla_deep_loop.h"
    sample_resolve(l, ln, a.count_trips ? trips : n, a.t.max_iter);
}
#undef MC_BLA_ON_ESCAPE

// MC_MANDEL_COLOUR_SMOOTH: the loop's escaping z kept (the loop leaves at its one escape test), then the shared epilogue
// (mandel_smooth.h) with c = Z_1 + ldexp(u, E).
#define MC_BLA_ON_ESCAPE(zx, zy) ezx = zx; ezy = zy;
__global__ void __launch_bounds__(64) mandel_perturb_bla_deep_smooth_kernel(PerturbBlaDeepArgs a, uint32_t* __restrict__ out_smooth) {
    const TileLane ln = tile_lane(a.t);
    const uint32_t gx = ln.gx, gy = ln.gy;
    const bool valid = ln.valid;
    double ezx = 0.0, ezy = 0.0;
#include "mandel_perturb_bla_deep_loop.h"
    const double2 c1 = Z[1];
    smooth_tile_store(a.t, ln, out_smooth, n, a.count_trips ? trips : n, ezx, ezy, c1.x + ldexp2(ux, E), c1.y + ldexp2(uy, E));
}

// MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE (mandel_adaptive_smooth.h): the smooth kernel's lane under the list mapping (a: the sample grid);
// q is of n, as the smooth plane's is.  (After every existing kernel, which keep their listings.)
__global__ void __launch_bounds__(64) mandel_perturb_bla_deep_list_smooth_kernel(PerturbBlaDeepArgs a, SmoothSampleList l) {
    const SampleLane ln = sample_lane(l.l);
    const uint32_t gx = ln.gx, gy = ln.gy;
    const bool valid = ln.valid;
    double ezx = 0.0, ezy = 0.0;
#include "mandel_perturb_bla_deep_loop.h"
    (void)trips;
    const double2 c1 = Z[1];
    smooth_sample_resolve(l, ln, smooth::smooth_count(n, a.t.max_iter, ezx, ezy, c1.x + ldexp2(ux, E), c1.y + ldexp2(uy, E)), a.t.max_iter);
}
#undef MC_BLA_ON_ESCAPE

}  // namespace

int perturb_bla_deep_launch(const PerturbBlaDeepArgs& a, dim3 grid, hipStream_t s, const SampleList* list, SmoothOut smooth,
                            const SmoothSampleList* slist) {
    if (slist) hipLaunchKernelGGL(mandel_perturb_bla_deep_list_smooth_kernel, grid, dim3(64), 0, s, a, *slist);
    else if (smooth.on) hipLaunchKernelGGL(mandel_perturb_bla_deep_smooth_kernel, grid, dim3(64), 0, s, a, smooth.q);
    else if (!list) hipLaunchKernelGGL(mandel_perturb_bla_deep_kernel, grid, dim3(64), 0, s, a);
    else hipLaunchKernelGGL(mandel_perturb_bla_deep_list_kernel, grid, dim3(64), 0, s, a, *list);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

}  // namespace mc
