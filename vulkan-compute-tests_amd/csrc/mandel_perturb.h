// MC_PRECISION_PERTURB (mandel_perturb.hip): the entry points the rest of the library calls.
#pragma once
#include "mandel_adaptive.h"
#include "mandel_orbit.h"
#include "mandel_target.h"
#include "mc_internal.h"

namespace mc {

struct SmoothSampleList;   // mandel_adaptive_smooth.h: the smooth list render (null everywhere below: not that render)

// launch_impl (mandelbrot.hip) hands precision 3 over after its common checks: orbit / view / max_iter checks, the colour and dc tables,
// the launch.  warm = the cold-start warm-up's one-tile launch (mc_context_warmup_mandelbrot).
// list: the list render of mandel_adaptive.h (p is the sample grid), or nullptr.
// d_smooth: the q plane of MC_MANDEL_COLOUR_SMOOTH, or nullptr; the flag in p selects the smooth instantiation of whichever kernel runs.
// slist: the smooth list render of mandel_adaptive_smooth.h (p is the sample grid and carries MC_MANDEL_COLOUR_SMOOTH; list is null).
int perturb_launch(mc_context* ctx, const mc_mandelbrot_params* p, void* d_rgba, void* d_iters, hipStream_t s, bool warm,
                   const SampleList* list = nullptr, void* d_smooth = nullptr, const SmoothSampleList* slist = nullptr);
// What the launchers below and launch_mapping (mandel_kernels.h) take for MC_MANDEL_COLOUR_SMOOTH: on = the smooth tile mapping (no
// list), q = its plane (may be null).
struct SmoothOut {
    bool on = false;
    uint32_t* q = nullptr;
};
// mc_context_destroy: the context's bound orbit, if any, is freed.
void perturb_release(mc_context* ctx);
// The bound orbit's scale, (scale_x, scale_y) * 2^scale_exp2 as the orbit object holds it; false when no orbit is bound (the zoom
// sequence compares successive keyframes' scales: api.hip).
bool perturb_bound_scale(mc_context* ctx, double* scale_x, double* scale_y, int32_t* scale_exp2);

// The deep kernel (mandel_perturb_deep.hip): orbits with min |scale| < 2^-960, or any orbit under MC_MANDEL_PERTURB_FORCE_DEEP.
// perturb_launch builds the arguments (the dc table holds the scale's mantissas: u = ((double)g / (double)n - 0.5) * mantissa).
struct PerturbDeepArgs {
    MandelTarget t;                  // t.table: [ux[W] | uy[H]]
    int32_t exp2;                    // E: the pixel's offset is u * 2^E
    uint32_t has_zero;               // some Z_j = 0 exactly, 1 <= j < L (centres such as 0 and -1)
};
int perturb_deep_launch(const PerturbDeepArgs& a, dim3 grid, hipStream_t s, const SampleList* list = nullptr, SmoothOut smooth = {},
                        const SmoothSampleList* slist = nullptr);

// The per-lane audit of the fast block (mandel_block_audit.h; mc_hook_mandel_block_audit and mc_hook_mandel_perturb_block_audit of
// libmc_compute_test.so).  d_out: four uint32_t per pixel / lane (n, accepted blocks, raised blocks, first bad block).
// mandelbrot.hip: F32 (MC_MANDEL_FMA honoured), DS, F64 on p's whole image or contiguous rows (mandelbrot_block_audit_kernel of
// mandel_kernels.h).  mandel_perturb.hip: StatePerturb, or (deep) StateDeep with E = exp2, on a device orbit table of L + 1 entries and
// d_table = [ux[n_lanes] | uy[n_lanes]] (mandelbrot_lane_audit_kernel).
int mandelbrot_block_audit_launch(mc_context* ctx, const mc_mandelbrot_params* p, bool sabotage, uint32_t* d_out, hipStream_t s);
int perturb_block_audit_launch(const double2* d_orbit, uint32_t L, bool deep, int32_t exp2, bool has_zero, const double* d_table,
                               uint32_t n_lanes, uint32_t max_iter, bool sabotage, uint32_t* d_out, hipStream_t s);
int perturb_deep_block_audit_launch(const PerturbDeepArgs& a, dim3 grid, bool sabotage, uint32_t* d_out, hipStream_t s);

// MC_PRECISION_PERTURB_BLA (mandel_perturb_bla.hip): PERTURB's loop with bilinear skips, for orbits rendered by the plain loop.
// perturb_launch builds the arguments from the binding: the dc table is PERTURB's, the BLA table the orbit's (mc_mandelbrot_orbit_bla),
// level-major with (A.x, A.y, B.x, B.y, R) per entry; level k starts at entry S(L-2) - S((L-2) >> k), S(n) = 2n - popcount(n)
// (the sum of floor(n / 2^j) over j >= 0), so the kernel needs no offset array.
struct PerturbBlaArgs {
    MandelTarget t;                  // t.table: [dcx[W] | dcy[H]]
    const double* bla;               // the BLA table (null when it has no entry: L < 3)
    uint32_t count_trips;            // MC_MANDEL_BLA_COUNT_TRIPS: write the loop-trip count in place of n
};
int perturb_bla_launch(const PerturbBlaArgs& a, dim3 grid, hipStream_t s, const SampleList* list = nullptr, SmoothOut smooth = {},
                       const SmoothSampleList* slist = nullptr);

// MC_PRECISION_PERTURB_BLA_DEEP (mandel_perturb_bla_deep.hip): the rescaled loop of the deep kernel with bilinear skips, for every orbit.
// The table (mc_mandelbrot_orbit_bla_deep) has precision 4's level layout; each entry is one BlaDeepRec (mandel_orbit.h).
struct PerturbBlaDeepArgs {
    MandelTarget t;                  // t.table: [ux[W] | uy[H]]
    const BlaDeepRec* bla;           // the table (null when it has no entry: L < 3)
    int32_t exp2;                    // E: the pixel's offset is u * 2^E (0 for an orbit of the old scale)
    uint32_t count_trips;            // MC_MANDEL_BLA_COUNT_TRIPS
};
int perturb_bla_deep_launch(const PerturbBlaDeepArgs& a, dim3 grid, hipStream_t s, const SampleList* list = nullptr, SmoothOut smooth = {},
                            const SmoothSampleList* slist = nullptr);

// mc_context_bind_mandelbrot_orbit_tables (mandel_bla_table.hip): the tables named in `tables` (MC_ORBIT_TABLE_*) built on the context's
// device from the orbit table d_orbit (Z_0 .. Z_length, already on the stream) and the orbit's scale fields, into d_bla / d_bla_deep
// (bla_table_bytes each; untouched when the table has no entry).  Blocking: returns with the stream idle and the timing of
// mc_context_last_table_timing recorded.
size_t bla_table_bytes(uint32_t table, uint32_t length);
int bla_table_build(mc_context* ctx, uint32_t tables, const void* d_orbit, uint32_t length, double scale_x, double scale_y, bool deep,
                    int32_t scale_exp2, void* d_bla, void* d_bla_deep, hipStream_t s);
// mc_context_destroy: the context's table-timing events are freed.
void bla_table_release(mc_context* ctx);

// mc_mandelbrot_orbit_create_device (mandel_orbit_device.hip): orbit_create's iteration loop (mandel_orbit.h) on the context's device.
// A launch runs at most orbit_launch_iters(k) = kOrbitLaunchWork / (k + 1)^2 iterations, clamped to [1, 65536].  3.2e7 gives 1864
// iterations at k = 130: 49 ms at the 26.3 us per iteration measured there (which also lists what the rule gives at the
// smaller limb counts, where an iteration's fixed part outweighs its products).
constexpr uint64_t kOrbitLaunchWork = 32000000ull;
uint32_t orbit_launch_iters(int k);
// The constructor with the kernel's phases as lane loops on the host (no device): what libmc_compute_test.so's
// mc_hook_orbit_create_lanes_host calls.
int orbit_create_lanes(const char* centre_x, const char* centre_y, double scale_x, double scale_y, int32_t scale_exp2, uint32_t max_iter,
                       mc_mandelbrot_orbit** out);
// mc_context_destroy: the context's orbit state, slice and events are freed.
void orbit_device_release(mc_context* ctx);

}  // namespace mc
