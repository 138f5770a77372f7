// Atom-domain periods (include/mc_compute.h: "atom domains"; what tests/mandel_atom_ref.py restates).
//
// The period of a pixel is the index m in [1, n] at which a_m = max(|x_m|, |y_m|) of its orbit z_1 .. z_n is smallest, the first such index.
// ONE update function for the host and the device: the kernels' capture (AtomCapture, below) and mc_mandelbrot_atom_scan
// (mandel_atom_host.cpp) both run atom::update, so the CPU suite tests the very source the kernels compile.
//
// THE CYCLE EXIT STAYS ON (F32, F64).  escape_time (mandel_escape.h) finishes a lane whose z at the end of a block equals, as a value, the z
// it held at an earlier block end j: from j on the orbit repeats the stretch z_(j+1) .. z_i for ever, so the lane HAS ALREADY SEEN every
// value its orbit will ever take (a +0 / -0 difference does not reach a_m: it is taken of |x| and |y|).  The update is strict (a_m < best),
// so a later visit of the minimum never replaces the index of the first one: (period, amin) over z_1 .. z_i are (period, amin) over
// z_1 .. z_M.  A wave leaves only when each of its lanes has escaped (frozen, below) or is known to cycle, so nothing is lost when it
// does.  tests/test_gpu_mandel_atom.py holds this to a restatement that iterates to M with no exit.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MC_ATOM_FN __host__ __device__ inline
#else
#define MC_ATOM_FN inline
#endif

namespace mc {
namespace atom {

constexpr uint64_t kInfBits = 0x7ff0000000000000ull;   // +inf: the amin of a pixel without a period, and of a period without a pixel
constexpr uint32_t kNoPixel = 0xffffffffu;

// (best, period) after z_m = (x, y), m >= 1; they start at (+inf, 0).  a = max(|x|, |y|) is exact.  Strict: an equal a keeps the earlier
// index.  A NaN part never updates (both comparisons are false).  live == false: the lane is frozen (it escaped at or before z_m).
MC_ATOM_FN void update(double& best, uint32_t& period, uint32_t m, double x, double y, bool live = true) {
    const double ax = __builtin_fabs(x), ay = __builtin_fabs(y);
    const double a = ax > ay ? ax : ay;
    const bool take = live && ax < best && ay < best;
    best = take ? a : best;
    period = take ? m : period;
}

}  // namespace atom
}  // namespace mc

#if defined(__HIPCC__)
#include "mc_internal.h"

namespace mc {

// What escape_time latches for an atom instantiation.  latch() runs after every EXACT step, and an atom state has no other kind
// (ExactSteps below), so its call count m is the iteration's index: the z of the call is z_m.  The lane freezes at its first escape, as
// EscapeCapture does: z_m of the escaping iteration and everything after it stay out (the contract's m runs to n).  m is wave-uniform.
struct AtomCapture {
    double best = __builtin_inf();
    uint32_t period = 0u, m = 0u;
    bool frozen = false;
    template <class State>
    __device__ __forceinline__ void latch(bool escaped, const State& st) {
        double x, y;
        st.escape_z(x, y);
        m = m + 1u;
        frozen = frozen || escaped;
        atom::update(best, period, m, x, y, !frozen);
    }
};

// A state without its fast block: every iteration is an exact step, which is where the capture hook runs.  (A fast block that carries the
// minimum through its accumulator is an optimisation left out: DESIGN.md §3.33.)  Everything else is the state's own: init, step, the
// cycle exit's same_z and kCycleCheckBlocks, the block length.
template <class State>
struct ExactSteps : State {
    static constexpr bool kHasFastBlock = false;
};

// The atom kernels' two planes beside the target's out_iters (either may be null), row-major over the whole image.
struct AtomOut {
    uint32_t* __restrict__ period;
    double* __restrict__ amin;
};

// mandelbrot.hip: every check of mc_mandelbrot_render_atom's request, then F32 / F64 here and PERTURB through perturb_atom_launch
// (mandel_perturb.hip: the binding's checks and the dc table).
int mandelbrot_atom_launch(mc_context* ctx, const mc_mandelbrot_params* p, void* d_iters, void* d_period, void* d_amin, hipStream_t s);
int perturb_atom_launch(mc_context* ctx, const mc_mandelbrot_params* p, void* d_iters, const AtomOut& o, hipStream_t s);

}  // namespace mc
#endif
