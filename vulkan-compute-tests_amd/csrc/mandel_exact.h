// mc_mandelbrot_exact_counts_device (mandel_exact.hip): what the rest of the library calls, and how a launch is sized.
#pragma once
#include <cstdint>

struct mc_context;

namespace mc {

// Iterations per launch for n limbs and n_pixels pixels on a device of `cus` compute units, clamped to [1, 65536]: a launch stays near
// the orbit kernel's 50 ms (kOrbitLaunchWork, mandel_perturb.h).
//  * n >= 17, one workgroup per pixel: orbit_launch_iters' kOrbitLaunchWork / n^2 divided by the rounds the grid needs at one
//    workgroup per CU.
//  * n <= 16, one wave per pixel: 50 ms over (the time of one iteration of a round of kExactWavesPerCu waves on every CU) x rounds.
//    That time is a linear fit, Ns0 + Ns1 * n, to what profiles/mandel_exact_probe.txt measured on an MI355X with 4096 pixels on 256
//    CUs, 16 waves per CU, every pixel running M: 4.681 us at 3 limbs, 5.639 at 8, 7.307 at 16 (the line gives 4.68, 5.69, 7.31).
//    DESIGN.md section 3.31 has the table.
constexpr uint64_t kExactWaveLaunchNs = 50000000ull;
constexpr uint64_t kExactWavesPerCu = 16;
constexpr uint64_t kExactWaveIterNs0 = 4075, kExactWaveIterNs1 = 202;   // ns per iteration of a round: Ns0 + Ns1 * n
uint32_t exact_launch_iters(int n, uint64_t n_pixels, uint32_t cus);

// mc_context_destroy: the context's exact-count state, count words and events are freed.
void exact_device_release(mc_context* ctx);

}  // namespace mc
