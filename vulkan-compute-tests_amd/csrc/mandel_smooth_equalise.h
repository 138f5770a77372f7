// MC_MANDEL_COLOUR_SMOOTH_EQUALISED: the rank map over fractional counts (include/mc_compute.h states the contract).
//
// One body for the host and the device.  The smooth plane's histogram is keyed by q >> 8; the knot map places knot j at the palette
// position 256 M C(j) / E, the share of escaped pixels below count j in 24.8 fixed point; remap moves a q linearly between the two knots
// around it.  Integer arithmetic only: mandel_smooth_remap_kernel (mandel_smooth_equalise.hip) and mc_mandelbrot_smooth_equalise_map /
// mc_mandelbrot_smooth_remap run these same functions.  The colour is smooth::smooth_colour of the remapped count.  The flag's refusals
// and the launchers' declarations are host code: mandel_smooth_equalise_host.h.
#pragma once
#include <cstdint>

#include "mandel_smooth.h"

namespace mc {
namespace smooth_equalise {

// qmap[max_iter + 1] from hist[max_iter + 1] (bins of q >> 8, bin max_iter the interior).  false: the total exceeds 2^32 - 1.
inline bool knot_map(uint32_t max_iter, const uint32_t* hist, uint32_t* qmap) {
    uint64_t total = 0;
    for (uint64_t j = 0; j <= max_iter; j++) total += hist[j];
    if (total > 0xffffffffull) return false;
    const uint64_t escaped = total - hist[max_iter];
    const uint64_t top = 256u * (uint64_t)max_iter;   // below 2^32; top * below < 2^32 * 2^32
    uint64_t below = 0;
    for (uint32_t j = 0; j < max_iter; j++) {
        qmap[j] = escaped ? (uint32_t)((top * below) / escaped) : 0u;
        below += hist[j];
    }
    qmap[max_iter] = (uint32_t)top;
    return true;
}

// pairs[2 j], pairs[2 j + 1] = (qmap[j], qmap[j + 1] - qmap[j]) for j < max_iter: what remap gathers, one aligned 8-byte entry per bin.
inline void compose_pairs(uint32_t max_iter, const uint32_t* qmap, uint32_t* pairs) {
    for (uint32_t j = 0; j < max_iter; j++) {
        pairs[2u * (size_t)j] = qmap[j];
        pairs[2u * (size_t)j + 1u] = qmap[j + 1] - qmap[j];
    }
}

// q' of a q below 256 * max_iter from its pair (qmap[j], qmap[j + 1] - qmap[j]), j = q >> 8.
MC_SMOOTH_FN uint32_t remap_pair(uint32_t q, uint32_t knot, uint32_t step) {
    return knot + (uint32_t)(((uint64_t)step * (q & 255u)) >> 8);
}

// q' of any q: 256 * max_iter (interior) at and above it.  pairs: max_iter entries of (knot, step).
MC_SMOOTH_FN uint32_t remap(uint32_t q, uint32_t max_iter, const uint32_t* pairs) {
    const uint32_t top = 256u * max_iter;
    if (q >= top) return top;
    const uint32_t j = q >> 8;
    return remap_pair(q, pairs[2u * (size_t)j], pairs[2u * (size_t)j + 1u]);
}

}  // namespace smooth_equalise
}  // namespace mc
