// MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE: the refine rule over smooth counts (include/mc_compute.h states the contract).
//
// One body for the host and the device: mandel_refine_smooth_kernel (mandel_refine_smooth.hip), mc_mandelbrot_refine_smooth and
// tools/mandel_refine_smooth_host_check.cpp run these same functions.  Integer arithmetic only.
//   a(y, x) = min(A(y, x), 256 M)                       A: the anchor plane, the plain smooth W x H render's q plane
//   refined(y, x) <=> |a(y, x) - a(y', x')| > tau       for one of the up to eight neighbours (y', x') inside the image
// The difference is formed without wrap.  tau = 0 is "differs at all"; tau >= 256 M refines nothing (no two clamped values are further
// apart); an interior neighbour is just the value 256 M.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MC_REFINE_FN __host__ __device__ inline
#else
#define MC_REFINE_FN inline
#endif

namespace mc {
namespace refine_smooth {

constexpr uint32_t kDefaultThreshold = 256u;   // tau of the calls that take none: one iteration

MC_REFINE_FN uint32_t clamped(uint32_t q, uint32_t top) { return q < top ? q : top; }
MC_REFINE_FN bool apart(uint32_t a, uint32_t b, uint32_t tau) { return (a > b ? a - b : b - a) > tau; }

// The rule for pixel (y, x) of the W x H plane (y < H, x < W); top = 256 * max_iter.  The pixel itself is among the nine reads and
// never counts (its difference is 0).
MC_REFINE_FN bool refined(const uint32_t* plane, uint32_t W, uint32_t H, uint32_t y, uint32_t x, uint32_t top, uint32_t tau) {
    const uint32_t a = clamped(plane[(size_t)y * W + x], top);
    const uint32_t y0 = y ? y - 1u : 0u, y1 = y + 1u < H ? y + 1u : y;
    const uint32_t x0 = x ? x - 1u : 0u, x1 = x + 1u < W ? x + 1u : x;
    bool r = false;
    for (uint32_t yy = y0; yy <= y1; yy++)
        for (uint32_t xx = x0; xx <= x1; xx++) r |= apart(a, clamped(plane[(size_t)yy * W + xx], top), tau);
    return r;
}

// The whole plane on the host: mask (W * H bytes of 0 / 1, or null) and the number of refined pixels.
inline uint64_t refine_plane(uint32_t W, uint32_t H, uint32_t max_iter, const uint32_t* plane, uint32_t tau, uint8_t* mask) {
    const uint32_t top = 256u * max_iter;
    uint64_t count = 0;
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++) {
            const bool r = refined(plane, W, H, y, x, top, tau);
            if (mask) mask[(size_t)y * W + x] = r ? 1u : 0u;
            count += r ? 1u : 0u;
        }
    return count;
}

}  // namespace refine_smooth
}  // namespace mc
