// MC_MANDEL_COLOUR_DISTANCE: the boundary distance estimate from the smooth-count plane, and its shading (include/mc_compute.h states the
// contract).
//
// One body for the host and the device.  The smooth count nu = q / 256 is the potential in disguise (G ~ 2^-nu), so the exterior estimate
// d ~ 2 G / |grad G| is 2 / (ln 2 |grad nu|): a function of the q plane alone, by finite differences between neighbouring pixels, in pixel
// pitches at every zoom depth.  distance_px takes a pixel's q and its four neighbours'; distance_colour dims the smooth colour of q by
// min(D / T, 1).  mandel_distance_kernel (mandel_distance.hip) and mc_mandelbrot_distance_plane / mc_mandelbrot_distance_colour run these
// same functions.  The flag's refusals and the launcher's declaration are host code: mandel_distance_host.h.
// Requires -ffp-contract=off, and the compiler's correctly rounded fp64 sqrt and division and fp32 division (no fast-math flag).
#pragma once
#include <cstdint>

#include "mandel_smooth.h"

namespace mc {
namespace distance {

constexpr double kScale = 1477.3197218702985;   // 1024 / ln 2: the central difference spans two pixels, q carries 8 fractional bits
constexpr float kFlat = 4096.0f;                // D where both differences are zero: above kScale, the largest value a gradient gives

// d(+1) - d(-1) along one axis, as the contract takes it: central where both neighbours exist, the one-sided difference doubled at a border,
// 0 on an axis of one pixel.
MC_SMOOTH_FN int64_t difference(uint32_t c, uint32_t lo, uint32_t hi, bool has_lo, bool has_hi) {
    if (has_lo && has_hi) return (int64_t)hi - (int64_t)lo;
    if (has_hi) return 2 * ((int64_t)hi - (int64_t)c);
    if (has_lo) return 2 * ((int64_t)c - (int64_t)lo);
    return 0;
}

// D of a pixel with smooth count c; l, r, u, d: its left, right, upper and lower neighbours' (storage rows), read only where has_* says the
// neighbour is inside the image.  interior = 256 * max_iter.
MC_SMOOTH_FN float distance_px(uint32_t interior, uint32_t c, uint32_t l, uint32_t r, uint32_t u, uint32_t d, bool has_l, bool has_r,
                               bool has_u, bool has_d) {
    if (c == interior) return 0.0f;
    if ((has_l && l == interior) || (has_r && r == interior) || (has_u && u == interior) || (has_d && d == interior)) return 0.0f;
    const int64_t gx = difference(c, l, r, has_l, has_r), gy = difference(c, u, d, has_u, has_d);
    const double a = (double)gx, b = (double)gy;
    const double g2 = (a * a) + (b * b);
    if (g2 == 0.0) return kFlat;
    return (float)(kScale / __builtin_sqrt(g2));
}

// D of pixel (y, x) of the dense W x H plane q.
MC_SMOOTH_FN float distance_at(const uint32_t* q, uint32_t W, uint32_t H, uint32_t max_iter, uint32_t y, uint32_t x) {
    const size_t i = (size_t)y * W + x;
    const bool has_l = x > 0u, has_r = x + 1u < W, has_u = y > 0u, has_d = y + 1u < H;
    return distance_px(256u * max_iter, q[i], has_l ? q[i - 1] : 0u, has_r ? q[i + 1] : 0u, has_u ? q[i - W] : 0u, has_d ? q[i + W] : 0u,
                       has_l, has_r, has_u, has_d);
}

// The shaded colour: lut[max_iter] for an interior pixel, else the smooth colour of q with rgb scaled by w = D >= T ? 1 : D / T.
MC_SMOOTH_FN void distance_colour(uint32_t q, float D, float T, uint32_t max_iter, const float* lut, float out[4]) {
    smooth::smooth_colour(q, max_iter, lut, out);
    if (q == 256u * max_iter) return;
    const float w = D >= T ? 1.0f : D / T;
    for (int c = 0; c < 3; c++) out[c] = out[c] * w;
    out[3] = 1.0f;
}

}  // namespace distance
}  // namespace mc
