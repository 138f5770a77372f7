// MC_MANDEL_COLOUR_SMOOTH: the fractional escape count and its colour (include/mc_compute.h states the contract).
//
// One body for the host and the device.  smooth_count continues a pixel's orbit from its escape state in IEEE double until |z|^2 > 65536
// (at most 64 iterations), takes the two strict fp32 log2 of the fraction and packs (count, fraction) as 24.8 fixed point; smooth_colour
// interpolates between two neighbouring entries of the colour table.  Every precision's kernel hands over (n, z, c) as doubles and runs
// this one function, so no precision has a second recurrence.  mc_mandelbrot_smooth_count / mc_mandelbrot_smooth_colour call the same
// functions on the host.  The flag's refusals and the launcher's declaration are host code: mandel_smooth_host.h.
//
// log2f32 is mc_log2 of mc_math.h, op for op.  It is restated here, not included: mc_math.h is device-only and part of the path tracer's
// build identity, which a Mandelbrot feature must not move.
// Requires -ffp-contract=off (the explicit __builtin_fmaf calls are the only fused operations).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MC_SMOOTH_FN __host__ __device__ inline
#else
#define MC_SMOOTH_FN inline
#endif

namespace mc {
namespace smooth {

constexpr uint32_t kMaxIter = 0x00ffffffu;   // 256 * max_iter must fit the plane's uint32_t (q is formed in 64 bits and clamped below it)
constexpr uint32_t kTailCap = 64u;           // the continuation's iteration cap
constexpr double kRadius2 = 65536.0;         // the continuation's threshold on |z|^2 (radius 256)

MC_SMOOTH_FN float as_float(uint32_t u) { return __builtin_bit_cast(float, u); }
MC_SMOOTH_FN uint32_t as_uint(float f) { return __builtin_bit_cast(uint32_t, f); }

// mc_log2 (mc_math.h), op for op
MC_SMOOTH_FN float log2f32(float x) {
    if (x == 0.0f) return -__builtin_inff();
    int e_adj = 0;
    if (x < 1.17549435e-38f) { x = x * 16777216.0f; e_adj = -24; }
    uint32_t u = as_uint(x);
    int e = (int)(u >> 23) - 127;
    float m = as_float((u & 0x007fffffu) | 0x3f800000u);
    if (m > 1.41421356237f) { m = m * 0.5f; e += 1; }
    float t = m - 1.0f;
    float z = t * t;
    float p = __builtin_fmaf(7.0376836292e-2f, t, -1.1514610310e-1f);
    p = __builtin_fmaf(p, t, 1.1676998740e-1f);
    p = __builtin_fmaf(p, t, -1.2420140846e-1f);
    p = __builtin_fmaf(p, t, 1.4249322787e-1f);
    p = __builtin_fmaf(p, t, -1.6668057665e-1f);
    p = __builtin_fmaf(p, t, 2.0000714765e-1f);
    p = __builtin_fmaf(p, t, -2.4999993993e-1f);
    p = __builtin_fmaf(p, t, 3.3333331174e-1f);
    float ln = __builtin_fmaf(t * z, p, __builtin_fmaf(-0.5f, z, t));
    const float LOG2E_HI = 1.44269502162933349609375f;
    const float LOG2E_LO = 1.92596299112661746e-8f;
    float r = __builtin_fmaf(ln, LOG2E_LO, 0.0f);
    r = __builtin_fmaf(ln, LOG2E_HI, r);
    return r + (float)(e + e_adj);
}

// q of include/mc_compute.h: n the pixel's count, (zx, zy) the z of the iteration that escaped, (cx, cy) the pixel's c.  max_iter <= kMaxIter.
MC_SMOOTH_FN uint32_t smooth_count(uint32_t n, uint32_t max_iter, double zx, double zy, double cx, double cy) {
    if (n >= max_iter) return 256u * max_iter;
    uint32_t k = 0u;
    double r = (zx * zx) + (zy * zy);
    while (!(r > kRadius2) && k < kTailCap) {   // a NaN keeps running to the cap
        const double t = ((zx * zx) - (zy * zy)) + cx;
        zy = ((2.0 * zx) * zy) + cy;
        zx = t;
        k++;
        r = (zx * zx) + (zy * zy);
    }
    float rf = (float)r;                          // round to nearest even
    if (!(rf > 65536.0f)) rf = 65536.0f;          // the cap was hit, or NaN
    if (rf > 3.402823466e+38f) rf = 3.402823466e+38f;   // inf
    const float l = log2f32(rf);
    const float s = l * 0.0625f;
    float t = log2f32(s);
    if (!(t > 0.0f)) t = 0.0f;
    if (t > 1.0f) t = 1.0f;
    const uint32_t f = (uint32_t)(256.0f * (1.0f - t));   // 0 .. 256
    const uint64_t q = 256u * (uint64_t)(n + k) + f, top = 256u * (uint64_t)max_iter - 1u;
    return (uint32_t)(q < top ? q : top);
}

// The colour of q (q <= 256 * max_iter) from the (max_iter + 1)-entry vec4 table of mc_mandelbrot_colour_lut.
MC_SMOOTH_FN void smooth_colour(uint32_t q, uint32_t max_iter, const float* lut, float out[4]) {
    if (q == 256u * max_iter) {
        for (int c = 0; c < 4; c++) out[c] = lut[4u * (size_t)max_iter + c];
        return;
    }
    const uint32_t idx = q >> 8, fr = q & 255u;
    const float w = (float)fr * 0.00390625f;
    const float* a = lut + 4u * (size_t)idx;
    const float* b = a + 4;
    for (int c = 0; c < 3; c++) out[c] = a[c] + ((b[c] - a[c]) * w);
    out[3] = 1.0f;
}

}  // namespace smooth
}  // namespace mc

#if defined(__HIPCC__)
#include "mandel_target.h"

namespace mc {

// What escape_time (mandel_escape.h) latches for a smooth instantiation: z of the lane's FIRST escape.  Lanes keep iterating after they
// escape, so the state at return is not the escape state; escapes are only ever detected in exact steps, which is where latch() is called.
// A State offers escape_z(zx, zy): the z its last step() tested, as doubles.
struct EscapeCapture {
    double zx = 0.0, zy = 0.0;
    bool have = false;
    template <class State>
    __device__ __forceinline__ void latch(bool escaped, const State& st) {
        double x, y;
        st.escape_z(x, y);
        const bool take = escaped && !have;
        zx = take ? x : zx;
        zy = take ? y : zy;
        have = have || escaped;
    }
};

// tile_store for a smooth instantiation: n into the count planes, q into out_smooth, the interpolated vec4 into out_rgba (any may be null).
// n_plane is what the count planes receive (n, or a BLA kernel's trip count).
template <class Target>
__device__ __forceinline__ void smooth_tile_store(const Target& t, const TileLane& ln, uint32_t* __restrict__ out_smooth, uint32_t n,
                                                  uint32_t n_plane, double zx, double zy, double cx, double cy) {
    if (ln.valid) {
        const size_t idx = (size_t)ln.ty * t.W + ln.gx;
        const uint32_t q = smooth::smooth_count(n, t.max_iter, zx, zy, cx, cy);
        if (t.out_iters) t.out_iters[idx] = n_plane;
        if (t.out_iters16) t.out_iters16[idx] = (uint16_t)n_plane;
        if (out_smooth) out_smooth[idx] = q;
        if (t.out_rgba) {
            float v[4];
            smooth::smooth_colour(q, t.max_iter, reinterpret_cast<const float*>(t.lut), v);
            t.out_rgba[idx] = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

}  // namespace mc
#endif
