// Path-tracer denoiser, the noise plane and the colour weight it steers (include/mc_compute.h states the contract, at mc_pathtrace_noise /
// mc_pathtrace_denoise_adaptive; tests/pt_noise_ref.py restates it in numpy).
//
// One body for the host and the device, as pt_denoise.h, whose filter_pixel the noise-guided filter runs unchanged: only the colour
// weight handed to it differs.  pt_noise_v_kernel / pt_noise_window_kernel / pt_denoise_adaptive_pass_kernel (pt_noise.hip) and
// mc_pathtrace_noise / mc_pathtrace_denoise_adaptive run these same functions.  Every operation is ONE IEEE-754 fp32 operation in the
// order written (fma only where written as fma).  Requires -ffp-contract=off.
//
// THE CONTRACT, noise plane (W x H, storage order; half: the linear accumulator after samples [0, h); full: the finished, encoded buffer):
//   per pixel q and c in r, g, b:   x = half[q].c * scale;   cl = min(max(x, 0), 1)  with  max(x, 0) = x < 0 ? 0 : x,  min(y, 1) = 1 < y ? 1 : y;
//     E = pow045(cl) * 255 + 0.5  (pathTracer.comp:453 as the strict kernels perform it: pow045(c) = exp2(0.45f * log2(c)));   e_c = E - full[q].c
//     v_q = (e_r*e_r + e_g*e_g) + e_b*e_b
//   per pixel p = (x, y):  sum = cnt = 0;  taps q = (x + a, y + b) in row-major order (b = -radius .. radius outer, a likewise inner), taps
//     outside the image skipped:  sum = sum + v_q;  cnt = cnt + 1.0f.   V_p = sum / cnt.
// THE CONTRACT, noise-guided filter: pt_denoise.h's with  kc_i(p) = (float)4^i / ((k_noise * k_noise) * V_p + 1.0f)  at the centre pixel.
// log2 and exp2 are mc_math.h's strict ones restated operation for operation (exp2: pt_denoise.h's), so that mc_math.h and with it the
// path tracer's build id stay as they are.
#pragma once
#include "pt_denoise.h"

namespace mc {
namespace ptd {

constexpr uint32_t kMaxNoiseRadius = 4;

// mc_math.h's strict mc_log2, operation for operation.
MC_PTD_FN float log2_strict(float x) {
    if (x == 0.0f) return -__builtin_inff();
    int e_adj = 0;
    if (x < 1.17549435e-38f) { x = x * 16777216.0f; e_adj = -24; }
    const uint32_t u = __builtin_bit_cast(uint32_t, x);
    int e = (int)(u >> 23) - 127;
    float m = __builtin_bit_cast(float, (u & 0x007fffffu) | 0x3f800000u);
    if (m > 1.41421356237f) { m = m * 0.5f; e += 1; }
    const float t = m - 1.0f;
    const float z = t * t;
    float p = __builtin_fmaf(7.0376836292e-2f, t, -1.1514610310e-1f);
    p = __builtin_fmaf(p, t, 1.1676998740e-1f);
    p = __builtin_fmaf(p, t, -1.2420140846e-1f);
    p = __builtin_fmaf(p, t, 1.4249322787e-1f);
    p = __builtin_fmaf(p, t, -1.6668057665e-1f);
    p = __builtin_fmaf(p, t, 2.0000714765e-1f);
    p = __builtin_fmaf(p, t, -2.4999993993e-1f);
    p = __builtin_fmaf(p, t, 3.3333331174e-1f);
    const float ln = __builtin_fmaf(t * z, p, __builtin_fmaf(-0.5f, z, t));
    const float LOG2E_HI = 1.44269502162933349609375f;
    const float LOG2E_LO = 1.92596299112661746e-8f;
    float r = __builtin_fmaf(ln, LOG2E_LO, 0.0f);
    r = __builtin_fmaf(ln, LOG2E_HI, r);
    return r + (float)(e + e_adj);
}

// The final encode of one linear component (pathTracer.comp:453, pathtrace_kernel.h's strict instantiation).
MC_PTD_FN float encode_strict(float x) {
    const float lo = (x < 0.0f) ? 0.0f : x;
    const float cl = (1.0f < lo) ? 1.0f : lo;
    return exp2_strict(0.45f * log2_strict(cl)) * 255.0f + 0.5f;
}

// v_q: the squared distance between the half render, encoded as if it were the whole, and the whole render.
MC_PTD_FN float noise_pixel(vec4 half, float scale, vec4 full) {
    const float er = encode_strict(half.x * scale) - full.x;
    const float eg = encode_strict(half.y * scale) - full.y;
    const float eb = encode_strict(half.z * scale) - full.z;
    return (er * er + eg * eg) + eb * eb;
}

// V_p: the mean of v over the window clipped to the image.
MC_PTD_FN float noise_window(uint32_t W, uint32_t H, uint32_t x, uint32_t y, int radius, const float* v) {
    float sum = 0.0f, cnt = 0.0f;
    for (int b = -radius; b <= radius; b++) {
        const int64_t qy = (int64_t)y + b;
        if (qy < 0 || qy >= (int64_t)H) continue;
        for (int a = -radius; a <= radius; a++) {
            const int64_t qx = (int64_t)x + a;
            if (qx < 0 || qx >= (int64_t)W) continue;
            sum = sum + v[(size_t)qy * W + (size_t)qx];
            cnt = cnt + 1.0f;
        }
    }
    return sum / cnt;
}

// kc_i(p): scale4 = (float)4^i, k2 = k_noise * k_noise (both formed once per pass, on the host).
MC_PTD_FN float colour_weight_adaptive(float scale4, float k2, float variance) { return scale4 / (k2 * variance + 1.0f); }

inline void noise_host(uint32_t W, uint32_t H, const vec4* half, float scale, const vec4* full, uint32_t radius, float* out_variance) {
    const size_t npix = (size_t)W * H;
    std::vector<float> v(npix);
    for (size_t q = 0; q < npix; q++) v[q] = noise_pixel(half[q], scale, full[q]);
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++) out_variance[(size_t)y * W + x] = noise_window(W, H, x, y, (int)radius, v.data());
}

// The whole noise-guided filter on the host: out may be rgba.  passes in 1 .. kMaxPasses.
inline void denoise_adaptive_host(uint32_t W, uint32_t H, uint32_t passes, float k_noise, float kn, float kx, const vec4* rgba, const vec4* normal_t,
                                  const vec4* position_id, const float* variance, vec4* out) {
    const size_t npix = (size_t)W * H;
    const float k2 = k_noise * k_noise;
    std::vector<vec4> tmp[2];
    const vec4* src = rgba;
    for (uint32_t i = 0; i < passes; i++) {
        std::vector<vec4>& dst = tmp[i & 1u];
        dst.resize(npix);
        const float scale4 = (float)(1u << (2u * i));
        for (uint32_t y = 0; y < H; y++)
            for (uint32_t x = 0; x < W; x++) {
                const size_t p = (size_t)y * W + x;
                dst[p] = filter_pixel(W, H, x, y, 1u << i, colour_weight_adaptive(scale4, k2, variance[p]), kn, kx, src, normal_t, position_id, src[p],
                                      normal_t[p], position_id[p]);
            }
        src = dst.data();
    }
    for (size_t p = 0; p < npix; p++) out[p] = src[p];
}

}  // namespace ptd
}  // namespace mc
