// Device math for the path tracer, in two flavours selected at compile time by `Fast`:
//
//  strict (Fast = 0): every operation is one IEEE-754 fp32 operation (correctly rounded +,-,*,/,
//     sqrt, fma) in a FIXED order, so results are bit-identical to a CPU evaluating the same sequence
//     (DESIGN.md §"mc math").  GLSL leaves sin/cos/pow/inversesqrt precision implementation-defined
//     (SURVEY.md H5); these algorithms are this build's canonical choice for them:
//        inversesqrt(x) := 1.0f / sqrt(x)
//        sin/cos        := Cody–Waite pi/2 reduction + cephes sinf/cosf kernels (fmaf form)
//        pow(x, y)      := exp2(y * log2(x)) with cephes-style logf/exp2f kernels (fmaf form)
//  fast (Fast = 1): gfx950 hardware approximations — v_rcp_f32, v_rsq_f32, v_sqrt_f32,
//     v_sin_f32/v_cos_f32 (input in revolutions), v_exp_f32/v_log_f32.  ~1 ulp each; toleranced parity.
//  careful (Fast = 2; the fast mode's second tier, include/mc_compute.h MC_PT_MATH_FAST_CAREFUL): division, square root and reciprocal
//     square root ROUNDED AS THE REFERENCE ROUNDS THEM — the strict mode's short forms (one hardware seed + 3 .. 7 ordinary
//     instructions) without their window tests; hardware sine / cosine / exp / log as in the fast tier.  Every fast-math shortcut
//     that is an identity of exact arithmetic stays; the translation unit that instantiates it does not contract.  A path then differs
//     from the reference's by far fewer roundings, and forks correspondingly less often (profiles/r05_fork_census*.txt).
//  `Fast` is an int so that `if (Fast)` keeps meaning "not strict".
//
// Requires -ffp-contract=off (explicit __builtin_fmaf calls are the only fused operations).
#pragma once
#include <hip/hip_runtime.h>

namespace mc {
namespace dm {

__device__ __forceinline__ float as_float(uint32_t u) { return __uint_as_float(u); }
__device__ __forceinline__ uint32_t as_uint(float f) { return __float_as_uint(f); }
// v, negated where the sign bit of s is CLEAR: bits(v) ^ (~bits(s) & 0x80000000) as ONE v_bitop3_b32 (truth table 0xc6: b ^ (~a & c)).
// Written with the builtin so that the three inputs stay one instruction at every use: from the spelled-out form the compiler forms
// the flip word ~bits(s) & 0x80000000 once, holds it in a register and pays a v_xor per use besides.
__device__ __forceinline__ float flip_where_sign_clear(float v, float s) {
#if defined(__HIP_DEVICE_COMPILE__)
    return as_float(__builtin_amdgcn_bitop3_b32(as_uint(s), as_uint(v), 0x80000000u, 0xc6));
#else
    return as_float(as_uint(v) ^ (~as_uint(s) & 0x80000000u));
#endif
}

// max(v, 0) as the single v_max_f32 the compiler emits for fmaxf(v, 0.0f) of an arithmetic result — for a v it cannot see the origin of.
// Why it is written out: in front of fmaxf of a value that comes out of a bit operation (flip_where_sign_clear) the compiler puts a
// canonicalising v_max_f32 v, v, v — seen with AMD clang 22.0.0git (roc-7.2.0, HIP 7.2.26015); __builtin_amdgcn_fmed3f(v, 0, inf) was
// folded back into the same pair.  The optimiser cannot see through the asm: when a compiler emits the single instruction for
// fmaxf(flip_where_sign_clear(..), 0.0f) by itself (`make asm`, the light contribution of pathtrace_pool_kernel), this goes.
// Device code only (its one caller is the sample-pool kernel).
__device__ __forceinline__ float max_zero_as_is(float v) {
    float r;
    asm("v_max_f32_e32 %0, 0, %1" : "=v"(r) : "v"(v));
    return r;
}

// ---- IEEE primitives ------------------------------------------------------------------------------
// hipcc's default for HIP is correctly-rounded fp32 divide and sqrt (-fhip-fp32-correctly-rounded-divide-sqrt);
// the parity tests (tests/test_gpu_parity.py::test_mc_math_bit_exact) verify both against the host bit for bit.
__device__ __forceinline__ float ieee_div(float a, float b) { return a / b; }
__device__ __forceinline__ float ieee_sqrt(float a) { return __builtin_sqrtf(a); }

// Short forms of the correctly rounded sqrt and reciprocal for arguments in [2^-100, 2^100): no operand scaling, no
// special-case fix-up, so 5 and 3 instructions (one transcendental each) instead of the compiler's 16 and 11.  Correct rounding is a property of the
// gfx950 v_sqrt/v_rsq/v_rcp seeds, established by enumeration, not by argument: tools/exact_math_exhaustive.hip and
// tests/test_gpu_parity.py::test_short_forms_exhaustive compare EVERY fp32 bit pattern with the IEEE expansions
// (sqrt clean for 2^-102 <= x < 2^128, 1/x for 2^-126 <= x < 2^126; profiles/r02_exact_math_exhaustive.txt).
// Outside the window — zero, denormals, inf, NaN, negatives — the wave takes the compiler's expansion, so the
// functions are correctly rounded everywhere.  The test is wave-wide (one compare, one scalar branch).
__device__ __forceinline__ bool in_short_window(float x) { return (as_uint(x) - 0x0D800000u) < 0x64000000u; }   // 2^-100 <= x < 2^100
__device__ __forceinline__ bool wave_all(bool p) { return __builtin_amdgcn_ballot_w64(!p) == 0ull; }            // over the active lanes
__device__ __forceinline__ float sqrt_short(float x) {
    float y = __builtin_amdgcn_rsqf(x);                      // the one transcendental
    float g = x * y;                                         // sqrt(x) within ~1.5 ulp
    float d = __builtin_fmaf(-g, g, x);                      // exact residual
    return __builtin_fmaf(d, 0.5f * y, g);
}
__device__ __forceinline__ float rcp_short(float b) {
    float r = __builtin_amdgcn_rcpf(b);
    float e = __builtin_fmaf(-b, r, 1.0f);
    return __builtin_fmaf(e, r, r);
}

// inversesqrt(x) := RN(1 / RN(sqrt(x))) (two roundings: the definition above) with ONE transcendental: the correctly rounded root s as in
// sqrt_short, then one Newton step on 1 / s seeded with the v_rsq_f32 value already at hand instead of a second seed from v_rcp_f32
// (a transcendental costs 13 issue cycles among other instructions, profiles/r04_no_trans_pmc.txt).  The step lands on the correctly
// rounded quotient everywhere in the window except where s = 2 - ulp (x = 4 - 1 ulp and 4 - 2 ulp of every second binade): there 1 / s =
// 0.5 + 2^-25 + ... sits just above a round-to-even tie that no step from below leaves (profiles/r02_exact_math_exhaustive.txt, "rsq only,
// 1 step on 1/s from y": exactly these two patterns per binade pair) — those two get their ulp added by an integer test on x's bits.
// Established like the other short forms: EVERY fp32 pattern of the window compared with the IEEE expansion on the device
// (tests/test_gpu_parity.py::test_short_forms_exhaustive, fn 5; profiles/r04_exact_rsqrt_one_trans.txt).
__device__ __forceinline__ float rsqrt_short(float x) {
    const float y = __builtin_amdgcn_rsqf(x);
    const float g = x * y;
    const float d = __builtin_fmaf(-g, g, x);
    const float s = __builtin_fmaf(d, 0.5f * y, g);           // = sqrt_short(x)
    const float e = __builtin_fmaf(-s, y, 1.0f);
    const float r = __builtin_fmaf(e, y, y);
    const uint32_t tie = ((as_uint(x) & 0x00fffffeu) == 0x007ffffeu) ? 1u : 0u;   // even biased exponent, mantissa 0x7ffffe / 0x7fffff
    return as_float(as_uint(r) + tie);
}

// Short division for numerators that share a positive divisor s (a colour divided by a probability, by pi, by the sample
// count): with y = RN(1/s),  q0 = a*y; r = fma(-s, q0, a); q = fma(r, y, q0)  IS the correctly rounded a/s for every pair of
// normal operands while nothing over- or underflows — all 2^23 x 2^23 mantissa pairs enumerated against the IEEE expansion,
// tools/exact_div_exhaustive.hip, profiles/r02_exact_div_exhaustive.txt: 7.04e13 divisions, 0 mismatches — and for a = +0.
// Window: s in [2^-60, 2^60), every numerator +0 or in [2^-60, 2^60) (quotient, residual and reciprocal stay normal); anything
// else — negative, -0, denormal, inf, NaN — is redone by the compiler's expansion (per lane; no render has such a lane).
// 3 instructions per numerator instead of 11, after one reciprocal (rcp_short, or a constant / host-computed RN(1/s)).
// 0x21800000 = 2^-60, 0x5D800000 = 2^60 as bit patterns; the window test is three unsigned compares (div3 below).
__device__ __forceinline__ float div_step(float a, float s, float y) {
    const float q0 = a * y;
    const float r = __builtin_fmaf(-s, q0, a);
    return __builtin_fmaf(r, y, q0);
}

// The careful tier (Fast == 2): the short forms of the strict mode (correct rounding enumerated over every fp32 pattern of their
// windows, see sqrt_short / rcp_short / div_step / rsqrt_short above) without the strict mode's window tests: outside the windows
// (denormal, infinite, NaN arguments — no finite path produces one) the result is merely inaccurate, and the one argument a path does
// produce there, an exact zero under a square root, is selected per lane.
template <int Fast> __device__ __forceinline__ float fdiv(float a, float b) {
    if (Fast == 2) return div_step(a, b, rcp_short(b));
    if (Fast) return a * __builtin_amdgcn_rcpf(b);
    return ieee_div(a, b);
}
// (a0, a1, a2) / s.  Strict: the short division inside its window (wave-wide test), the compiler's IEEE expansion outside.
// HaveY: the caller supplies y = RN(1/s) — a constant or a host-computed kernel argument — instead of rcp_short(s).
template <int Fast, bool HaveY> __device__ __forceinline__ void div3(float& a0, float& a1, float& a2, float s, float y) {
    if constexpr (!Fast) {
        // the short form for every lane; the lanes outside the window (never seen in a render) redo it the long way
        const uint32_t b0 = as_uint(a0), b1 = as_uint(a1), b2 = as_uint(a2);
        uint32_t hi = b0 > b1 ? b0 : b1; hi = hi > b2 ? hi : b2;                           // v_max3_u32
        const uint32_t l0 = b0 - 1u, l1 = b1 - 1u, l2 = b2 - 1u;                           // +0 wraps to 0xffffffff: passes
        uint32_t lo = l0 < l1 ? l0 : l1; lo = lo < l2 ? lo : l2;                           // v_min3_u32
        const bool outside = ((as_uint(s) - 0x21800000u) >= 0x3C000000u) | (hi >= 0x5D800000u) | (lo < 0x21800000u - 1u);
        if constexpr (!HaveY) y = rcp_short(s);
        const float q0 = div_step(a0, s, y), q1 = div_step(a1, s, y), q2 = div_step(a2, s, y);
        if (__builtin_expect(outside, 0)) { a0 = ieee_div(a0, s); a1 = ieee_div(a1, s); a2 = ieee_div(a2, s); }
        else { a0 = q0; a1 = q1; a2 = q2; }
        return;
    }
    a0 = fdiv<Fast>(a0, s); a1 = fdiv<Fast>(a1, s); a2 = fdiv<Fast>(a2, s);
}
template <int Fast> __device__ __forceinline__ float fsqrt(float a) {
    // Careful tier: the strict mode's short form WITHOUT its window test.  Outside the window it is merely inaccurate, with two
    // exceptions stated here: -0 maps to +0 (the reference keeps -0; no decision downstream reads the sign of a zero root),
    // and a DENORMAL argument gives NaN (rsq = inf, inf - inf) — in the intersectors a sphere whose discriminant is a denormal then
    // fails every comparison and is a miss where the reference reports a grazing hit.  A discriminant below 2^-126 at scene scale
    // (radii 0.2 - 1e5, |b| >= 1e-4) does not occur: 254 566 fuzzed scenes, 0 non-finite pixels.
    if (Fast == 2) { const float r = sqrt_short(a); return a == 0.0f ? 0.0f : r; }
    if (Fast) return __builtin_amdgcn_sqrtf(a);
    if (__builtin_expect(wave_all(in_short_window(a)), 1)) return sqrt_short(a);
    return ieee_sqrt(a);
}
template <int Fast> __device__ __forceinline__ float inversesqrt(float a) {
    if (Fast == 2) return rsqrt_short(a);
    if (Fast) return __builtin_amdgcn_rsqf(a);
    if (__builtin_expect(wave_all(in_short_window(a)), 1)) return rsqrt_short(a);
    return ieee_div(1.0f, ieee_sqrt(a));
}

// ---- strict sin / cos ------------------------------------------------------------------------------
// The quadrant count k = (int)q below IS, by definition, what the conversion instruction (v_cvt_i32_f32) computes: truncation in range,
// saturation to INT32_MAX / INT32_MIN for |q| >= 2^31 (|x| >= 2^31 * pi/2 ~ 3.37e9, +-inf), 0 for NaN; and k + 1 in mc_cos / mc_sincos
// is taken modulo 2^32.  The oracle writes the same definition out (oracle/oracle_core.h quadrant_i32) and
// tests/test_gpu_math_edges.py compares the two on every stratum of fp32.  Out there the result is DEFINED, not accurate: accuracy is
// claimed only for the ranges of DESIGN.md section 4 (nothing rendered leaves [0, 2 pi]).
__device__ __forceinline__ void sincos_reduce(float x, float& r, int& k) {
    const float TWO_OVER_PI = 0.636619772367581343f;
    const float PIO2_HI = 1.5703125f;
    const float PIO2_MID = 4.837512969970703125e-4f;
    const float PIO2_LO = 7.54978995489188216e-8f;
    float q = __builtin_rintf(x * TWO_OVER_PI);   // v_rndne_f32 (round to nearest even)
    r = __builtin_fmaf(q, -PIO2_HI, x);
    r = __builtin_fmaf(q, -PIO2_MID, r);
    r = __builtin_fmaf(q, -PIO2_LO, r);
    k = (int)q;
}
__device__ __forceinline__ float sin_kernel(float r) {
    float z = r * r;
    float p = __builtin_fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f);
    p = __builtin_fmaf(p, z, -1.6666654611e-1f);
    return __builtin_fmaf(p * z, r, r);
}
__device__ __forceinline__ float cos_kernel(float r) {
    float z = r * r;
    float p = __builtin_fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f);
    p = __builtin_fmaf(p, z, 4.166664568298827e-2f);
    float t = __builtin_fmaf(-0.5f, z, 1.0f);
    return __builtin_fmaf(p * z, z, t);
}
__device__ __forceinline__ float mc_sin(float x) {
    float r; int k; sincos_reduce(x, r, k);
    float s = (k & 1) ? cos_kernel(r) : sin_kernel(r);
    return (k & 2) ? -s : s;
}
__device__ __forceinline__ float mc_cos(float x) {
    float r; int k; sincos_reduce(x, r, k);
    float c = (k & 1) ? sin_kernel(r) : cos_kernel(r);
    return ((k + 1) & 2) ? -c : c;
}
// both at once (shares the reduction and both kernels; bit-identical to mc_sin/mc_cos)
__device__ __forceinline__ void mc_sincos(float x, float& s, float& c) {
    float r; int k; sincos_reduce(x, r, k);
    float sk = sin_kernel(r), ck = cos_kernel(r);
    float sv = (k & 1) ? ck : sk;
    float cv = (k & 1) ? sk : ck;
    // conditional negation = flipping the sign bit (also of a zero or a NaN, as the unary minus does): bit 1 of k, moved to
    // bit 31, xor-ed in — three 2-cycle integer operations instead of a compare and a select of the 4-cycle class
    s = as_float(as_uint(sv) ^ (((uint32_t)k << 30) & 0x80000000u));
    c = as_float(as_uint(cv) ^ (((uint32_t)(k + 1) << 30) & 0x80000000u));
}

// sin/cos of angle = two_pi_f32 * u where `angle` is the already-rounded fp32 product the shader
// computes (pathTracer.comp:412,426) and `u` the random number it came from.
template <int Fast> __device__ __forceinline__ void sincos_angle(float angle, float u, float& s, float& c) {
    if (Fast) {
        // v_sin_f32 / v_cos_f32 take revolutions: sin(2*pi*u).  u in [0,1].
        s = __builtin_amdgcn_sinf(u);
        c = __builtin_amdgcn_cosf(u);
    } else {
        mc_sincos(angle, s, c);
    }
}

// ---- the fast tier's transcendentals as prioritised groups (the sample-pool kernel's bounce) ---------------------------
// gfx950 prices a transcendental that stands alone among other instructions at 11 - 13 issue cycles and one issued directly behind
// another at 8.3 - 9; with seven waves of EQUAL priority interleaving on a SIMD none ever is behind another, wherever the compiler
// puts it, but a wave that raises its priority for the length of a group gets the group issued back to back
// (profiles/valu_microbench_prio.txt: 10.0 - 13.1 cycles each as they stand, 8.3 - 9.8 between s_setprio 3 and s_setprio 0).
// Each helper is ONE block: the independent transcendentals of one place in the bounce, the same opcodes on the same operands as
// inversesqrt<1>, fsqrt<1> and sincos_angle<1> emit (v_rsq_f32, v_sqrt_f32, v_sin_f32 / v_cos_f32 on the random number in
// revolutions) — every result keeps its bits.  The closing s_nop is the wait state a transcendental's result needs before an
// ordinary instruction reads it: the compiler's hazard recogniser does not look inside a block.  Outputs that are not computed in
// place are early-clobber: no result may land in the register of an operand another member of the group still reads.
#ifdef MC_PT_TRANS_UNGROUPED   // diagnostic build only (tests/test_gpu_pool_trans_groups.py): the instruction order before the groups
constexpr bool kTransGroups = false;
#else
constexpr bool kTransGroups = true;
#endif
// the light sample (:409, :412): 1 / |xc| and the sine and cosine of 2 pi u
__device__ __forceinline__ void light_trans_group(float xcc, float u, float& inv_len, float& s, float& c) {
    inv_len = xcc;
    asm volatile("s_setprio 3\n\t"
                 "v_rsq_f32_e32 %0, %0\n\t"
                 "v_sin_f32_e32 %1, %3\n\t"
                 "v_cos_f32_e32 %2, %3\n\t"
                 "s_setprio 0\n\t"
                 "s_nop 0"
                 : "+v"(inv_len), "=&v"(s), "=&v"(c) : "v"(u));
}
// the cosine-weighted bounce (:426, :428): sqrt(u2), the sine and cosine of 2 pi u1, sqrt(1 - u2)
__device__ __forceinline__ void bounce_trans_group(float u1, float u2, float& r2s, float& s1, float& c1, float& C) {
    C = 1.0f - u2;
    asm volatile("s_setprio 3\n\t"
                 "v_sqrt_f32_e32 %0, %5\n\t"
                 "v_sin_f32_e32 %1, %4\n\t"
                 "v_cos_f32_e32 %2, %4\n\t"
                 "v_sqrt_f32_e32 %3, %3\n\t"
                 "s_setprio 0\n\t"
                 "s_nop 0"
                 : "=&v"(r2s), "=&v"(s1), "=&v"(c1), "+v"(C) : "v"(u1), "v"(u2));
}

// ---- strict log2 / exp2 / pow ------------------------------------------------------------------------
__device__ __forceinline__ float mc_log2(float x) {
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
__device__ __forceinline__ float mc_exp2(float y) {
    if (!(y >= -125.0f)) return 0.0f;
    if (y > 127.0f) return __builtin_inff();
    float n = __builtin_rintf(y);
    float f = y - n;
    float p = __builtin_fmaf(1.535336188319500e-4f, f, 1.339887440266574e-3f);
    p = __builtin_fmaf(p, f, 9.618437357674640e-3f);
    p = __builtin_fmaf(p, f, 5.550357105498874e-2f);
    p = __builtin_fmaf(p, f, 2.402264791363012e-1f);
    p = __builtin_fmaf(p, f, 6.931472028550421e-1f);
    p = __builtin_fmaf(p, f, 1.0f);
    int e = (int)n + 127;
    return p * as_float((uint32_t)e << 23);
}
template <int Fast> __device__ __forceinline__ float fpow(float x, float y) {
    if (Fast) return __builtin_amdgcn_exp2f(y * __builtin_amdgcn_logf(x));   // v_exp_f32(y * v_log_f32(x))
    return mc_exp2(y * mc_log2(x));
}

// GLSL max/min (NaN behaviour differs from v_max_f32): max(x,y) = x<y ? y : x ; min(x,y) = y<x ? y : x
__device__ __forceinline__ float gmax(float x, float y) { return (x < y) ? y : x; }
__device__ __forceinline__ float gmin(float x, float y) { return (y < x) ? y : x; }

}  // namespace dm
}  // namespace mc
