// The BLA tables of MC_PRECISION_PERTURB_BLA and MC_PRECISION_PERTURB_BLA_DEEP: the one text of an entry's arithmetic (include/mc_compute.h
// states the rules; tests/mandel_bla_ref.py and tests/mandel_bla_deep_ref.py restate them).
//
// One body for the host and the device.  The host builders (mc_mandelbrot_orbit_bla / _bla_deep, mandel_orbit.cpp: a translation unit
// without HIP) and the device builders (mandel_bla_table.hip) run these same functions: the level-0 entry of a step and the merge of two
// adjacent entries of the level below, in plain double and in floatexp (norm / add / less and the +-2^20 exponent bound).
// Everything here is IEEE double in the order written: both translation units are built with -ffp-contract=off.  On the device ldexp is
// v_ldexp_f64 and the exponent v_frexp_exp_i32_f64, exact with subnormals kept, as in the deep kernels; no value that reaches a frexp here
// is an infinity or a NaN (floatexp mantissas are normalised, and a quotient's divisor is at least 0.5).
#pragma once
#include <cmath>
#include <cstdint>

#include "mandel_orbit.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MC_BLA_FN __host__ __device__ inline
#else
#define MC_BLA_FN inline
#endif

namespace mc {
namespace blatab {

// Both tables over an orbit of length L: level 0 holds steps 1 .. L-2, level k (L-2) >> k entries, while that is at least one.
struct Shape {
    uint64_t n0, total;
    uint32_t levels;
};
inline Shape shape(uint32_t length) {
    Shape sh{length >= 3 ? (uint64_t)length - 2 : 0, 0, 0};
    for (; (sh.n0 >> sh.levels) >= 1; sh.levels++) sh.total += sh.n0 >> sh.levels;
    return sh;
}

MC_BLA_FN double abs_(double v) { return __builtin_fabs(v); }
MC_BLA_FN double max_(double a, double b) { return __builtin_fmax(a, b); }
MC_BLA_FN double min_(double a, double b) { return __builtin_fmin(a, b); }
MC_BLA_FN bool finite_(double v) { return __builtin_isfinite(v); }
// ldexp(x, k) and the k of frexp (x = f * 2^k, f in [0.5, 1)) for a finite nonzero x
MC_BLA_FN double ldexp_(double x, int k) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_ldexp(x, k);
#else
    return std::ldexp(x, k);
#endif
}
MC_BLA_FN int frexp_exp_(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_frexp_exp(x);
#else
    int k = 0;
    (void)std::frexp(x, &k);
    return k;
#endif
}

// ---- MC_PRECISION_PERTURB_BLA: an entry is five doubles (A.x, A.y, B.x, B.y, R) ----

constexpr int kPlainDoubles = 5;

// the scale's bound on N1(dc)
MC_BLA_FN double plain_cm(double scale_x, double scale_y) { return 0.5 * (abs_(scale_x) + abs_(scale_y)); }

// level 0, the step Z_j -> Z_(j+1)
MC_BLA_FN void plain_level0(double zx, double zy, double* e) {
    const double eps = 0x1p-53;
    e[0] = zx + zx;
    e[1] = zy + zy;
    e[2] = 1.0;
    e[3] = 0.0;
    e[4] = eps * max_(abs_(e[0]), abs_(e[1]));
}

// level k >= 1: x = (k-1, m) then y = (k-1, m + 2^(k-1))
MC_BLA_FN void plain_merge(const double* x, const double* y, double cm, double* e) {
    e[0] = (y[0] * x[0]) - (y[1] * x[1]);
    e[1] = (y[0] * x[1]) + (y[1] * x[0]);
    e[2] = ((y[0] * x[2]) - (y[1] * x[3])) + y[2];
    e[3] = ((y[0] * x[3]) + (y[1] * x[2])) + y[3];
    const double na = abs_(x[0]) + abs_(x[1]);
    const double nb = abs_(x[2]) + abs_(x[3]);
    const double q_ = (y[4] - (nb * cm)) / na;
    const bool ok = finite_(e[0]) && finite_(e[1]) && finite_(e[2]) && finite_(e[3]) && finite_(q_) && na > 0.0 && q_ > 0.0;
    e[4] = ok ? min_(x[4], q_) : 0.0;
}

// ---- MC_PRECISION_PERTURB_BLA_DEEP: floatexp values (x, y) * 2^e, normalised (max(|x|, |y|) in [0.5, 1), or x = y = 0 with e = 0).
//      Exponents are formed in 64 bits here; the table's bound keeps every stored one within +-2^20. ----

struct Fx {
    double x, y;
    int64_t e;
};
MC_BLA_FN Fx fx_norm(double x, double y, int64_t e) {
    const double a = max_(abs_(x), abs_(y));
    if (a == 0.0) return {0.0, 0.0, 0};
    const int k = frexp_exp_(a);
    return {ldexp_(x, -k), ldexp_(y, -k), e + k};
}
// p + q for mantissas in any range: a zero operand yields the other, normalised; otherwise both are aligned with ldexp at the larger of
// their frexp exponents, added, and the sum normalised.
MC_BLA_FN Fx fx_add(const Fx& p, const Fx& q) {
    if (p.x == 0.0 && p.y == 0.0) return fx_norm(q.x, q.y, q.e);
    if (q.x == 0.0 && q.y == 0.0) return fx_norm(p.x, p.y, p.e);
    const int kp = frexp_exp_(max_(abs_(p.x), abs_(p.y)));
    const int kq = frexp_exp_(max_(abs_(q.x), abs_(q.y)));
    const int64_t e = p.e + kp > q.e + kq ? p.e + kp : q.e + kq;
    return fx_norm(ldexp_(p.x, (int)(p.e - e)) + ldexp_(q.x, (int)(q.e - e)),
                   ldexp_(p.y, (int)(p.e - e)) + ldexp_(q.y, (int)(q.e - e)), e);
}
// a < b for normalised nonnegative reals (zero below every positive value)
MC_BLA_FN bool fx_less(const Fx& a, const Fx& b) {
    if (b.x == 0.0) return false;
    if (a.x == 0.0) return true;
    return a.e < b.e || (a.e == b.e && a.x < b.x);
}
constexpr int64_t kFxBound = int64_t(1) << 20;   // an entry with an exponent beyond +-2^20 is stored as zero (R = 0)

MC_BLA_FN void deep_put(BlaDeepRec& r, const Fx& A, const Fx& B, const Fx& R) {
    const bool out = A.e < -kFxBound || A.e > kFxBound || B.e < -kFxBound || B.e > kFxBound || R.e < -kFxBound || R.e > kFxBound;
    const Fx z{0.0, 0.0, 0};
    const Fx& a = out ? z : A;
    const Fx& b = out ? z : B;
    const Fx& q = out ? z : R;
    r.ax = a.x; r.ay = a.y; r.bx = b.x; r.by = b.y; r.r = q.x;
    r.ea = (int32_t)a.e; r.eb = (int32_t)b.e; r.er = (int32_t)q.e;
    r.pad[0] = r.pad[1] = r.pad[2] = 0;
}
MC_BLA_FN void deep_get(const BlaDeepRec& r, Fx& A, Fx& B, Fx& R) {
    A = {r.ax, r.ay, r.ea}; B = {r.bx, r.by, r.eb}; R = {r.r, 0.0, r.er};
}

// cm = norm(0.5 * (|mx| + |my|), 0, E): E = 0 and (mx, my) = the scale for an orbit that is not deep
MC_BLA_FN Fx deep_cm(double scale_x, double scale_y, bool deep, int32_t scale_exp2) {
    return fx_norm(0.5 * (abs_(scale_x) + abs_(scale_y)), 0.0, deep ? scale_exp2 : 0);
}

MC_BLA_FN void deep_level0(double zx, double zy, BlaDeepRec& r) {
    const Fx A = fx_norm(zx + zx, zy + zy, 0);
    const Fx R = A.x == 0.0 && A.y == 0.0 ? Fx{0.0, 0.0, 0} : Fx{max_(abs_(A.x), abs_(A.y)), 0.0, A.e - 53};
    deep_put(r, A, Fx{0.5, 0.0, 1}, R);
}

MC_BLA_FN void deep_merge(const BlaDeepRec& x, const BlaDeepRec& y, const Fx& cm, BlaDeepRec& r) {
    Fx xa, xb, xr, ya, yb, yr;
    deep_get(x, xa, xb, xr);   // (k-1, m), m = 1 + q 2^k
    deep_get(y, ya, yb, yr);   // (k-1, m + 2^(k-1))
    const Fx A = fx_norm((ya.x * xa.x) - (ya.y * xa.y), (ya.x * xa.y) + (ya.y * xa.x), ya.e + xa.e);
    const Fx B = fx_add(Fx{(ya.x * xb.x) - (ya.y * xb.y), (ya.x * xb.y) + (ya.y * xb.x), ya.e + xb.e}, yb);
    const double na = abs_(xa.x) + abs_(xa.y);
    const double nb = abs_(xb.x) + abs_(xb.y);
    const Fx diff = fx_add(yr, Fx{-(nb * cm.x), 0.0, xb.e + cm.e});   // Ry - N1(Bx) cm
    Fx R{0.0, 0.0, 0};
    if (na > 0.0 && diff.x > 0.0) {
        const Fx qv = fx_norm(diff.x / na, 0.0, diff.e - xa.e);
        R = fx_less(qv, xr) ? qv : xr;                                 // min(Rx, q); Rx = 0 gives 0
    }
    deep_put(r, A, B, R);
}

}  // namespace blatab
}  // namespace mc
