// The reference orbit of MC_PRECISION_PERTURB on the host (include/mc_compute.h states the contract): Z_0 .. Z_L at the
// view's centre in binary fixed point of `bits` fractional bits (uint64_t limbs, unsigned __int128 products), from decimal text, rounded
// to a double table; the orbit object, and the two BLA tables built from that table.  No HIP: the library links this file as it is, and
// tools/orbit_host_check.cpp runs it alone under the sanitizers.  IEEE double in source order (-ffp-contract=off, like every other TU).
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "mandel_orbit.h"

// ---- multi-limb fixed point -----------------------------------------------------------------------------------------------------
namespace {

// Sign and magnitude; m[0 .. k-1] the fractional limbs (least significant first), m[k] the integer limb.  k <= 130: 8320 >= 8288
// fractional bits, the most a scale of 2^-8192 asks for (mc_mandelbrot_orbit_create_deep).  Every loop runs over the k + 1 limbs in
// use, never the whole array: a shallow orbit (k = 2 or 3) does the same work as with a 17-limb array.
constexpr int kMaxFrac = 130;
struct Fix {
    uint64_t m[kMaxFrac + 1];
    bool neg;
};

struct FixOps {
    int k;   // fractional limbs; every Fix holds k + 1 limbs
    int n() const { return k + 1; }
    void zero(Fix& a) const { std::memset(a.m, 0, sizeof a.m); a.neg = false; }
    bool is_zero(const Fix& a) const {
        for (int i = 0; i < n(); i++) if (a.m[i]) return false;
        return true;
    }
    int cmp_mag(const Fix& a, const Fix& b) const {
        for (int i = n() - 1; i >= 0; i--) if (a.m[i] != b.m[i]) return a.m[i] < b.m[i] ? -1 : 1;
        return 0;
    }
    static void add_mag(const uint64_t* a, const uint64_t* b, uint64_t* r, int n) {
        unsigned __int128 c = 0;
        for (int i = 0; i < n; i++) { c += (unsigned __int128)a[i] + b[i]; r[i] = (uint64_t)c; c >>= 64; }
    }
    static void sub_mag(const uint64_t* a, const uint64_t* b, uint64_t* r, int n) {   // a >= b
        uint64_t borrow = 0;
        for (int i = 0; i < n; i++) {
            uint64_t t = a[i] - b[i];
            uint64_t b1 = a[i] < b[i];
            r[i] = t - borrow;
            borrow = b1 | (t < borrow);
        }
    }
    // r = a + b (signed).  r may alias a or b.
    void add(const Fix& a, const Fix& b, Fix& r) const {
        if (a.neg == b.neg) { add_mag(a.m, b.m, r.m, n()); r.neg = a.neg; }
        else if (cmp_mag(a, b) >= 0) { bool s = a.neg; sub_mag(a.m, b.m, r.m, n()); r.neg = s; }
        else { bool s = b.neg; sub_mag(b.m, a.m, r.m, n()); r.neg = s; }
        if (is_zero(r)) r.neg = false;
    }
    // r = a - b: a + b with b's sign flipped (no copy of b).  r may alias a or b.
    void sub(const Fix& a, const Fix& b, Fix& r) const {
        const bool bneg = !b.neg && !is_zero(b);
        if (a.neg == bneg) { add_mag(a.m, b.m, r.m, n()); r.neg = a.neg; }
        else if (cmp_mag(a, b) >= 0) { bool s = a.neg; sub_mag(a.m, b.m, r.m, n()); r.neg = s; }
        else { sub_mag(b.m, a.m, r.m, n()); r.neg = bneg; }
        if (is_zero(r)) r.neg = false;
    }
    // r = a * b rounded to nearest (ties away from zero) at the last fractional bit.  The integer part stays below 2^64 (|Z| <= 8).
    void mul(const Fix& a, const Fix& b, Fix& r) const {
        const int nn = n();
        uint64_t p[2 * (kMaxFrac + 1)];
        std::memset(p, 0, 2 * nn * sizeof(uint64_t));   // the 2(k + 1) limbs in use only
        for (int i = 0; i < nn; i++) {
            unsigned __int128 c = 0;
            const uint64_t ai = a.m[i];
            for (int j = 0; j < nn; j++) {
                c += (unsigned __int128)ai * b.m[j] + p[i + j];
                p[i + j] = (uint64_t)c;
                c >>= 64;
            }
            p[i + nn] = (uint64_t)c;
        }
        unsigned __int128 c = p[k - 1] >> 63;   // the first dropped bit
        for (int i = 0; i < nn; i++) { c += p[k + i]; r.m[i] = (uint64_t)c; c >>= 64; }
        r.neg = (a.neg != b.neg) && !is_zero(r);
    }
    void twice(Fix& a) const {   // exact
        for (int i = n() - 1; i > 0; i--) a.m[i] = (a.m[i] << 1) | (a.m[i - 1] >> 63);
        a.m[0] <<= 1;
    }
    // |a| > 2 (a >= 0 here: a sum of squares)
    bool above_two(const Fix& a) const {
        if (a.m[k] != 2) return a.m[k] > 2;
        for (int i = 0; i < k; i++) if (a.m[i]) return true;
        return false;
    }
    // bits [lo, lo + cnt) of the magnitude, cnt <= 64
    uint64_t bits_at(const Fix& a, int lo, int cnt) const {
        uint64_t v = 0;
        for (int b = 0; b < cnt; b++) {
            const int pos = lo + b;
            if (pos >= 0 && pos < 64 * n() && ((a.m[pos >> 6] >> (pos & 63)) & 1u)) v |= 1ull << b;
        }
        return v;
    }
    bool any_below(const Fix& a, int pos) const {   // any bit of the magnitude below position pos
        for (int i = 0; i < n() && 64 * i < pos; i++) {
            const int in = pos - 64 * i;
            const uint64_t mask = in >= 64 ? ~0ull : ((1ull << in) - 1);
            if (a.m[i] & mask) return true;
        }
        return false;
    }
    // Nearest double, ties to even (subnormals included: the quantum below 2^-1022 is 2^-1074).
    double to_double(const Fix& a) const {
        int top = -1;
        for (int i = n() - 1; i >= 0 && top < 0; i--)
            if (a.m[i]) top = 64 * i + 63 - __builtin_clzll(a.m[i]);
        if (top < 0) return 0.0;
        const int F = 64 * k;
        int shift = top - 52;
        if (shift < F - 1074) shift = F - 1074;
        uint64_t mant;
        if (shift <= 0) {
            mant = bits_at(a, 0, top + 1);
            shift = 0;
        } else {
            mant = bits_at(a, shift, top - shift + 1);
            const bool half = bits_at(a, shift - 1, 1) != 0;
            const bool sticky = any_below(a, shift - 1);
            if (half && (sticky || (mant & 1u))) mant++;
        }
        const double v = std::ldexp((double)mant, shift - F);
        return a.neg ? -v : v;
    }
};

// [+-]? (digits [. digits?] | . digits) ([eE] [+-]? digits)?, |value| <= 4, rounded to odd at the last of the k * 64 fractional bits.
bool parse_decimal(const char* s, const FixOps& ops, Fix& out) {
    if (!s) return false;
    const size_t len = strnlen(s, 4097);
    if (len == 0 || len > 4096) return false;
    size_t i = 0;
    bool neg = false;
    if (s[i] == '+' || s[i] == '-') neg = s[i++] == '-';
    std::vector<int> digits;
    int64_t int_digits = 0;
    while (s[i] >= '0' && s[i] <= '9') { digits.push_back(s[i++] - '0'); int_digits++; }
    size_t frac_digits = 0;
    if (s[i] == '.') {
        i++;
        while (s[i] >= '0' && s[i] <= '9') { digits.push_back(s[i++] - '0'); frac_digits++; }
    }
    if (int_digits == 0 && frac_digits == 0) return false;
    int64_t e = 0;
    if (s[i] == 'e' || s[i] == 'E') {
        i++;
        bool eneg = false;
        if (s[i] == '+' || s[i] == '-') eneg = s[i++] == '-';
        if (!(s[i] >= '0' && s[i] <= '9')) return false;
        while (s[i] >= '0' && s[i] <= '9') {
            if (e < 100000000) e = e * 10 + (s[i] - '0');   // saturates: far beyond any digit count of 4096 characters
            i++;
        }
        if (eneg) e = -e;
    }
    if (i != len) return false;
    // value = 0.d1 d2 ... x 10^point after dropping leading zeros
    int64_t point = int_digits + e;
    size_t first = 0;
    while (first < digits.size() && digits[first] == 0) { first++; point--; }
    ops.zero(out);
    if (first == digits.size()) return true;   // zero
    size_t last = digits.size();
    while (digits[last - 1] == 0) last--;
    if (point > 1) return false;               // >= 10
    uint32_t int_part = 0;
    if (point == 1) int_part = (uint32_t)digits[first++];
    // Horner from the last digit: acc = floor((acc + d * 2^F) / 10) per digit gives floor(fraction * 2^F) exactly; a nonzero remainder
    // anywhere means the fraction had more bits (the sticky bit)
    const int k = ops.k, n = ops.n();
    bool sticky = false;
    auto div10 = [&]() {
        unsigned __int128 rem = 0;
        for (int j = n - 1; j >= 0; j--) {
            unsigned __int128 cur = (rem << 64) | out.m[j];
            out.m[j] = (uint64_t)(cur / 10u);
            rem = cur % 10u;
        }
        if (rem) sticky = true;
    };
    for (size_t j = last; j > first; j--) {
        out.m[k] += (uint64_t)digits[j - 1];
        div10();
    }
    for (int64_t z = 0; z < -point && !ops.is_zero(out); z++) div10();   // the zeros between the point and the first digit (once
                                                                          // the floor is 0 more of them change nothing but sticky)
    out.m[k] += int_part;
    if (sticky) out.m[0] |= 1u;   // round to odd
    if (out.m[k] > 4) return false;
    if (out.m[k] == 4)
        for (int j = 0; j < k; j++) if (out.m[j]) return false;
    out.neg = neg && !ops.is_zero(out);
    return true;
}

// `fn`: `why` as the error detail; the status to return.
int refuse(const char* fn, const std::string& why, int status = MC_ERR_INVALID_ARGUMENT) {
    mc::set_error_detail(std::string(fn) + ": " + why);
    return status;
}

// The iteration loop on the host, with an mc::OrbitLoop's contract.
int host_loop(const FixOps& ops, const Fix& cx, const Fix& cy, uint32_t max_iter, bool deep, std::vector<double>& z, uint32_t* length,
              uint32_t* tiny_j) {
    z.reserve(2 * ((size_t)max_iter + 1) < 2 * 65536 ? 2 * ((size_t)max_iter + 1) : 2 * 65536);
    const double tiny = std::ldexp(1.0, -960);
    Fix zx, zy, sx, sy, t;
    ops.zero(zx); ops.zero(zy); ops.zero(sx); ops.zero(sy);
    uint32_t L = max_iter;
    for (uint32_t j = 0; j < max_iter; j++) {
        ops.mul(zx, zy, t);                           // Z_{j+1} = Z_j^2 + c_ref
        ops.twice(t);
        ops.add(t, cy, zy);
        ops.sub(sx, sy, t);
        ops.add(t, cx, zx);
        const double dx = ops.to_double(zx), dy = ops.to_double(zy);
        if (deep && std::fabs(dx) < tiny && std::fabs(dy) < tiny && !(ops.is_zero(zx) && ops.is_zero(zy))) {
            *tiny_j = j + 1;
            return mc::kOrbitTinyEntry;
        }
        z.push_back(dx);
        z.push_back(dy);
        ops.mul(zx, zx, sx);
        ops.mul(zy, zy, sy);
        ops.add(sx, sy, t);
        if (ops.above_two(t)) { L = j + 1; break; }
    }
    *length = L;
    return MC_OK;
}

// The orbit of every constructor.  bits and the refusal of scales below the floor are decided by the caller; deep = the tiny-entry
// refusal of include/mc_compute.h applies.  `fn` names the entry point in the error detail.  An empty loop: host_loop.
int make_orbit(const char* fn, const mc::OrbitLoop& loop, const char* centre_x, const char* centre_y, int64_t bits, bool below_floor,
               bool deep, uint32_t max_iter, mc_mandelbrot_orbit** out) {
    FixOps ops{(int)((bits + 63) / 64)};
    Fix cx, cy;
    if (ops.k > kMaxFrac) ops.k = kMaxFrac;          // (only reached below the floor, refused after the strings are checked)
    if (!parse_decimal(centre_x, ops, cx))
        return refuse(fn, "centre_x is not a decimal of at most 4096 characters with |value| <= 4");
    if (!parse_decimal(centre_y, ops, cy))
        return refuse(fn, "centre_y is not a decimal of at most 4096 characters with |value| <= 4");
    if (below_floor)
        return refuse(fn, deep ? "scale below 2^-8192 (the orbit's fixed point would need more than 130 limbs)"
                               : "scale below 2^-960 (pixel offsets would leave the normal doubles)", MC_ERR_UNSUPPORTED);
    mc_mandelbrot_orbit* o = new (std::nothrow) mc_mandelbrot_orbit();
    if (!o) return MC_ERR_OUT_OF_MEMORY;
    uint32_t tiny_j = 0;
    int rc;
    try {
        o->z.push_back(0.0); o->z.push_back(0.0);
        rc = loop ? loop(ops.k, cx.m, cy.m, cx.neg, cy.neg, max_iter, deep, o->z, &o->length, &tiny_j)
                  : host_loop(ops, cx, cy, max_iter, deep, o->z, &o->length, &tiny_j);
    } catch (const std::bad_alloc&) {
        rc = MC_ERR_OUT_OF_MEMORY;
    }
    if (rc) {
        delete o;
        if (rc != mc::kOrbitTinyEntry) return rc;
        return refuse(fn, "orbit entry Z_" + std::to_string(tiny_j) +
                              " is nonzero with both parts below 2^-960 (the centre sits on a nucleus far more closely than"
                              " the view needs; the double table cannot hold that entry)", MC_ERR_UNSUPPORTED);
    }
    o->max_iter = max_iter;
    o->bits = (uint32_t)bits;
    o->deep = deep;
    *out = o;
    return MC_OK;
}

// What every constructor checks first, in this order; *out is NULL from the second refusal on.
int check_arguments(const char* fn, const char* centre_x, const char* centre_y, double scale_x, double scale_y, uint32_t max_iter,
                    mc_mandelbrot_orbit** out) {
    if (!out || !centre_x || !centre_y) return refuse(fn, "NULL argument");
    if (max_iter == 0) return refuse(fn, "max_iter must be at least 1");
    *out = nullptr;
    if (!std::isfinite(scale_x) || !std::isfinite(scale_y) || scale_x == 0.0 || scale_y == 0.0)
        return refuse(fn, "scale_x and scale_y must be finite and nonzero");
    return MC_OK;
}

// mc_mandelbrot_orbit_create under the name `fn`, past check_arguments.
int create_plain(const char* fn, const mc::OrbitLoop& loop, const char* centre_x, const char* centre_y, double scale_x, double scale_y,
                 uint32_t max_iter, mc_mandelbrot_orbit** out) {
    const double smin = std::fmin(std::fabs(scale_x), std::fabs(scale_y));
    int e = 0;
    (void)std::frexp(smin, &e);                      // smin = f * 2^e, f in [0.5, 1): ceil(-log2 smin) = 1 - e exactly
    int64_t bits = (int64_t)1 - e + 96;
    if (bits < 64) bits = 64;
    const int rc = make_orbit(fn, loop, centre_x, centre_y, bits, smin < std::ldexp(1.0, -960), false, max_iter, out);
    if (rc) return rc;
    (*out)->scale_x = scale_x;
    (*out)->scale_y = scale_y;
    return MC_OK;
}

}  // namespace

int mc::orbit_create(const char* fn, const char* fn_plain, const OrbitLoop& loop, const char* centre_x, const char* centre_y,
                     double scale_x, double scale_y, int32_t scale_exp2, uint32_t max_iter, mc_mandelbrot_orbit** out) {
    if (int rc = check_arguments(fn, centre_x, centre_y, scale_x, scale_y, max_iter, out)) return rc;
    // min |scale| = f * 2^emin, f in [0.5, 1), from the mantissas' frexp exponents plus scale_exp2 (64-bit: no overflow)
    int ex = 0, ey = 0;
    const double fx = std::frexp(std::fabs(scale_x), &ex), fy = std::frexp(std::fabs(scale_y), &ey);
    const int64_t emin = (ex < ey || (ex == ey && fx <= fy) ? (int64_t)ex : (int64_t)ey) + scale_exp2;
    if (emin >= -959) {                              // the scale is a double of at least 2^-960: exactly mc_mandelbrot_orbit_create
        const int64_t emax = (ex > ey ? ex : ey) + (int64_t)scale_exp2;
        if (emax > 1024) return refuse(fn, "scale above the double range", MC_ERR_UNSUPPORTED);
        const double sx = std::ldexp(scale_x, scale_exp2);   // exact: both results are normal doubles
        const double sy = std::ldexp(scale_y, scale_exp2);
        if (!std::isfinite(sx) || !std::isfinite(sy)) return refuse(fn, "scale above the double range", MC_ERR_UNSUPPORTED);
        return create_plain(fn_plain, loop, centre_x, centre_y, sx, sy, max_iter, out);
    }
    const int rc = make_orbit(fn, loop, centre_x, centre_y, 1 - emin + 96, emin < -8191, true, max_iter, out);   // bits > 1056
    if (rc) return rc;
    (*out)->scale_x = scale_x;
    (*out)->scale_y = scale_y;
    (*out)->scale_exp2 = scale_exp2;
    return MC_OK;
}

extern "C" {

int mc_mandelbrot_orbit_create(const char* centre_x, const char* centre_y, double scale_x, double scale_y, uint32_t max_iter,
                               mc_mandelbrot_orbit** out) {
    const char* fn = "mc_mandelbrot_orbit_create";
    if (int rc = check_arguments(fn, centre_x, centre_y, scale_x, scale_y, max_iter, out)) return rc;
    return create_plain(fn, {}, centre_x, centre_y, scale_x, scale_y, max_iter, out);
}

int mc_mandelbrot_orbit_create_deep(const char* centre_x, const char* centre_y, double scale_x, double scale_y, int32_t scale_exp2,
                                    uint32_t max_iter, mc_mandelbrot_orbit** out) {
    return mc::orbit_create("mc_mandelbrot_orbit_create_deep", "mc_mandelbrot_orbit_create", {}, centre_x, centre_y, scale_x, scale_y,
                            scale_exp2, max_iter, out);
}

int mc_mandelbrot_orbit_destroy(mc_mandelbrot_orbit* o) {
    delete o;
    return MC_OK;
}

int mc_mandelbrot_orbit_info(const mc_mandelbrot_orbit* o, uint32_t* length, uint32_t* max_iter, uint32_t* bits) {
    if (!o) return MC_ERR_INVALID_ARGUMENT;
    if (length) *length = o->length;
    if (max_iter) *max_iter = o->max_iter;
    if (bits) *bits = o->bits;
    return MC_OK;
}

int mc_mandelbrot_orbit_copy(const mc_mandelbrot_orbit* o, double* out_z) {
    if (!o || !out_z) return MC_ERR_INVALID_ARGUMENT;
    std::memcpy(out_z, o->z.data(), o->z.size() * sizeof(double));
    return MC_OK;
}

}  // extern "C"

namespace {

// Both BLA tables over an orbit of length L: level 0 holds steps 1 .. L-2, level k (L-2) >> k entries, while that is at least one.
struct BlaShape {
    uint64_t n0, total;
    uint32_t levels;
};
BlaShape bla_shape(uint32_t length) {
    BlaShape sh{length >= 3 ? (uint64_t)length - 2 : 0, 0, 0};
    for (; (sh.n0 >> sh.levels) >= 1; sh.levels++) sh.total += sh.n0 >> sh.levels;
    return sh;
}

}  // namespace

extern "C" {

// The BLA table of include/mc_compute.h (MC_PRECISION_PERTURB_BLA), operation by operation.
int mc_mandelbrot_orbit_bla(mc_mandelbrot_orbit* o, uint32_t* levels, uint64_t* entries) {
    if (!o) return refuse("mc_mandelbrot_orbit_bla", "NULL orbit");
    if (o->deep)
        return refuse("mc_mandelbrot_orbit_bla", "a deep orbit (min |scale| < 2^-960) renders by the rescaled loop, which has no BLA",
                      MC_ERR_UNSUPPORTED);
    if (!o->has_bla) {
        const BlaShape sh = bla_shape(o->length);
        const uint64_t n0 = sh.n0, total = sh.total;
        const uint32_t nlev = sh.levels;
        std::vector<double> t;
        try {
            t.resize(5 * total);
        } catch (const std::bad_alloc&) {
            return refuse("mc_mandelbrot_orbit_bla", "the table does not fit in host memory", MC_ERR_OUT_OF_MEMORY);
        }
        const double eps = std::ldexp(1.0, -53);
        const double cm = 0.5 * (std::fabs(o->scale_x) + std::fabs(o->scale_y));
        for (uint64_t j = 1; j <= n0; j++) {
            double* e = &t[5 * (j - 1)];
            const double zx = o->z[2 * j], zy = o->z[2 * j + 1];
            e[0] = zx + zx;
            e[1] = zy + zy;
            e[2] = 1.0;
            e[3] = 0.0;
            e[4] = eps * std::fmax(std::fabs(e[0]), std::fabs(e[1]));
        }
        uint64_t prev = 0, off = n0;   // level k-1 starts at prev, level k at off
        for (uint32_t k = 1; k < nlev; k++) {
            const uint64_t cnt = n0 >> k;
            for (uint64_t q = 0; q < cnt; q++) {
                const double* x = &t[5 * (prev + 2 * q)];       // (k-1, m), m = 1 + q 2^k
                const double* y = &t[5 * (prev + 2 * q + 1)];   // (k-1, m + 2^(k-1))
                double* e = &t[5 * (off + q)];
                e[0] = (y[0] * x[0]) - (y[1] * x[1]);
                e[1] = (y[0] * x[1]) + (y[1] * x[0]);
                e[2] = ((y[0] * x[2]) - (y[1] * x[3])) + y[2];
                e[3] = ((y[0] * x[3]) + (y[1] * x[2])) + y[3];
                const double na = std::fabs(x[0]) + std::fabs(x[1]);
                const double nb = std::fabs(x[2]) + std::fabs(x[3]);
                const double q_ = (y[4] - (nb * cm)) / na;
                const bool ok = std::isfinite(e[0]) && std::isfinite(e[1]) && std::isfinite(e[2]) && std::isfinite(e[3]) &&
                                std::isfinite(q_) && na > 0.0 && q_ > 0.0;
                e[4] = ok ? std::fmin(x[4], q_) : 0.0;
            }
            prev = off;
            off += cnt;
        }
        o->bla.swap(t);
        o->bla_levels = nlev;
        o->bla_entries = total;
        o->has_bla = true;
    }
    if (levels) *levels = o->bla_levels;
    if (entries) *entries = o->bla_entries;
    return MC_OK;
}

namespace {

// Floatexp values of MC_PRECISION_PERTURB_BLA_DEEP (include/mc_compute.h): (x, y) * 2^e, normalised (max(|x|, |y|) in [0.5, 1), or
// x = y = 0 with e = 0).  Exponents are formed in 64 bits here; the table's bound keeps every stored one within +-2^20.
struct Fx {
    double x, y;
    int64_t e;
};
Fx fx_norm(double x, double y, int64_t e) {
    const double a = std::fmax(std::fabs(x), std::fabs(y));
    if (a == 0.0) return {0.0, 0.0, 0};
    int k = 0;
    (void)std::frexp(a, &k);
    return {std::ldexp(x, -k), std::ldexp(y, -k), e + k};
}
// p + q for mantissas in any range: a zero operand yields the other, normalised; otherwise both are aligned with ldexp at the larger of
// their frexp exponents, added, and the sum normalised.
Fx fx_add(const Fx& p, const Fx& q) {
    if (p.x == 0.0 && p.y == 0.0) return fx_norm(q.x, q.y, q.e);
    if (q.x == 0.0 && q.y == 0.0) return fx_norm(p.x, p.y, p.e);
    int kp = 0, kq = 0;
    (void)std::frexp(std::fmax(std::fabs(p.x), std::fabs(p.y)), &kp);
    (void)std::frexp(std::fmax(std::fabs(q.x), std::fabs(q.y)), &kq);
    const int64_t e = p.e + kp > q.e + kq ? p.e + kp : q.e + kq;
    return fx_norm(std::ldexp(p.x, (int)(p.e - e)) + std::ldexp(q.x, (int)(q.e - e)),
                   std::ldexp(p.y, (int)(p.e - e)) + std::ldexp(q.y, (int)(q.e - e)), e);
}
// a < b for normalised nonnegative reals (zero below every positive value)
bool fx_less(const Fx& a, const Fx& b) {
    if (b.x == 0.0) return false;
    if (a.x == 0.0) return true;
    return a.e < b.e || (a.e == b.e && a.x < b.x);
}
constexpr int64_t kFxBound = int64_t(1) << 20;   // an entry with an exponent beyond +-2^20 is stored as zero (R = 0)

}  // namespace

// The floatexp BLA table of include/mc_compute.h (MC_PRECISION_PERTURB_BLA_DEEP), operation by operation.
int mc_mandelbrot_orbit_bla_deep(mc_mandelbrot_orbit* o, uint32_t* levels, uint64_t* entries) {
    if (!o) return refuse("mc_mandelbrot_orbit_bla_deep", "NULL orbit");
    if (!o->has_bla_deep) {
        const BlaShape sh = bla_shape(o->length);
        const uint64_t n0 = sh.n0, total = sh.total;
        const uint32_t nlev = sh.levels;
        std::vector<mc::BlaDeepRec> t;
        try {
            t.resize(total);
        } catch (const std::bad_alloc&) {
            return refuse("mc_mandelbrot_orbit_bla_deep", "the table does not fit in host memory", MC_ERR_OUT_OF_MEMORY);
        }
        auto put = [](mc::BlaDeepRec& r, const Fx& A, const Fx& B, const Fx& R) {
            const bool out = A.e < -kFxBound || A.e > kFxBound || B.e < -kFxBound || B.e > kFxBound || R.e < -kFxBound || R.e > kFxBound;
            const Fx z{0.0, 0.0, 0};
            const Fx& a = out ? z : A;
            const Fx& b = out ? z : B;
            const Fx& q = out ? z : R;
            r.ax = a.x; r.ay = a.y; r.bx = b.x; r.by = b.y; r.r = q.x;
            r.ea = (int32_t)a.e; r.eb = (int32_t)b.e; r.er = (int32_t)q.e;
            r.pad[0] = r.pad[1] = r.pad[2] = 0;
        };
        auto get = [](const mc::BlaDeepRec& r, Fx& A, Fx& B, Fx& R) {
            A = {r.ax, r.ay, r.ea}; B = {r.bx, r.by, r.eb}; R = {r.r, 0.0, r.er};
        };
        const Fx cm = fx_norm(0.5 * (std::fabs(o->scale_x) + std::fabs(o->scale_y)), 0.0, o->deep ? o->scale_exp2 : 0);
        for (uint64_t j = 1; j <= n0; j++) {
            const double zx = o->z[2 * j], zy = o->z[2 * j + 1];
            const Fx A = fx_norm(zx + zx, zy + zy, 0);
            const Fx R = A.x == 0.0 && A.y == 0.0 ? Fx{0.0, 0.0, 0} : Fx{std::fmax(std::fabs(A.x), std::fabs(A.y)), 0.0, A.e - 53};
            put(t[j - 1], A, Fx{0.5, 0.0, 1}, R);
        }
        uint64_t prev = 0, off = n0;   // level k-1 starts at prev, level k at off
        for (uint32_t k = 1; k < nlev; k++) {
            const uint64_t cnt = n0 >> k;
            for (uint64_t q = 0; q < cnt; q++) {
                Fx xa, xb, xr, ya, yb, yr;
                get(t[prev + 2 * q], xa, xb, xr);       // (k-1, m), m = 1 + q 2^k
                get(t[prev + 2 * q + 1], ya, yb, yr);   // (k-1, m + 2^(k-1))
                const Fx A = fx_norm((ya.x * xa.x) - (ya.y * xa.y), (ya.x * xa.y) + (ya.y * xa.x), ya.e + xa.e);
                const Fx B = fx_add(Fx{(ya.x * xb.x) - (ya.y * xb.y), (ya.x * xb.y) + (ya.y * xb.x), ya.e + xb.e}, yb);
                const double na = std::fabs(xa.x) + std::fabs(xa.y);
                const double nb = std::fabs(xb.x) + std::fabs(xb.y);
                const Fx diff = fx_add(yr, Fx{-(nb * cm.x), 0.0, xb.e + cm.e});   // Ry - N1(Bx) cm
                Fx R{0.0, 0.0, 0};
                if (na > 0.0 && diff.x > 0.0) {
                    const Fx qv = fx_norm(diff.x / na, 0.0, diff.e - xa.e);
                    R = fx_less(qv, xr) ? qv : xr;                                 // min(Rx, q); Rx = 0 gives 0
                }
                put(t[off + q], A, B, R);
            }
            prev = off;
            off += cnt;
        }
        o->bla_deep.swap(t);
        o->bla_deep_levels = nlev;
        o->bla_deep_entries = total;
        o->has_bla_deep = true;
    }
    if (levels) *levels = o->bla_deep_levels;
    if (entries) *entries = o->bla_deep_entries;
    return MC_OK;
}

int mc_mandelbrot_orbit_bla_deep_copy(const mc_mandelbrot_orbit* o, double* mant, int32_t* exps) {
    if (!o || !mant || !exps || !o->has_bla_deep)
        return refuse("mc_mandelbrot_orbit_bla_deep_copy", "NULL argument, or no table (mc_mandelbrot_orbit_bla_deep builds it)");
    for (size_t j = 0; j < o->bla_deep.size(); j++) {
        const mc::BlaDeepRec& r = o->bla_deep[j];
        mant[5 * j] = r.ax; mant[5 * j + 1] = r.ay; mant[5 * j + 2] = r.bx; mant[5 * j + 3] = r.by; mant[5 * j + 4] = r.r;
        exps[3 * j] = r.ea; exps[3 * j + 1] = r.eb; exps[3 * j + 2] = r.er;
    }
    return MC_OK;
}

int mc_mandelbrot_orbit_bla_copy(const mc_mandelbrot_orbit* o, double* out) {
    if (!o || !out || !o->has_bla)
        return refuse("mc_mandelbrot_orbit_bla_copy", "NULL argument, or no table (mc_mandelbrot_orbit_bla builds it)");
    if (!o->bla.empty()) std::memcpy(out, o->bla.data(), o->bla.size() * sizeof(double));
    return MC_OK;
}

}  // extern "C"
