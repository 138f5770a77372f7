// The reference orbit of MC_PRECISION_PERTURB on the host (include/mc_compute.h states the contract): Z_0 .. Z_L at the
// view's centre in binary fixed point of `bits` fractional bits (uint64_t limbs, unsigned __int128 products), from decimal text, rounded
// to a double table; the orbit object, and the two BLA tables built from that table.  No HIP: the library links this file as it is, and
// tools/orbit_host_check.cpp runs it alone under the sanitizers.  IEEE double in source order (-ffp-contract=off, like every other TU).
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "mandel_bla_table.h"
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

const char* below_floor_text(bool deep) {
    return deep ? "scale below 2^-8192 (the orbit's fixed point would need more than 130 limbs)"
                : "scale below 2^-960 (pixel offsets would leave the normal doubles)";
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
    if (below_floor) return refuse(fn, below_floor_text(deep), MC_ERR_UNSUPPORTED);
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
    try {
        o->cx.assign(cx.m, cx.m + ops.n());
        o->cy.assign(cy.m, cy.m + ops.n());
    } catch (const std::bad_alloc&) {
        delete o;
        return MC_ERR_OUT_OF_MEMORY;
    }
    o->cx_neg = cx.neg;
    o->cy_neg = cy.neg;
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

// What an orbit object stores for a view's scale, and what the scale asks of the fixed point: the one text of it, for every constructor
// and for mc_mandelbrot_orbit_rescale.  deep: (x, y) are the mantissas and exp2 the exponent; otherwise (x, y) is the scale and exp2 is 0.
struct OrbitScale {
    double x, y;
    int32_t exp2;
    bool deep;
    int64_t bits;       // the header's formula
    bool below_floor;   // refused (after the centre strings are checked): below_floor_text(deep)
};

// mc_mandelbrot_orbit_create's scale: finite nonzero doubles.
OrbitScale plain_scale(double scale_x, double scale_y) {
    const double smin = std::fmin(std::fabs(scale_x), std::fabs(scale_y));
    int e = 0;
    (void)std::frexp(smin, &e);                      // smin = f * 2^e, f in [0.5, 1): ceil(-log2 smin) = 1 - e exactly
    int64_t bits = (int64_t)1 - e + 96;
    if (bits < 64) bits = 64;
    return {scale_x, scale_y, 0, false, bits, smin < std::ldexp(1.0, -960)};
}

// mc_mandelbrot_orbit_create_deep's scale (scale_x, scale_y) * 2^scale_exp2, finite nonzero mantissas: folded into plain doubles when
// min |scale| >= 2^-960 (the orbit is mc_mandelbrot_orbit_create's), kept as mantissas and exponent below.
int normalise_scale(const char* fn, double scale_x, double scale_y, int32_t scale_exp2, OrbitScale* s) {
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
        *s = plain_scale(sx, sy);
        return MC_OK;
    }
    *s = {scale_x, scale_y, scale_exp2, true, 1 - emin + 96, emin < -8191};   // bits > 1056
    return MC_OK;
}

void store_scale(mc_mandelbrot_orbit* o, const OrbitScale& s) {
    o->scale_x = s.x;
    o->scale_y = s.y;
    o->scale_exp2 = s.exp2;
    o->deep = s.deep;
}

// The orbit for a normalised scale, past check_arguments; `fn` names the entry point in the error detail.
int create_scaled(const char* fn, const mc::OrbitLoop& loop, const char* centre_x, const char* centre_y, const OrbitScale& s,
                  uint32_t max_iter, mc_mandelbrot_orbit** out) {
    const int rc = make_orbit(fn, loop, centre_x, centre_y, s.bits, s.below_floor, s.deep, max_iter, out);
    if (rc) return rc;
    store_scale(*out, s);
    return MC_OK;
}

}  // namespace

int mc::orbit_create(const char* fn, const char* fn_plain, const OrbitLoop& loop, const char* centre_x, const char* centre_y,
                     double scale_x, double scale_y, int32_t scale_exp2, uint32_t max_iter, mc_mandelbrot_orbit** out) {
    if (int rc = check_arguments(fn, centre_x, centre_y, scale_x, scale_y, max_iter, out)) return rc;
    OrbitScale s;
    if (int rc = normalise_scale(fn, scale_x, scale_y, scale_exp2, &s)) return rc;
    return create_scaled(s.deep ? fn : fn_plain, loop, centre_x, centre_y, s, max_iter, out);
}

// ---- exact counts of sampled pixels (include/mc_compute.h: "exact counts") ----------------------------------------------------------
namespace {

// v * 2^exp2 as a Fix.  1: a bit would fall below the last fractional bit; 2: it does not fit under the integer limb's top bits.
int offset_fix(const FixOps& ops, double v, int64_t exp2, Fix& out) {
    ops.zero(out);
    if (v == 0.0) return 0;
    int e = 0;
    const double f = std::frexp(std::fabs(v), &e);          // f in [0.5, 1), subnormals included
    uint64_t m = (uint64_t)std::ldexp(f, 53);               // an integer below 2^53, exactly
    int64_t s = (int64_t)e - 53 + exp2 + 64 * (int64_t)ops.k;   // |v| 2^exp2 2^F = m 2^s
    const int tz = __builtin_ctzll(m);
    m >>= tz;
    s += tz;
    if (s < 0) return 1;
    const int len = 64 - __builtin_clzll(m);
    if (s + len > 64 * (int64_t)ops.k + 8) return 2;        // 256 or more: |c| > 4 whatever c_ref is
    const int limb = (int)(s >> 6), r = (int)(s & 63);
    out.m[limb] |= m << r;
    if (r && limb + 1 < ops.n()) out.m[limb + 1] |= m >> (64 - r);
    out.neg = v < 0.0;
    return 0;
}

bool above_four(const FixOps& ops, const Fix& a) {
    if (a.m[ops.k] != 4) return a.m[ops.k] > 4;
    for (int i = 0; i < ops.k; i++) if (a.m[i]) return true;
    return false;
}

}  // namespace

int mc::exact_prepare(const char* fn, const mc_mandelbrot_orbit* o, uint32_t max_iter, uint32_t extra_limbs, uint64_t n_pixels,
                      const double* dcx, const double* dcy, int32_t dc_exp2, const uint32_t* out_n, ExactPixels* px) {
    if (!o || !dcx || !dcy || !out_n) return refuse(fn, "NULL argument");
    if (n_pixels == 0 || n_pixels > (1u << 20)) return refuse(fn, "n_pixels must be in [1, 2^20]");
    if (max_iter == 0 || max_iter == 0xffffffffu) return refuse(fn, "max_iter must be in [1, 2^32 - 2]");
    const int k0 = (int)((o->bits + 63) / 64);
    if ((int)o->cx.size() != k0 + 1 || (int)o->cy.size() != k0 + 1) return refuse(fn, "the orbit object carries no centre");
    if (extra_limbs > 131u || k0 + 1 + (int)extra_limbs > kMaxFrac + 1)
        return refuse(fn, "more than 131 limbs (" + std::to_string(k0 + 1) + " of the orbit plus " + std::to_string(extra_limbs) + " extra)",
                      MC_ERR_UNSUPPORTED);
    const FixOps ops{k0 + (int)extra_limbs};
    const int n = ops.n();
    Fix rx, ry, off, c;
    ops.zero(rx); ops.zero(ry);
    for (int i = 0; i <= k0; i++) { rx.m[i + extra_limbs] = o->cx[i]; ry.m[i + extra_limbs] = o->cy[i]; }
    rx.neg = o->cx_neg; ry.neg = o->cy_neg;
    try {
        px->n = n;
        px->cx.assign((size_t)n_pixels * n, 0u);
        px->cy.assign((size_t)n_pixels * n, 0u);
        px->cx_neg.assign(n_pixels, 0u);
        px->cy_neg.assign(n_pixels, 0u);
    } catch (const std::bad_alloc&) {
        return MC_ERR_OUT_OF_MEMORY;
    }
    for (uint64_t p = 0; p < n_pixels; p++) {
        for (int axis = 0; axis < 2; axis++) {
            const double v = axis ? dcy[p] : dcx[p];
            const std::string who = std::string("pixel ") + std::to_string(p) + (axis ? ": dcy" : ": dcx");
            if (!std::isfinite(v)) return refuse(fn, who + " is not finite");
            const int bad = offset_fix(ops, v, dc_exp2, off);
            if (bad == 1)
                return refuse(fn, who + " * 2^dc_exp2 has bits below 2^-" + std::to_string(64 * ops.k) + ", the last fractional bit of " +
                                      std::to_string(n) + " limbs (never truncated: raise extra_limbs)", MC_ERR_UNSUPPORTED);
            if (bad == 0) ops.add(axis ? ry : rx, off, c);
            if (bad == 2 || above_four(ops, c)) return refuse(fn, who + ": |c| above 4", MC_ERR_UNSUPPORTED);
            std::memcpy((axis ? px->cy.data() : px->cx.data()) + (size_t)p * n, c.m, (size_t)n * sizeof(uint64_t));
            (axis ? px->cy_neg : px->cx_neg)[p] = c.neg;
        }
    }
    return MC_OK;
}

void mc::fix_mul_round(int n, const uint64_t* a, const uint64_t* b, uint64_t* r) {
    const FixOps ops{n - 1};
    Fix fa, fb, fr;
    ops.zero(fa); ops.zero(fb);
    std::memcpy(fa.m, a, (size_t)n * sizeof(uint64_t));
    std::memcpy(fb.m, b, (size_t)n * sizeof(uint64_t));
    ops.mul(fa, fb, fr);
    std::memcpy(r, fr.m, (size_t)n * sizeof(uint64_t));
}

// host_loop without the doubles.
uint32_t mc::exact_count_host(int n, const uint64_t* cxm, const uint64_t* cym, bool cx_neg, bool cy_neg, uint32_t max_iter) {
    const FixOps ops{n - 1};
    Fix cx, cy, zx, zy, sx, sy, t;
    ops.zero(cx); ops.zero(cy);
    std::memcpy(cx.m, cxm, (size_t)n * sizeof(uint64_t));
    std::memcpy(cy.m, cym, (size_t)n * sizeof(uint64_t));
    cx.neg = cx_neg; cy.neg = cy_neg;
    ops.zero(zx); ops.zero(zy); ops.zero(sx); ops.zero(sy);
    for (uint32_t j = 0; j < max_iter; j++) {
        ops.mul(zx, zy, t);
        ops.twice(t);
        ops.add(t, cy, zy);
        ops.sub(sx, sy, t);
        ops.add(t, cx, zx);
        ops.mul(zx, zx, sx);
        ops.mul(zy, zy, sy);
        ops.add(sx, sy, t);
        if (ops.above_two(t)) return j;
    }
    return max_iter;
}

extern "C" {

int mc_mandelbrot_orbit_create(const char* centre_x, const char* centre_y, double scale_x, double scale_y, uint32_t max_iter,
                               mc_mandelbrot_orbit** out) {
    const char* fn = "mc_mandelbrot_orbit_create";
    if (int rc = check_arguments(fn, centre_x, centre_y, scale_x, scale_y, max_iter, out)) return rc;
    return create_scaled(fn, {}, centre_x, centre_y, plain_scale(scale_x, scale_y), max_iter, out);
}

int mc_mandelbrot_orbit_create_deep(const char* centre_x, const char* centre_y, double scale_x, double scale_y, int32_t scale_exp2,
                                    uint32_t max_iter, mc_mandelbrot_orbit** out) {
    return mc::orbit_create("mc_mandelbrot_orbit_create_deep", "mc_mandelbrot_orbit_create", {}, centre_x, centre_y, scale_x, scale_y,
                            scale_exp2, max_iter, out);
}

// The table of `o` under another scale of the same centre (include/mc_compute.h).
int mc_mandelbrot_orbit_rescale(const mc_mandelbrot_orbit* o, double scale_x, double scale_y, int32_t scale_exp2,
                                mc_mandelbrot_orbit** out) {
    const char* fn = "mc_mandelbrot_orbit_rescale";
    if (!out || !o) return refuse(fn, "NULL argument");
    *out = nullptr;
    if (!std::isfinite(scale_x) || !std::isfinite(scale_y) || scale_x == 0.0 || scale_y == 0.0)
        return refuse(fn, "scale_x and scale_y must be finite and nonzero");
    OrbitScale s;
    if (int rc = normalise_scale(fn, scale_x, scale_y, scale_exp2, &s)) return rc;
    if (s.below_floor) return refuse(fn, below_floor_text(s.deep), MC_ERR_UNSUPPORTED);
    if (s.bits > (int64_t)o->bits)
        return refuse(fn, "the orbit was computed for a shallower view (it carries " + std::to_string(o->bits) +
                              " fractional bits, this scale asks for " + std::to_string(s.bits) + ")", MC_ERR_UNSUPPORTED);
    mc_mandelbrot_orbit* r = new (std::nothrow) mc_mandelbrot_orbit();
    if (!r) return MC_ERR_OUT_OF_MEMORY;
    try {
        r->z = o->z;
        r->cx = o->cx;
        r->cy = o->cy;
    } catch (const std::bad_alloc&) {
        delete r;
        return MC_ERR_OUT_OF_MEMORY;
    }
    r->length = o->length;
    r->max_iter = o->max_iter;
    r->bits = o->bits;
    r->cx_neg = o->cx_neg;
    r->cy_neg = o->cy_neg;
    store_scale(r, s);
    *out = r;
    return MC_OK;
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

// The BLA table of include/mc_compute.h (MC_PRECISION_PERTURB_BLA), operation by operation.
int mc_mandelbrot_orbit_bla(mc_mandelbrot_orbit* o, uint32_t* levels, uint64_t* entries) {
    if (!o) return refuse("mc_mandelbrot_orbit_bla", "NULL orbit");
    if (o->deep)
        return refuse("mc_mandelbrot_orbit_bla", "a deep orbit (min |scale| < 2^-960) renders by the rescaled loop, which has no BLA",
                      MC_ERR_UNSUPPORTED);
    if (!o->has_bla) {
        const mc::blatab::Shape sh = mc::blatab::shape(o->length);
        const uint64_t n0 = sh.n0, total = sh.total;
        const uint32_t nlev = sh.levels;
        std::vector<double> t;
        try {
            t.resize(5 * total);
        } catch (const std::bad_alloc&) {
            return refuse("mc_mandelbrot_orbit_bla", "the table does not fit in host memory", MC_ERR_OUT_OF_MEMORY);
        }
        const double cm = mc::blatab::plain_cm(o->scale_x, o->scale_y);
        for (uint64_t j = 1; j <= n0; j++) mc::blatab::plain_level0(o->z[2 * j], o->z[2 * j + 1], &t[5 * (j - 1)]);
        uint64_t prev = 0, off = n0;   // level k-1 starts at prev, level k at off
        for (uint32_t k = 1; k < nlev; k++) {
            const uint64_t cnt = n0 >> k;
            for (uint64_t q = 0; q < cnt; q++)   // x = (k-1, m), m = 1 + q 2^k, then y = (k-1, m + 2^(k-1))
                mc::blatab::plain_merge(&t[5 * (prev + 2 * q)], &t[5 * (prev + 2 * q + 1)], cm, &t[5 * (off + q)]);
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

// The floatexp BLA table of include/mc_compute.h (MC_PRECISION_PERTURB_BLA_DEEP), operation by operation.
int mc_mandelbrot_orbit_bla_deep(mc_mandelbrot_orbit* o, uint32_t* levels, uint64_t* entries) {
    if (!o) return refuse("mc_mandelbrot_orbit_bla_deep", "NULL orbit");
    if (!o->has_bla_deep) {
        const mc::blatab::Shape sh = mc::blatab::shape(o->length);
        const uint64_t n0 = sh.n0, total = sh.total;
        const uint32_t nlev = sh.levels;
        std::vector<mc::BlaDeepRec> t;
        try {
            t.resize(total);
        } catch (const std::bad_alloc&) {
            return refuse("mc_mandelbrot_orbit_bla_deep", "the table does not fit in host memory", MC_ERR_OUT_OF_MEMORY);
        }
        const mc::blatab::Fx cm = mc::blatab::deep_cm(o->scale_x, o->scale_y, o->deep, o->scale_exp2);
        for (uint64_t j = 1; j <= n0; j++) mc::blatab::deep_level0(o->z[2 * j], o->z[2 * j + 1], t[j - 1]);
        uint64_t prev = 0, off = n0;   // level k-1 starts at prev, level k at off
        for (uint32_t k = 1; k < nlev; k++) {
            const uint64_t cnt = n0 >> k;
            for (uint64_t q = 0; q < cnt; q++)   // x = (k-1, m), m = 1 + q 2^k, then y = (k-1, m + 2^(k-1))
                mc::blatab::deep_merge(t[prev + 2 * q], t[prev + 2 * q + 1], cm, t[off + q]);
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

// The offsets the perturbation kernels use (mandel_perturb.hip: ensure_dc_table), in source order.
int mc_mandelbrot_exact_pixel_offsets(const mc_mandelbrot_orbit* o, uint32_t width, uint32_t height, uint64_t n_pixels, const uint32_t* gx,
                                      const uint32_t* gy, double* dcx, double* dcy, int32_t* dc_exp2) {
    const char* fn = "mc_mandelbrot_exact_pixel_offsets";
    if (!o || !gx || !gy || !dcx || !dcy || !dc_exp2) return refuse(fn, "NULL argument");
    if (width == 0 || height == 0 || width > (1u << 20) || height > (1u << 20)) return refuse(fn, "width and height must be in [1, 2^20]");
    if (n_pixels == 0 || n_pixels > (1u << 20)) return refuse(fn, "n_pixels must be in [1, 2^20]");
    for (uint64_t p = 0; p < n_pixels; p++)
        if (gx[p] >= width || gy[p] >= height) return refuse(fn, "pixel " + std::to_string(p) + " lies outside the view");
    for (uint64_t p = 0; p < n_pixels; p++) {
        dcx[p] = ((double)gx[p] / (double)width - 0.5) * o->scale_x;
        dcy[p] = ((double)gy[p] / (double)height - 0.5) * o->scale_y;
    }
    *dc_exp2 = o->deep ? o->scale_exp2 : 0;
    return MC_OK;
}

int mc_mandelbrot_exact_counts(const mc_mandelbrot_orbit* o, uint32_t max_iter, uint32_t extra_limbs, uint64_t n_pixels, const double* dcx,
                               const double* dcy, int32_t dc_exp2, uint32_t* out_n) {
    mc::ExactPixels px;
    if (int rc = mc::exact_prepare("mc_mandelbrot_exact_counts", o, max_iter, extra_limbs, n_pixels, dcx, dcy, dc_exp2, out_n, &px)) return rc;
    for (uint64_t p = 0; p < n_pixels; p++)
        out_n[p] = mc::exact_count_host(px.n, &px.cx[(size_t)p * px.n], &px.cy[(size_t)p * px.n], px.cx_neg[p] != 0, px.cy_neg[p] != 0,
                                        max_iter);
    return MC_OK;
}

}  // extern "C"
