// Locating minibrots, the host side (include/mc_compute.h: "atom domains"): the scan of a caller's sequence with the
// kernels' own update (mandel_atom.h), the domains of a host plane, Newton's method in perturbation space and the centre as decimal text.
// Plain C++17 and no HIP header, like mandel_orbit.cpp: it also builds and runs on its own (tools/mandel_atom_host_check.cpp).
// IEEE double, one operation at a time in source order: built with -ffp-contract=off like every other unit.
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "mandel_atom.h"
#include "mandel_orbit.h"

namespace {

int refuse(const char* fn, const std::string& why, int status = MC_ERR_INVALID_ARGUMENT) {
    mc::set_error_detail(std::string(fn) + ": " + why);
    return status;
}

uint64_t bits_of(double v) {
    uint64_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}

struct C2 {
    double x, y;
};

// One Newton step's iteration: z_p and D = dz_p/dc of c = c_ref + o over the orbit's table, the contract's loop.
void iterate(const mc_mandelbrot_orbit* orb, uint32_t period, C2 o, C2* z_out, C2* D_out) {
    const double* Z = orb->z.data();
    const uint32_t L = orb->length;
    double dx = 0.0, dy = 0.0, zmx = 0.0, zmy = 0.0, Dx = 0.0, Dy = 0.0;
    uint32_t m = 0;
    for (uint32_t k = 0; k < period; k++) {
        const double zkx = m == 0u ? dx : zmx + dx, zky = m == 0u ? dy : zmy + dy;   // z_k, as StatePerturb::escape_z forms it
        const double tx = zkx + zkx, ty = zky + zky;
        const double nDx = ((tx * Dx) - (ty * Dy)) + 1.0, nDy = (tx * Dy) + (ty * Dx);
        Dx = nDx; Dy = nDy;
        // StatePerturb::step with dc = o
        m = m + 1u;
        const uint32_t j = m < L ? m : L;
        const double z1x = Z[2 * (size_t)j], z1y = Z[2 * (size_t)j + 1];
        const double ax = (zmx + zmx) + dx, ay = (zmy + zmy) + dy;
        const double ndx = ((ax * dx) - (ay * dy)) + o.x, ndy = ((ax * dy) + (ay * dx)) + o.y;
        const double zx = z1x + ndx, zy = z1y + ndy;
        const double r = (zx * zx) + (zy * zy);
        if (m == L || r < ((ndx * ndx) + (ndy * ndy))) { dx = zx; dy = zy; m = 0; zmx = zmy = 0.0; }
        else { dx = ndx; dy = ndy; zmx = z1x; zmy = z1y; }
    }
    z_out->x = m == 0u ? dx : zmx + dx;
    z_out->y = m == 0u ? dy : zmy + dy;
    D_out->x = Dx;
    D_out->y = Dy;
}

// z / D by Smith's division: |D|^2 is never formed (it overflows at 1e-150 and below).
C2 smith(C2 z, C2 D) {
    C2 q;
    if (std::fabs(D.x) >= std::fabs(D.y)) {
        const double r = D.y / D.x, den = D.x + (D.y * r);
        q.x = (z.x + (z.y * r)) / den;
        q.y = (z.y - (z.x * r)) / den;
    } else {
        const double r = D.x / D.y, den = D.y + (D.x * r);
        q.x = ((z.x * r) + z.y) / den;
        q.y = ((z.y * r) - z.x) / den;
    }
    return q;
}

// ---- multi-limb magnitudes for the centre's text: least significant limb first ---------------------------------------------------------
using Limbs = std::vector<uint64_t>;

int cmp_mag(const Limbs& a, const Limbs& b) {
    for (size_t i = a.size(); i-- > 0;)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return 0;
}
void add_mag(Limbs& a, const Limbs& b) {   // a += b (same size; the caller leaves head room)
    unsigned __int128 c = 0;
    for (size_t i = 0; i < a.size(); i++) { c += (unsigned __int128)a[i] + b[i]; a[i] = (uint64_t)c; c >>= 64; }
}
void sub_mag(Limbs& a, const Limbs& b) {   // a -= b, a >= b
    uint64_t borrow = 0;
    for (size_t i = 0; i < a.size(); i++) {
        const uint64_t t = a[i] - b[i], b1 = a[i] < b[i];
        a[i] = t - borrow;
        borrow = b1 | (t < borrow);
    }
}

// One coordinate: (centre limbs, sign) + v * 2^exp2, exactly, as sign, integer part and `frac` fractional limbs.
struct Sum {
    Limbs m;        // frac fractional limbs, then two integer limbs
    size_t frac;
    bool neg;
};
Sum exact_sum(const std::vector<uint64_t>& centre, bool centre_neg, double v, int64_t exp2) {
    const size_t k0 = centre.size() - 1;   // the centre's fractional limbs
    uint64_t mant = 0;
    int64_t low = 0;                       // |v| 2^exp2 = mant 2^low, mant odd (or v = 0)
    if (v != 0.0) {
        int e = 0;
        const double f = std::frexp(std::fabs(v), &e);
        mant = (uint64_t)std::ldexp(f, 53);
        const int tz = __builtin_ctzll(mant);
        mant >>= tz;
        low = (int64_t)e - 53 + tz + exp2;
    }
    size_t extra = 0;                      // zero limbs below the centre's, as many as the offset's lowest bit needs
    if (mant && low < -(int64_t)(64 * k0)) extra = (size_t)((-low - (int64_t)(64 * k0) + 63) / 64);
    Sum s;
    s.frac = k0 + extra;
    s.m.assign(s.frac + 2, 0u);
    for (size_t i = 0; i <= k0; i++) s.m[extra + i] = centre[i];
    s.neg = centre_neg;
    if (mant) {
        Limbs off(s.m.size(), 0u);
        const int64_t pos = low + (int64_t)(64 * s.frac);   // >= 0
        const size_t limb = (size_t)(pos >> 6);
        const int r = (int)(pos & 63);
        if (limb < off.size()) off[limb] |= mant << r;
        if (r && limb + 1 < off.size()) off[limb + 1] |= mant >> (64 - r);
        const bool off_neg = v < 0.0;
        if (off_neg == s.neg) add_mag(s.m, off);
        else if (cmp_mag(s.m, off) >= 0) sub_mag(s.m, off);
        else { Limbs t = off; sub_mag(t, s.m); s.m = t; s.neg = off_neg; }
    }
    bool zero = true;
    for (uint64_t w : s.m) zero = zero && w == 0u;
    if (zero) s.neg = false;
    return s;
}

// [-]I.FFF with frac_digits fractional digits, truncated toward zero.  The integer part is below 2^64 here.
std::string decimal(Sum s, uint32_t frac_digits) {
    std::string out = s.neg ? "-" : "";
    out += std::to_string((unsigned long long)s.m[s.frac]);
    if (!frac_digits) return out;
    out += '.';
    Limbs f(s.m.begin(), s.m.begin() + (long)s.frac);
    size_t lo = 0;   // limbs below lo are zero: multiplying by 10 only adds zeros there
    for (uint32_t d = 0; d < frac_digits; d++) {
        while (lo < f.size() && f[lo] == 0u) lo++;
        unsigned __int128 c = 0;
        for (size_t i = lo; i < f.size(); i++) { c += (unsigned __int128)f[i] * 10u; f[i] = (uint64_t)c; c >>= 64; }
        out += (char)('0' + (int)(uint64_t)c);
    }
    return out;
}

}  // namespace

extern "C" {

int mc_mandelbrot_atom_scan(const double* z, uint32_t n, uint32_t* period, double* amin) {
    if ((!z && n) || !period || !amin) return MC_ERR_INVALID_ARGUMENT;
    double best = __builtin_inf();
    uint32_t per = 0u;
    for (uint32_t m = 1; m <= n; m++) mc::atom::update(best, per, m, z[2 * (size_t)(m - 1)], z[2 * (size_t)(m - 1) + 1]);
    *period = per;
    *amin = best;
    return MC_OK;
}

int mc_mandelbrot_atom_domains(const uint32_t* period, const double* amin, uint64_t n_pixels, uint32_t max_iter, uint32_t* count,
                               double* amin_table, uint32_t* pixel) {
    const char* fn = "mc_mandelbrot_atom_domains";
    if (!period || !amin || !count || !amin_table || !pixel) return refuse(fn, "NULL argument");
    if (n_pixels > 0xffffffffull) return refuse(fn, "pixel indices are uint32_t: n_pixels must stay below 2^32");
    if (max_iter == 0xffffffffu) return refuse(fn, "max_iter + 1 entries must be countable in 32 bits");
    for (uint64_t i = 0; i < n_pixels; i++)
        if (period[i] > max_iter) return refuse(fn, "pixel " + std::to_string(i) + ": period " + std::to_string(period[i]) + " above max_iter");
    const double inf = __builtin_inf();
    for (uint64_t v = 0; v <= max_iter; v++) { count[v] = 0u; amin_table[v] = inf; pixel[v] = mc::atom::kNoPixel; }
    for (uint64_t i = 0; i < n_pixels; i++) {   // ascending i and a strict comparison: the lowest index attaining the minimum
        const uint32_t v = period[i];
        const uint64_t key = bits_of(amin[i]);
        count[v]++;
        if (key > mc::atom::kInfBits) continue;   // a negative value or a NaN: counted, never a minimum
        const uint64_t cur = bits_of(amin_table[v]);
        if (key < cur || (key == cur && pixel[v] == mc::atom::kNoPixel)) { amin_table[v] = amin[i]; pixel[v] = (uint32_t)i; }
    }
    return MC_OK;
}

int mc_mandelbrot_nucleus_refine(const mc_mandelbrot_orbit* o, uint32_t period, uint32_t max_steps, double offset[2], uint32_t* steps,
                                 double last_step[2]) {
    const char* fn = "mc_mandelbrot_nucleus_refine";
    if (!o || !offset || !steps || !last_step) return refuse(fn, "NULL argument");
    if (o->deep) return refuse(fn, "a deep orbit (min |scale| < 2^-960): the offsets leave the double range");
    if (period == 0u) return refuse(fn, "period must be at least 1");
    if (period > o->max_iter) return refuse(fn, "period above the orbit's max_iter");
    if (max_steps == 0u) return refuse(fn, "max_steps must be at least 1");
    if (!o->length || o->z.size() < 2 * ((size_t)o->length + 1)) return refuse(fn, "the orbit object carries no table");
    C2 c = {offset[0], offset[1]};
    if (!std::isfinite(c.x) || !std::isfinite(c.y)) return refuse(fn, "the start offset is not finite");
    *steps = 0u;
    last_step[0] = last_step[1] = 0.0;
    const double eps = std::ldexp(1.0, -52);
    for (uint32_t s = 1; s <= max_steps; s++) {
        C2 z, D;
        iterate(o, period, c, &z, &D);
        const std::string at = "step " + std::to_string(s);
        if (!std::isfinite(D.x) || !std::isfinite(D.y)) return refuse(fn, at + ": the derivative is not finite", MC_ERR_UNSUPPORTED);
        const C2 q = smith(z, D);
        if (!std::isfinite(q.x) || !std::isfinite(q.y)) return refuse(fn, at + ": the Newton step z / D is not finite", MC_ERR_UNSUPPORTED);
        c.x = c.x - q.x;
        c.y = c.y - q.y;
        if (!std::isfinite(c.x) || !std::isfinite(c.y)) return refuse(fn, at + ": the offset is not finite", MC_ERR_UNSUPPORTED);
        offset[0] = c.x; offset[1] = c.y;
        last_step[0] = q.x; last_step[1] = q.y;
        *steps = s;
        const double qa = std::fmax(std::fabs(q.x), std::fabs(q.y)), oa = std::fmax(std::fabs(c.x), std::fabs(c.y));
        if (qa <= eps * oa) break;
    }
    return MC_OK;
}

int mc_mandelbrot_orbit_offset_text(const mc_mandelbrot_orbit* o, double ox, double oy, uint32_t frac_digits, char* out_x, char* out_y,
                                    size_t capacity) {
    const char* fn = "mc_mandelbrot_orbit_offset_text";
    if (!o || !out_x || !out_y) return refuse(fn, "NULL argument");
    if (!std::isfinite(ox) || !std::isfinite(oy)) return refuse(fn, "the offset is not finite");
    if (frac_digits > 1000000u) return refuse(fn, "frac_digits above 1000000");
    const size_t k0 = ((size_t)o->bits + 63) / 64;
    if (o->cx.size() != k0 + 1 || o->cy.size() != k0 + 1) return refuse(fn, "the orbit object carries no centre");
    const int64_t e2 = o->deep ? (int64_t)o->scale_exp2 : 0;
    try {
        const std::string sx = decimal(exact_sum(o->cx, o->cx_neg, ox, e2), frac_digits);
        const std::string sy = decimal(exact_sum(o->cy, o->cy_neg, oy, e2), frac_digits);
        const size_t need = (sx.size() > sy.size() ? sx.size() : sy.size()) + 1;
        if (capacity < need) return refuse(fn, "capacity " + std::to_string(capacity) + " is too small: " + std::to_string(need) + " bytes needed");
        std::memcpy(out_x, sx.c_str(), sx.size() + 1);
        std::memcpy(out_y, sy.c_str(), sy.size() + 1);
    } catch (const std::bad_alloc&) {
        return MC_ERR_OUT_OF_MEMORY;
    }
    return MC_OK;
}

}  // extern "C"
