// The reference orbit's host side (mandel_orbit.cpp): the object, its constructor and the one seam to an iteration loop that runs
// elsewhere.  Plain C++17 and no HIP header, so that mandel_orbit.cpp also builds and runs on its own (tools/orbit_host_check.cpp).
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/mc_compute.h"

namespace mc {

// MC_PRECISION_PERTURB_BLA_DEEP: one entry of the table of mc_mandelbrot_orbit_bla_deep, mantissas and exponents together in one 64-byte
// record, so that a probe reads a single record.  The kernel reads this layout (mandel_perturb_bla_deep.hip).
struct BlaDeepRec {
    double ax, ay, bx, by, r;        // the mantissas: A = (ax, ay) * 2^ea, B = (bx, by) * 2^eb, R = r * 2^er
    int32_t ea, eb, er, pad[3];
};
static_assert(sizeof(BlaDeepRec) == 64, "one table entry is one 64-byte record");

}  // namespace mc

struct mc_mandelbrot_orbit {
    std::vector<double> z;   // (L + 1) * 2: re, im
    uint32_t length = 0, max_iter = 0, bits = 0;
    double scale_x = 0.0, scale_y = 0.0;   // the scale as doubles; a deep orbit: the mantissas
    int32_t scale_exp2 = 0;                // a deep orbit: the scale is (scale_x, scale_y) * 2^scale_exp2
    bool deep = false;                     // min |scale| < 2^-960: rendered by the deep kernel (mandel_perturb_deep.hip)
    // MC_PRECISION_PERTURB_BLA: the table of mc_mandelbrot_orbit_bla, level-major (A.x, A.y, B.x, B.y, R) per entry
    std::vector<double> bla;
    uint32_t bla_levels = 0;
    uint64_t bla_entries = 0;
    bool has_bla = false;                  // built (a table may have no entry: L < 3)
    // MC_PRECISION_PERTURB_BLA_DEEP: the floatexp table of mc_mandelbrot_orbit_bla_deep, same layout, one record per entry
    std::vector<mc::BlaDeepRec> bla_deep;
    uint32_t bla_deep_levels = 0;
    uint64_t bla_deep_entries = 0;
    bool has_bla_deep = false;
    // The centre as the constructor parsed it: ceil(bits / 64) + 1 limbs each, least significant first (the last is the integer limb),
    // sign and magnitude.  What mc_mandelbrot_exact_counts iterates from; mc_mandelbrot_orbit_rescale copies it.
    std::vector<uint64_t> cx, cy;
    bool cx_neg = false, cy_neg = false;
};

namespace mc {

void set_error_detail(const std::string& s);   // api.hip (the stand-alone check brings its own)

// "Run the iteration loop": cx, cy are the centre's k + 1 limbs (least significant first) with their signs.  z holds Z_0 on entry and
// Z_0 .. Z_L on success (MC_OK, *length = L).  kOrbitTinyEntry: the tiny-entry refusal at Z_(*tiny_j); any other value is returned to the
// caller as the status.  A std::bad_alloc from z may pass through: orbit_create catches it.
constexpr int kOrbitTinyEntry = -1;
using OrbitLoop = std::function<int(int k, const uint64_t* cx, const uint64_t* cy, bool cx_neg, bool cy_neg, uint32_t max_iter, bool deep,
                                    std::vector<double>& z, uint32_t* length, uint32_t* tiny_j)>;

// mc_mandelbrot_orbit_create_deep under the name `fn` in the error detail; a scale that is a double of at least 2^-960 is exactly
// mc_mandelbrot_orbit_create under the name `fn_plain`.  An empty loop runs the host's own (FixOps).
int orbit_create(const char* fn, const char* fn_plain, const OrbitLoop& loop, const char* centre_x, const char* centre_y, double scale_x,
                 double scale_y, int32_t scale_exp2, uint32_t max_iter, mc_mandelbrot_orbit** out);

// mc_mandelbrot_exact_counts (include/mc_compute.h): every check of the arguments and every pixel's c = c_ref + offset, added exactly.
// n limbs per number; cx / cy hold pixel p's magnitude at [p * n, (p + 1) * n), least significant limb first.  `fn` names the entry point
// in the error detail.  The device form (mandel_exact.hip) uploads these; the host form iterates them with FixOps.
struct ExactPixels {
    int n = 0;
    std::vector<uint64_t> cx, cy;
    std::vector<uint8_t> cx_neg, cy_neg;
};
int exact_prepare(const char* fn, const mc_mandelbrot_orbit* o, uint32_t max_iter, uint32_t extra_limbs, uint64_t n_pixels,
                  const double* dcx, const double* dcy, int32_t dc_exp2, const uint32_t* out_n, ExactPixels* px);
// FixOps::mul on magnitudes of n limbs (n - 1 fractional): r = (a b + 2^(F - 1)) >> F.  For tools/mandel_exact_host_check.cpp.
void fix_mul_round(int n, const uint64_t* a, const uint64_t* b, uint64_t* r);
// The contract's loop on FixOps for one c of n limbs: the count in [0, max_iter].
uint32_t exact_count_host(int n, const uint64_t* cx, const uint64_t* cy, bool cx_neg, bool cy_neg, uint32_t max_iter);

}  // namespace mc
