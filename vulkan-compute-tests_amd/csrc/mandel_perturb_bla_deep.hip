// MC_PRECISION_PERTURB_BLA_DEEP: the rescaled loop of mandel_perturb_deep.hip with bilinear skips (include/mc_compute.h states the
// contract).
//
// A pixel's offset is delta = w * 2^S exactly (§3.7's state: w, S, the phase, m), and each trip either SKIPS 2^k iterations by one
// entry of the host's floatexp table or runs §3.7's rescaled iteration exactly (escape, rebase and the Z = 0 rule included).
//  * the level: the trip structure of mandel_perturb_bla.hip: level 1 first, then the top level the alignment, the orbit's end and the
//    iterations left allow, then bisection.  The radius test N1(w) 2^S < R is ldexp(N1(w), S - er) < r: exact (R's mantissa r is 0 or
//    in [0.5, 1), so a result that under- or overflows compares as the exact value would).
//  * a skip: P = A w at exponent ea + S, Q = B u at exponent eb + E, aligned with ldexp at the larger frexp exponent, added and
//    normalised; then the plain phase (S = 0, w = d) if |delta'|inf >= T, else the scaled phase with the normalised mantissas and their
//    exponent (delta' = 0: w = 0, S = E, as at the start).
//  * a table entry is one 64-byte record (5 mantissas, 3 exponents), so a probe is one record read.
//  * IEEE double in source order (-ffp-contract=off), fp64 denormals kept; ldexp = v_ldexp_f64, the exponent = v_frexp_exp_i32_f64.
#include "mandel_kernels.h"
#include "mandel_perturb.h"
#include "mc_internal.h"

namespace mc {

namespace {

constexpr double kT = 0x1p-500;        // the phase threshold T
constexpr double kWinHi = 0x1p256;     // the renormalisation window of |w|inf
constexpr double kWinLo = 0x1p-256;

__device__ __forceinline__ double pow2(int k) { return __builtin_amdgcn_ldexp(1.0, k); }
__device__ __forceinline__ double ldexp2(double x, int k) { return __builtin_amdgcn_ldexp(x, k); }
__device__ __forceinline__ int frexp_exp(double x) { return __builtin_amdgcn_frexp_exp(x); }

// S(n) = sum over j >= 0 of floor(n / 2^j) = 2n - popcount(n): level k of the table starts at entry S(n) - S(n >> k), n = L - 2
__device__ __forceinline__ uint64_t level_sum(uint64_t n) { return 2u * n - (uint64_t)__popcll(n); }

// ONE kernel body over the mapping policies of mandel_kernels.h (MapTile, MapList, MapSmoothTile, MapSmoothList; x is what the mapping
// takes beside a: nothing, the sample list, the q plane, the smooth sample list).  The loop stands lexically in the body: inlined from a
// __device__ function it leaves the register allocator with two operands of one v_add3_u32 swapped.  The smooth
// mappings keep the escaping z (the loop leaves at its one escape test) and form c after the loop.
template <class Map, class... X>
__global__ void __launch_bounds__(64) mandel_perturb_bla_deep_kernel(PerturbBlaDeepArgs a, X... x) {
    const auto ln = Map::lane(a.t, x...);
    const uint32_t gx = ln.gx, gy = ln.gy;
    const bool valid = ln.valid;
    [[maybe_unused]] double ezx = 0.0, ezy = 0.0;   // MC_MANDEL_COLOUR_SMOOTH: the escaping z (the loop leaves at its one escape test)
    const double2* __restrict__ Z = a.t.orbit;
    const BlaDeepRec* __restrict__ T = a.bla;
    const uint32_t L = a.t.L, M = a.t.max_iter;
    const int32_t E = a.exp2;
    const uint64_t n0 = L >= 3u ? (uint64_t)L - 2u : 0u;   // level 0's entries
    const uint64_t s0 = level_sum(n0);
    const double ux = a.t.table[valid ? gx : 0u], uy = a.t.table[a.t.W + (valid ? gy : 0u)];
    double wx = 0.0, wy = 0.0, dx = 0.0, dy = 0.0;   // delta = w * 2^S;  d = ldexp(w, S)
    int32_t S = E;
    bool scaled = true;
    uint32_t m = 0u, i = valid ? 0u : M, n = M, trips = 0u;
    while (i < M) {
        trips++;
        // the step's orbit entries, issued before the probes (m <= L-1 here, so m + 1 <= L)
        const double2 zm = Z[m], z1 = Z[m + 1u];
        uint32_t kcap = 0u;
        if (m >= 1u && L - 1u - m >= 2u) {
            const uint32_t ka = m == 1u ? 31u : (uint32_t)__builtin_ctz(m - 1u);
            const uint32_t kl = 31u - (uint32_t)__builtin_clz(L - 1u - m);
            const uint32_t ki = 31u - (uint32_t)__builtin_clz(M - i);
            kcap = ka < kl ? ka : kl;
            kcap = kcap < ki ? kcap : ki;
        }
        const double nw = fabs(wx) + fabs(wy);
        uint32_t k = 0u;
        double Ax = 0.0, Ay = 0.0, Bx = 0.0, By = 0.0;
        int32_t eA = 0, eB = 0;
        if (kcap >= 1u) {
            // probe(kk): is N1(w) 2^S < R_kk(m)?  On success the entry's (A, B) are kept
            auto probe = [&](uint32_t kk) -> bool {
                const uint64_t e = (s0 - level_sum(n0 >> kk)) + (uint64_t)((m - 1u) >> kk);
                const BlaDeepRec t = T[e];
                if (!(ldexp2(nw, S - t.er) < t.r)) return false;
                Ax = t.ax; Ay = t.ay; Bx = t.bx; By = t.by; eA = t.ea; eB = t.eb;
                return true;
            };
            if (probe(1u)) {
                uint32_t lo = 1u, hi = kcap;   // level lo passes; the answer is in [lo, hi]
                if (hi > lo) {
                    if (probe(hi)) lo = hi;
                    else hi = hi - 1u;
                }
                while (lo < hi) {
                    const uint32_t mid = (lo + hi + 1u) >> 1;
                    if (probe(mid)) lo = mid;
                    else hi = mid - 1u;
                }
                k = lo;   // lo moves only on a passing probe, so (A, B) are level lo's entry
            }
        }
        if (k) {   // skip 2^k iterations: delta' = A delta + B u 2^E in floatexp; no escape test, no rebase test
            const double px = (Ax * wx) - (Ay * wy), py = (Ax * wy) + (Ay * wx);
            const double qx = (Bx * ux) - (By * uy), qy = (Bx * uy) + (By * ux);
            const double ap = fmax(fabs(px), fabs(py)), aq = fmax(fabs(qx), fabs(qy));
            const int32_t eP = eA + S, eQ = eB + E;
            double sx, sy;
            int32_t e;
            if (ap == 0.0) { sx = qx; sy = qy; e = eQ; }
            else if (aq == 0.0) { sx = px; sy = py; e = eP; }
            else {
                const int32_t kp = eP + frexp_exp(ap), kq = eQ + frexp_exp(aq);
                e = kp > kq ? kp : kq;
                sx = ldexp2(px, eP - e) + ldexp2(qx, eQ - e);
                sy = ldexp2(py, eP - e) + ldexp2(qy, eQ - e);
            }
            const double as = fmax(fabs(sx), fabs(sy));   // normalise: (sx, sy) 2^e with max part in [0.5, 1), or exactly 0
            if (as == 0.0) {
                wx = wy = dx = dy = 0.0;
                S = E;
                scaled = true;
            } else {
                const int32_t ks = frexp_exp(as);
                sx = ldexp2(sx, -ks); sy = ldexp2(sy, -ks);
                e = e + ks;
                dx = ldexp2(sx, e); dy = ldexp2(sy, e);
                if (fmax(fabs(dx), fabs(dy)) >= kT) { scaled = false; S = 0; wx = dx; wy = dy; }
                else { scaled = true; S = e; wx = sx; wy = sy; }
            }
            m = m + (1u << k);
            i = i + (1u << k);
        } else {   // §3.7's rescaled iteration i, exactly
            double nwx, nwy;
            int32_t nS = S;
            if (scaled && zm.x == 0.0 && zm.y == 0.0) {                     // Z_m = 0: a fresh exponent
                nS = max(S + S, E);
                const double px = pow2((S + S) - nS), pu = pow2(E - nS);
                nwx = (((wx * wx) - (wy * wy)) * px) + (ux * pu);
                nwy = (((wx * wy) + (wy * wx)) * px) + (uy * pu);
            } else {
                const double pu = pow2(E - S);
                const double ax = (zm.x + zm.x) + dx, ay = (zm.y + zm.y) + dy;
                nwx = ((ax * wx) - (ay * wy)) + (ux * pu);
                nwy = ((ax * wy) + (ay * wx)) + (uy * pu);
            }
            const double ndx = ldexp2(nwx, nS), ndy = ldexp2(nwy, nS);
            m = m + 1u;
            const double zx = z1.x + ndx, zy = z1.y + ndy;
            const double r = (zx * zx) + (zy * zy);
            if (r > 2.0) { if constexpr (Map::kSmooth) { ezx = zx; ezy = zy; } n = i; break; }
            if (m == L || r < ((ndx * ndx) + (ndy * ndy))) {                 // rebase: Z_0 = 0, delta = z
                m = 0u;
                dx = zx; dy = zy;
                const double am = fmax(fabs(zx), fabs(zy));
                if (am >= kT) { scaled = false; S = 0; wx = zx; wy = zy; }
                else {
                    scaled = true;
                    S = am == 0.0 ? E : frexp_exp(am);                       // exactly 0: restart as at the start
                    wx = ldexp2(zx, -S); wy = ldexp2(zy, -S);
                }
            } else {
                wx = nwx; wy = nwy; dx = ndx; dy = ndy; S = nS;
                if (scaled) {
                    if (fmax(fabs(ndx), fabs(ndy)) >= kT) { scaled = false; S = 0; wx = ndx; wy = ndy; }
                    else {
                        const double am = fmax(fabs(nwx), fabs(nwy));
                        if (am > kWinHi || am < kWinLo) {
                            const int32_t e = frexp_exp(am);
                            wx = ldexp2(nwx, -e); wy = ldexp2(nwy, -e);
                            S = nS + e;
                        }
                    }
                }
            }
            i = i + 1u;
        }
    }
    const uint32_t shown = a.count_trips ? trips : n;   // trips <= M: every trip but an escaping one advances i by at least one
    if constexpr (Map::kSmooth) {
        const double2 c1 = Z[1];
        Map::store(a.t, ln, x..., n, shown, ezx, ezy, c1.x + ldexp2(ux, E), c1.y + ldexp2(uy, E));
    } else {
        Map::store(a.t, ln, x..., n, shown);
    }
}

}  // namespace

int perturb_bla_deep_launch(const PerturbBlaDeepArgs& a, dim3 grid, hipStream_t s, const SampleList* list, SmoothOut smooth,
                            const SmoothSampleList* slist) {
    const MappingKernels<PerturbBlaDeepArgs> k = {
        mandel_perturb_bla_deep_kernel<MapTile>,
        mandel_perturb_bla_deep_kernel<MapList, SampleList>,
        mandel_perturb_bla_deep_kernel<MapSmoothTile, SmoothPlane>,
        mandel_perturb_bla_deep_kernel<MapSmoothList, SmoothSampleList>,
    };
    return launch_mapping(k, a, grid, s, list, smooth, slist);
}

}  // namespace mc
