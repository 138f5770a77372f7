// MC_PRECISION_PERTURB_BLA: PERTURB's loop with bilinear skips (include/mc_compute.h states the contract).
//
// Each pixel runs a loop of its own, one trip at a time: a trip either SKIPS 2^K iterations by one entry (A, B) of the host's BLA table,
// d' = A d + B dc, or runs PERTURB's iteration exactly (escape and rebase tests included).  The escape-time framework of mandel_escape.h
// is not used: its fast block assumes m advances by one per iteration, which a skip breaks.
//  * the level: the largest k >= 1 that the alignment of m, the orbit's end, the iterations left and the radius R_k(m) allow.  The valid
//    levels form a prefix (R_k(m) never increases with k), so the kernel probes level 1 first (a lane whose offset has grown fails it:
//    one probe), then the highest level the three limits allow, then bisects between them.  A probe reads the whole entry (40 B), so
//    the skip has (A, B) in registers once the level is known.
//  * divergence: lanes that skip and lanes that step in the same trip run both branches under the exec mask; a lane's trip is one or
//    the other, so the restatement's per-pixel loop is exactly what each lane computes.  Before any rebase and while every lane takes
//    the same level, a wave shares m and every table read is wave-uniform (one cache line per probe).
//  * IEEE double in source order (-ffp-contract=off), fp64 denormals kept.
#include "mandel_kernels.h"
#include "mandel_perturb.h"
#include "mc_internal.h"

namespace mc {

namespace {

// S(n) = sum over j >= 0 of floor(n / 2^j) = 2n - popcount(n): level k of the table starts at entry S(n) - S(n >> k), n = L - 2
__device__ __forceinline__ uint64_t level_sum(uint64_t n) { return 2u * n - (uint64_t)__popcll(n); }

// ONE kernel body over the mapping policies of mandel_kernels.h (MapTile, MapList, MapSmoothTile, MapSmoothList; x is what the mapping
// takes beside a: nothing, the sample list, the q plane, the smooth sample list).  The loop stands lexically in the body: inlined from a
// __device__ function it leaves the register allocator with two operands of one v_add3_u32 swapped.  The smooth
// mappings keep the escaping z (the loop leaves at its one escape test) and form c after the loop.
template <class Map, class... X>
__global__ void __launch_bounds__(64) mandel_perturb_bla_kernel(PerturbBlaArgs a, X... x) {
    const auto ln = Map::lane(a.t, x...);
    const uint32_t gx = ln.gx, gy = ln.gy;
    const bool valid = ln.valid;
    [[maybe_unused]] double ezx = 0.0, ezy = 0.0;   // MC_MANDEL_COLOUR_SMOOTH: the escaping z (the loop leaves at its one escape test)
    const double2* __restrict__ Z = a.t.orbit;
    const double* __restrict__ T = a.bla;
    const uint32_t L = a.t.L, M = a.t.max_iter;
    const uint64_t n0 = L >= 3u ? (uint64_t)L - 2u : 0u;   // level 0's entries
    const uint64_t s0 = level_sum(n0);
    const double dcx = a.t.table[valid ? gx : 0u], dcy = a.t.table[a.t.W + (valid ? gy : 0u)];
    double dx = 0.0, dy = 0.0;
    uint32_t m = 0u, i = valid ? 0u : M, n = M, trips = 0u;
    while (i < M) {
        trips++;
        // the step's orbit entries, issued before the probes (m <= L-1 here, so m + 1 <= L)
        const double2 zm = Z[m], z1 = Z[m + 1u];
        // kcap: the largest k the alignment ((m-1) divisible by 2^k), the orbit's end (m + 2^k <= L-1) and the iterations left
        // (i + 2^k <= M) allow; 0 = no level (m = 0, or fewer than two steps before Z_(L-1))
        uint32_t kcap = 0u;
        if (m >= 1u && L - 1u - m >= 2u) {
            const uint32_t ka = m == 1u ? 31u : (uint32_t)__builtin_ctz(m - 1u);
            const uint32_t kl = 31u - (uint32_t)__builtin_clz(L - 1u - m);
            const uint32_t ki = 31u - (uint32_t)__builtin_clz(M - i);
            kcap = ka < kl ? ka : kl;
            kcap = kcap < ki ? kcap : ki;
        }
        const double nd = fabs(dx) + fabs(dy);
        uint32_t k = 0u;
        double Ax = 0.0, Ay = 0.0, Bx = 0.0, By = 0.0;
        if (kcap >= 1u) {
            // probe(kk): is N1(d) < R_kk(m)?  On success the entry's (A, B) are kept
            auto probe = [&](uint32_t kk) -> bool {
                const uint64_t e = (s0 - level_sum(n0 >> kk)) + (uint64_t)((m - 1u) >> kk);
                const double* t = T + 5u * e;
                const double ax = t[0], ay = t[1], bx = t[2], by = t[3], r = t[4];
                if (!(nd < r)) return false;
                Ax = ax; Ay = ay; Bx = bx; By = by;
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
        if (k) {   // skip 2^k iterations: no escape test, no rebase test
            const double ndx = ((Ax * dx) - (Ay * dy)) + ((Bx * dcx) - (By * dcy));
            const double ndy = ((Ax * dy) + (Ay * dx)) + ((Bx * dcy) + (By * dcx));
            dx = ndx; dy = ndy;
            m = m + (1u << k);
            i = i + (1u << k);
        } else {   // PERTURB's iteration i, exactly
            const double ax = (zm.x + zm.x) + dx, ay = (zm.y + zm.y) + dy;
            const double ndx = ((ax * dx) - (ay * dy)) + dcx;
            const double ndy = ((ax * dy) + (ay * dx)) + dcy;
            m = m + 1u;
            const double zx = z1.x + ndx, zy = z1.y + ndy;
            const double r = (zx * zx) + (zy * zy);
            if (r > 2.0) { if constexpr (Map::kSmooth) { ezx = zx; ezy = zy; } n = i; break; }
            if (m == L || r < ((ndx * ndx) + (ndy * ndy))) { dx = zx; dy = zy; m = 0u; }   // rebase onto Z_0
            else { dx = ndx; dy = ndy; }
            i = i + 1u;
        }
    }
    const uint32_t shown = a.count_trips ? trips : n;   // trips <= M: every trip but an escaping one advances i by at least one
    if constexpr (Map::kSmooth) {
        const double2 c1 = Z[1];
        Map::store(a.t, ln, x..., n, shown, ezx, ezy, c1.x + dcx, c1.y + dcy);
    } else {
        Map::store(a.t, ln, x..., n, shown);
    }
}

}  // namespace

int perturb_bla_launch(const PerturbBlaArgs& a, dim3 grid, hipStream_t s, const SampleList* list, SmoothOut smooth,
                       const SmoothSampleList* slist) {
    const MappingKernels<PerturbBlaArgs> k = {
        mandel_perturb_bla_kernel<MapTile>,
        mandel_perturb_bla_kernel<MapList, SampleList>,
        mandel_perturb_bla_kernel<MapSmoothTile, SmoothPlane>,
        mandel_perturb_bla_kernel<MapSmoothList, SmoothSampleList>,
    };
    return launch_mapping(k, a, grid, s, list, smooth, slist);
}

}  // namespace mc
