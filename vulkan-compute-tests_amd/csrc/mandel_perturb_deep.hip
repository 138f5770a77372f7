// MC_PRECISION_PERTURB below 2^-960: rescaled perturbation (include/mc_compute.h states the contract).
//
// A pixel's offset from the reference orbit is carried as delta = w * 2^S exactly (w a double2, S a per-lane int), so that it keeps 53
// significant bits while it is far below the double range.  Two phases:
//  * plain (S = 0): StatePerturb's arithmetic, op for op; entered once |delta|inf >= T = 2^-500, left only by a rebase below T.
//  * scaled: w' = ((2 Z_m + 2^S w) w) + u 2^(E - S), each power of two ldexp(1, k) (0 below 2^-1074); a step at Z_m = 0 takes a fresh
//    exponent S' = max(2S, E) (delta^2 + dc can be far smaller than delta); w is renormalised to [0.5, 1) when |w|inf leaves
//    [2^-256, 2^256].
// The fast block runs U = 8 steps of the general formula with S fixed and the block's orbit entries fetched at its start; a lane that
// would renormalise, change phase, rebase, meet a Z = 0 step or escape raises needs_exact, and the block is replayed by step().
// IEEE double in source order (-ffp-contract=off), fp64 denormals kept; ldexp = v_ldexp_f64, the exponent = v_frexp_exp_i32_f64.
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
__device__ __forceinline__ uint32_t hi_word(double x) { return (uint32_t)((uint64_t)__double_as_longlong(x) >> 32); }

struct StateDeep {
    using Args = PerturbDeepArgs;
    static constexpr int kBlock = 8;        // the escape-time block length U: the fast block prefetches this many orbit entries
    static constexpr bool kEscapeCBeforeLoop = false;   // as StatePerturb: c needs a load of Z_1
    const double2* __restrict__ Z;
    uint32_t L;
    int32_t E;
    bool zeros;                             // the table holds Z_j = 0 for some 1 <= j < L (uniform)
    double ux, uy;                          // the pixel's offset is u * 2^E
    double wx, wy, dx, dy, zmx, zmy;        // delta = w * 2^S;  d = ldexp(w, S) (delta as a double);  zm = Z[m]
    int32_t S;
    uint32_t m;
    bool scaled;
    __device__ __forceinline__ void init(uint32_t gx, uint32_t gy, const PerturbDeepArgs& a) {
        Z = a.t.orbit;
        L = a.t.L;
        E = a.exp2;
        zeros = a.has_zero != 0u;
        ux = a.t.table[gx];
        uy = a.t.table[a.t.W + gy];
        wx = wy = dx = dy = zmx = zmy = 0.0;
        S = E;                               // the start: delta = 0 in the scaled phase at exponent E
        m = 0;
        scaled = true;
    }
    // Exact iteration (the loop of include/mc_compute.h).  As StatePerturb: escaped lanes keep iterating, the load index is clamped.
    __device__ __forceinline__ bool step() {
        m = m + 1u;
        const double2 z1 = Z[m < L ? m : L];
        double nwx, nwy;
        int32_t nS = S;
        if (scaled && zmx == 0.0 && zmy == 0.0) {                       // Z_m = 0: a fresh exponent
            nS = max(S + S, E);
            const double px = pow2((S + S) - nS), pu = pow2(E - nS);
            nwx = (((wx * wx) - (wy * wy)) * px) + (ux * pu);
            nwy = (((wx * wy) + (wy * wx)) * px) + (uy * pu);
        } else {
            const double pu = pow2(E - S);
            const double ax = (zmx + zmx) + dx, ay = (zmy + zmy) + dy;
            nwx = ((ax * wx) - (ay * wy)) + (ux * pu);
            nwy = ((ax * wy) + (ay * wx)) + (uy * pu);
        }
        const double ndx = ldexp2(nwx, nS), ndy = ldexp2(nwy, nS);
        const double zx = z1.x + ndx, zy = z1.y + ndy;
        const double r = (zx * zx) + (zy * zy);
        if (m == L || r < ((ndx * ndx) + (ndy * ndy))) {                 // rebase: Z_0 = 0, delta = z
            m = 0;
            zmx = zmy = 0.0;
            dx = zx; dy = zy;
            const double a = fmax(fabs(zx), fabs(zy));
            if (a >= kT) { scaled = false; S = 0; wx = zx; wy = zy; }
            else {
                scaled = true;
                S = a == 0.0 ? E : frexp_exp(a);                         // exactly 0: restart as at the start
                wx = ldexp2(zx, -S); wy = ldexp2(zy, -S);
            }
        } else {
            zmx = z1.x; zmy = z1.y;
            wx = nwx; wy = nwy; dx = ndx; dy = ndy; S = nS;
            if (scaled) {
                if (fmax(fabs(ndx), fabs(ndy)) >= kT) { scaled = false; S = 0; wx = ndx; wy = ndy; }
                else {
                    const double a = fmax(fabs(nwx), fabs(nwy));
                    if (a > kWinHi || a < kWinLo) {
                        const int32_t e = frexp_exp(a);
                        wx = ldexp2(nwx, -e); wy = ldexp2(nwy, -e);
                        S = nS + e;
                    }
                }
            }
        }
        return r > 2.0;
    }
    // MC_MANDEL_COLOUR_SMOOTH: the z the last step() tested (as StatePerturb: d after a rebase, else Z[m] + d, step()'s own addition);
    // c = Z_1 + ldexp(u, E).
    __device__ __forceinline__ void escape_z(double& x, double& y) const {
        x = m == 0u ? dx : zmx + dx;
        y = m == 0u ? dy : zmy + dy;
    }
    __device__ __forceinline__ void escape_c(double& x, double& y) const {
        const double2 z1 = Z[1];
        x = z1.x + ldexp2(ux, E);
        y = z1.y + ldexp2(uy, E);
    }
    // Fast block: the general formula with S fixed, u * 2^(E - S) formed once per block, Z[m+1 .. m+U] fetched at the block's start.
    // needs_exact = the escape filter of F64 / PERTURB, OR a rebase or m reaching L, OR (scaled lanes) a Z = 0 step ahead (m = 0, or
    // a table with zeros), a renormalisation or a phase change somewhere in the block.  The last three are tested on the high words
    // of max(|w'|) and min(|w'|) over the block: a superset of the exact tests (raising it needlessly only costs a replay).
    static constexpr bool kHasFastBlock = true;
    static constexpr uint32_t kCycleCheckBlocks = 0;   // no cycle exit: the state includes m (as StatePerturb)
    struct Acc {
        uint32_t hi;        // OR of the high words of |z|^2
        uint32_t whi, wlo;  // max / min over the block of the high word of |w'|inf
        bool exact;         // rebase, m == L, or a scaled lane at a Z = 0 step
        bool scaled;
        int32_t S;
        double cux, cuy;    // u * 2^(E - S)
        double2 z[kBlock];  // Z[m+1 ..], consumed one per iteration
    };
    __device__ __forceinline__ Acc acc_init() const {
        Acc acc;
        acc.hi = 0u;
        acc.whi = 0u;
        acc.wlo = 0x7ff00000u;
        acc.exact = (L - m <= (uint32_t)kBlock) || (scaled && (m == 0u || zeros));
        acc.scaled = scaled;
        acc.S = S;
        const double pu = pow2(E - S);
        acc.cux = ux * pu;
        acc.cuy = uy * pu;
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            const uint32_t j = m + 1u + (uint32_t)k;
            acc.z[k] = Z[j < L ? j : L];
        }
        return acc;
    }
    __device__ __forceinline__ void advance_fast(Acc& acc) {
        const double2 z1 = acc.z[0];
#pragma unroll
        for (int k = 0; k + 1 < kBlock; k++) acc.z[k] = acc.z[k + 1];
        const double ax = (zmx + zmx) + dx, ay = (zmy + zmy) + dy;
        const double nwx = ((ax * wx) - (ay * wy)) + acc.cux;
        const double nwy = ((ax * wy) + (ay * wx)) + acc.cuy;
        const double ndx = ldexp2(nwx, S), ndy = ldexp2(nwy, S);
        const double zx = z1.x + ndx, zy = z1.y + ndy;
        const double r = (zx * zx) + (zy * zy);
        acc.hi |= hi_word(r);
        acc.exact |= r < ((ndx * ndx) + (ndy * ndy));
        const uint32_t wh = hi_word(fmax(fabs(nwx), fabs(nwy)));
        acc.whi = max(acc.whi, wh);
        acc.wlo = min(acc.wlo, wh);
        wx = nwx; wy = nwy; dx = ndx; dy = ndy; zmx = z1.x; zmy = z1.y;
        m = m + 1u;
    }
    static __device__ __forceinline__ bool needs_exact(const Acc& acc) {
        if (acc.hi > 0x3fffffffu || acc.exact) return true;
        if (!acc.scaled) return false;
        // |w'|inf < 2^(whi's exponent + 1) =: a: a phase change needs ldexp(a, S) > T; a renormalisation needs |w'| > 2^256
        // (high word >= 0x4ff00000) or < 2^-256 (high word < 0x2ff00000)
        const double above = __longlong_as_double((long long)(((uint64_t)((acc.whi & 0x7ff00000u) + 0x00100000u)) << 32));
        return acc.whi >= 0x4ff00000u || acc.wlo < 0x2ff00000u || ldexp2(above, acc.S) >= kT;
    }
    // every word the state iterates on, by bit pattern, with S, m and the phase (mandel_block_audit.h)
    __device__ __forceinline__ bool bits_equal(const StateDeep& o) const {
        return Z == o.Z && L == o.L && E == o.E && zeros == o.zeros && S == o.S && m == o.m && scaled == o.scaled &&
               same_bits(ux, o.ux) && same_bits(uy, o.uy) && same_bits(wx, o.wx) && same_bits(wy, o.wy) && same_bits(dx, o.dx) &&
               same_bits(dy, o.dy) && same_bits(zmx, o.zmx) && same_bits(zmy, o.zmy);
    }
};

}  // namespace

int perturb_deep_launch(const PerturbDeepArgs& a, dim3 grid, hipStream_t s, const SampleList* list, SmoothOut smooth,
                        const SmoothSampleList* slist) {
    return launch_state<StateDeep>(a, grid, s, list, smooth, slist);
}

int perturb_deep_block_audit_launch(const PerturbDeepArgs& a, dim3 grid, bool sabotage, uint32_t* d_out, hipStream_t s) {
    return launch_block_audit<StateDeep, true>(a, grid, s, sabotage, d_out);
}

}  // namespace mc
