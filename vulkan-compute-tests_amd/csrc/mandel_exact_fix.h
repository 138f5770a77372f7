// Exact counts of sampled pixels (include/mc_compute.h: "exact counts"): the contract's iteration in lane-parallel form,
// one pixel per WAVE, for numbers of at most 16 limbs (H = 2n <= 32 half-limbs of 32 bits).  Like mandel_orbit_fix.h, whose number
// format, V / -V sums and generate / propagate carry scheme these are, the same source runs as the 64 threads of a one-wave block on the
// device (mandel_exact.hip, a barrier after each phase: with one wave per block it orders the wave's own LDS traffic and nothing else)
// and as lane loops on the host (lanes 0 .. 63 in order, phase by phase).  Pure integer arithmetic: the results equal FixOps bit for bit.
//
//  * a product has 2H <= 64 columns: lane c owns column c, at most H 32 x 32 -> 64 multiply-adds into 96 bits, for the three products
//    of an iteration at once (they share their operands' reads); its carry resolution is ONE ballot word per product.
//  * a signed sum has H + 1 <= 33 positions: one ballot word each.
//  * zx and zy lie in LDS with kPad zero words on either side, so that column c reads b[c - i] for every i without a bound.
// From 17 limbs on the six phases of mandel_orbit_fix.h run unchanged, one workgroup per pixel (group_* below).
#pragma once
#include "mandel_orbit_fix.h"

namespace mc {
namespace exactfix {

using orbitfix::kNegCx;
using orbitfix::kNegCy;
using orbitfix::kNegPr;
using orbitfix::kNegZx;
using orbitfix::kNegZy;

constexpr int kWaveMaxLimbs = 16;               // the structural threshold: 2H = 64 columns fill one wave
constexpr int kWaveHalf = 2 * kWaveMaxLimbs;    // 32 half-limbs at most
constexpr int kWaveLanes = 64;
constexpr int kPad = 32;                        // zero words below and above zx, zy (c - i reaches -(H - 1) and 2H - 1)
constexpr uint32_t kRunningWord = 0xffffffffu;  // a pixel's status / count word while it runs (a count is at most 2^32 - 2)

// One pixel's working set: LDS on the device, the heap on the host.
struct WaveMem {
    int n, H;
    uint32_t zx[kPad + 2 * kWaveHalf], zy[kPad + 2 * kWaveHalf];   // the number at [kPad, kPad + H)
    uint32_t sx[kWaveHalf], sy[kWaveHalf], pr[kWaveHalf], cx[kWaveHalf], cy[kWaveHalf];   // pr = zx zy, rounded
    uint32_t neg[8];
    uint32_t w[3][3][2 * kWaveHalf];   // product columns: the three 32-bit words of each
    uint32_t tl[5][kWaveLanes];        // low words between the two resolve phases
    unsigned long long G[5], P[5];
    uint32_t R[5][kWaveHalf + 4];      // the sums: V_x, -V_x, V_y, -V_y, sx + sy
    uint32_t efrac;
};

MC_ORBIT_HD uint32_t wterm(const uint32_t* a, int H, int h, bool neg) {
    const uint32_t v = h < H ? a[h] : 0u;
    return neg ? ~v : v;
}

// Digit h of sum `inst` (H + 1 positions).  0 / 1: +-(sx - sy + cx); 2 / 3: +-(pr + pr + cy); 4: sx + sy.  Below 2^34.
MC_ORBIT_HD uint64_t wave_sum_digit(const WaveMem& m, int inst, int h) {
    const int H = m.H;
    if (inst == 4) return (uint64_t)wterm(m.sx, H, h, false) + wterm(m.sy, H, h, false);
    const bool flip = (inst & 1) != 0;
    const bool x = inst < 2;
    const uint32_t* a0 = x ? m.sx : m.pr;
    const uint32_t* a1 = x ? m.sy : m.pr;
    const uint32_t* a2 = x ? m.cx : m.cy;
    const bool n0 = (x ? false : m.neg[kNegPr] != 0) != flip;
    const bool n1 = (x ? true : m.neg[kNegPr] != 0) != flip;
    const bool n2 = (m.neg[x ? kNegCx : kNegCy] != 0) != flip;
    uint64_t d = (uint64_t)wterm(a0, H, h, n0) + wterm(a1, H, h, n1) + wterm(a2, H, h, n2);
    if (h == 0) d += (uint64_t)n0 + (uint64_t)n1 + (uint64_t)n2;
    return d;
}

// Digit h of product `inst` (2H positions): the low word of column h, the middle word of column h - 1, the high word of column h - 2,
// and the first dropped bit's weight, 2^(F - 1), at position H - 3.
MC_ORBIT_HD uint64_t wave_prod_digit(const WaveMem& m, int inst, int h) {
    uint64_t d = m.w[inst][0][h];
    if (h >= 1) d += m.w[inst][1][h - 1];
    if (h >= 2) d += m.w[inst][2][h - 2];
    if (h == m.H - 3) d += 0x80000000u;
    return d;
}

// The wave's generate and propagate words of instance `inst`: every lane of the wave calls it.
MC_ORBIT_HD void wave_put_bits(WaveMem& m, int inst, int lane, bool g, bool p) {
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long gm = __ballot(g), pm = __ballot(p);
    if (lane == 0) { m.G[inst] = gm; m.P[inst] = pm; }
#else
    if (lane == 0) { m.G[inst] = 0; m.P[inst] = 0; }   // lane 0 comes first in the host's lane loop
    m.G[inst] |= (unsigned long long)g << lane;
    m.P[inst] |= (unsigned long long)p << lane;
#endif
}

// First resolve phase of instances [i0, i1): position = lane.  t = low 32 bits + the neighbour's high bits, below 2^32 + 4.
template <bool PROD>
MC_ORBIT_HD void wave_resolve_p1(WaveMem& m, int lane, int i0, int i1) {
    const int N = PROD ? 2 * m.H : m.H + 1;
    for (int inst = i0; inst < i1; inst++) {
        bool g = false, p = false;
        if (lane < N) {
            const uint64_t d = PROD ? wave_prod_digit(m, inst, lane) : wave_sum_digit(m, inst, lane);
            const uint64_t c = lane > 0 ? (PROD ? wave_prod_digit(m, inst, lane - 1) : wave_sum_digit(m, inst, lane - 1)) >> 32 : 0u;
            const uint64_t t = (d & 0xffffffffu) + c;
            m.tl[inst][lane] = (uint32_t)t;
            g = (t >> 32) != 0;
            p = (uint32_t)t == 0xffffffffu;
        }
        wave_put_bits(m, inst, lane, g, p);
    }
}

// Second resolve phase: the carry into every position from ONE 64-bit word, (A + B) ^ A ^ B with A = G | P, B = G.
template <bool PROD>
MC_ORBIT_HD void wave_resolve_p2(WaveMem& m, int lane, int i0, int i1) {
    const int H = m.H, N = PROD ? 2 * H : H + 1;
    if (lane >= N) return;
    for (int inst = i0; inst < i1; inst++) {
        const unsigned long long A = m.G[inst] | m.P[inst], B = m.G[inst];
        const unsigned long long carries = (A + B) ^ A ^ B;
        const uint32_t v = m.tl[inst][lane] + (uint32_t)((carries >> lane) & 1u);
        if (PROD) {
            uint32_t* dst = inst == 0 ? m.pr : inst == 1 ? m.sx : m.sy;
            if (lane >= H - 2 && lane < 2 * H - 2) dst[lane - (H - 2)] = v;   // positions 2(n - 1) .. 2(n - 1) + H - 1
        } else {
            m.R[inst][lane] = v;
            if (inst == 4 && lane < H - 2 && v) m.efrac = 1u;
        }
    }
}

// The three products of the new Z, column `lane` of each: zx zy -> w[0], zx^2 -> w[1], zy^2 -> w[2].
MC_ORBIT_HD void wave_prod_columns(WaveMem& m, int lane) {
    const int H = m.H;
    if (lane >= 2 * H) return;
    uint64_t lo0 = 0, lo1 = 0, lo2 = 0;
    uint32_t hi0 = 0, hi1 = 0, hi2 = 0;
    const uint32_t* bx = m.zx + kPad + lane;   // bx[-i] = zx[lane - i], zero outside the number
    const uint32_t* by = m.zy + kPad + lane;
    for (int i = 0; i < H; i++) {
        const uint64_t ax = m.zx[kPad + i], ay = m.zy[kPad + i];
        const uint64_t vx = bx[-i], vy = by[-i];
        const uint64_t p0 = ax * vy, p1 = ax * vx, p2 = ay * vy;
        lo0 += p0; hi0 += lo0 < p0;
        lo1 += p1; hi1 += lo1 < p1;
        lo2 += p2; hi2 += lo2 < p2;
    }
    m.w[0][0][lane] = (uint32_t)lo0; m.w[0][1][lane] = (uint32_t)(lo0 >> 32); m.w[0][2][lane] = hi0;
    m.w[1][0][lane] = (uint32_t)lo1; m.w[1][1][lane] = (uint32_t)(lo1 >> 32); m.w[1][2][lane] = hi1;
    m.w[2][0][lane] = (uint32_t)lo2; m.w[2][1][lane] = (uint32_t)(lo2 >> 32); m.w[2][2][lane] = hi2;
}

// ---- one iteration: phases 0 .. 7, a barrier after each --------------------------------------------------------------------------
// State on entry: z_j in (zx, zy) and its products (sx, sy, pr).  After phase 7 wave_escaped tells whether |z_(j+1)|^2 > 2.
//   0  digits of the four signed sums, first resolve phase       4  first resolve phase of the products
//   1  second resolve phase                                      5  second resolve phase: sx, sy, pr of z_(j+1)
//   2  z_(j+1) selected from +-V                                 6  sx + sy, first resolve phase
//   3  product columns of z_(j+1)                                7  second resolve phase
constexpr int kWavePhases = 8;

MC_ORBIT_HD void wave_phase(WaveMem& m, int phase, int lane) {
    const int H = m.H;
    switch (phase) {
        case 0: wave_resolve_p1<false>(m, lane, 0, 4); break;
        case 1: wave_resolve_p2<false>(m, lane, 0, 4); break;
        case 2: {
            const bool xneg = (m.R[0][H] >> 31) != 0, yneg = (m.R[2][H] >> 31) != 0;
            if (lane < H) {
                m.zx[kPad + lane] = m.R[xneg ? 1 : 0][lane];
                m.zy[kPad + lane] = m.R[yneg ? 3 : 2][lane];
            }
            if (lane == 0) { m.neg[kNegZx] = xneg; m.neg[kNegZy] = yneg; m.neg[kNegPr] = xneg != yneg; m.efrac = 0u; }
            break;
        }
        case 3: wave_prod_columns(m, lane); break;
        case 4: wave_resolve_p1<true>(m, lane, 0, 3); break;
        case 5: wave_resolve_p2<true>(m, lane, 0, 3); break;
        case 6: wave_resolve_p1<false>(m, lane, 4, 5); break;
        default: wave_resolve_p2<false>(m, lane, 4, 5); break;
    }
}

MC_ORBIT_HD bool wave_escaped(const WaveMem& m) {   // FixOps::above_two on the exact sum (valid after phase 7)
    const uint64_t ip = (uint64_t)m.R[4][m.H - 2] | ((uint64_t)m.R[4][m.H - 1] << 32);
    return ip > 2u || (ip == 2u && m.efrac != 0u);
}

// ---- the lane loops on the host (the CPU check of the shared arithmetic; no device) ------------------------------------------------
#if !defined(__HIP_DEVICE_COMPILE__)

inline void wave_init(WaveMem& m, int n, const uint64_t* cx, const uint64_t* cy, bool cx_neg, bool cy_neg) {
    m = WaveMem();
    m.n = n;
    m.H = 2 * n;
    for (int i = 0; i < n; i++) {
        m.cx[2 * i] = (uint32_t)cx[i]; m.cx[2 * i + 1] = (uint32_t)(cx[i] >> 32);
        m.cy[2 * i] = (uint32_t)cy[i]; m.cy[2 * i + 1] = (uint32_t)(cy[i] >> 32);
    }
    m.neg[kNegCx] = cx_neg;
    m.neg[kNegCy] = cy_neg;
}

// The count of one c of n <= 16 limbs by the wave kernel's phases.
inline uint32_t wave_count_lanes(int n, const uint64_t* cx, const uint64_t* cy, bool cx_neg, bool cy_neg, uint32_t max_iter) {
    WaveMem* m = new WaveMem();
    wave_init(*m, n, cx, cy, cx_neg, cy_neg);
    uint32_t j = 0;
    for (; j < max_iter; j++) {
        for (int ph = 0; ph < kWavePhases; ph++)
            for (int lane = 0; lane < kWaveLanes; lane++) wave_phase(*m, ph, lane);
        if (wave_escaped(*m)) break;
    }
    delete m;
    return j;
}

// The rounded products of the wave kernel: a b, a^2, b^2 of n-limb magnitudes (phases 3 .. 5 alone).
inline void wave_mul_lanes(int n, const uint64_t* a, const uint64_t* b, uint64_t* ab, uint64_t* aa, uint64_t* bb) {
    WaveMem* m = new WaveMem();
    wave_init(*m, n, a, b, false, false);
    for (int h = 0; h < 2 * n; h++) { m->zx[kPad + h] = m->cx[h]; m->zy[kPad + h] = m->cy[h]; }
    for (int ph = 3; ph <= 5; ph++)
        for (int lane = 0; lane < kWaveLanes; lane++) wave_phase(*m, ph, lane);
    for (int i = 0; i < n; i++) {
        ab[i] = (uint64_t)m->pr[2 * i] | ((uint64_t)m->pr[2 * i + 1] << 32);
        aa[i] = (uint64_t)m->sx[2 * i] | ((uint64_t)m->sx[2 * i + 1] << 32);
        bb[i] = (uint64_t)m->sy[2 * i] | ((uint64_t)m->sy[2 * i + 1] << 32);
    }
    delete m;
}

#endif

// ---- the workgroup kernel's iteration (n >= 17 limbs): mandel_orbit_fix.h's phases, without phase 4's lane-0 doubles ---------------
// State on entry as there: z_j and its products, whose escape test is still open.  status / j as in the orbit: escaped with j = the
// first j whose |z_j|^2 > 2, so the count is j - 1.  At j = max_iter only the escape test of z_(max_iter) is left: group_last.
MC_ORBIT_HD void group_phase(orbitfix::Mem& m, int phase, int lane) {
    if (phase == 4) {
        if (lane == 0) m.j = m.j + 1u;
        orbitfix::resolve_p1<true>(m, lane, orbitfix::kProds);
    } else {
        orbitfix::orbit_phase(m, phase, lane, false, nullptr, 0u);
    }
}

#if !defined(__HIP_DEVICE_COMPILE__)

inline void group_init(orbitfix::Mem& m, int n, const uint64_t* cx, const uint64_t* cy, bool cx_neg, bool cy_neg) {
    m = orbitfix::Mem();
    m.k = n - 1;
    m.H = 2 * n;
    for (int i = 0; i < n; i++) {
        m.cx[2 * i] = (uint32_t)cx[i]; m.cx[2 * i + 1] = (uint32_t)(cx[i] >> 32);
        m.cy[2 * i] = (uint32_t)cy[i]; m.cy[2 * i + 1] = (uint32_t)(cy[i] >> 32);
    }
    m.neg[kNegCx] = cx_neg;
    m.neg[kNegCy] = cy_neg;
}

// The count of one c of n <= 131 limbs by the workgroup kernel's phases.
inline uint32_t group_count_lanes(int n, const uint64_t* cx, const uint64_t* cy, bool cx_neg, bool cy_neg, uint32_t max_iter) {
    orbitfix::Mem* m = new orbitfix::Mem();
    group_init(*m, n, cx, cy, cx_neg, cy_neg);
    uint32_t count = max_iter;
    for (;;) {
        for (int ph = 0; ph < 2; ph++)
            for (int lane = 0; lane < orbitfix::kLanes; lane++) group_phase(*m, ph, lane);
        if (m->j == max_iter) {
            if (orbitfix::escaped(*m)) count = max_iter - 1u;
            break;
        }
        for (int lane = 0; lane < orbitfix::kLanes; lane++) group_phase(*m, 2, lane);
        if (m->status != orbitfix::kRunning) { count = m->j - 1u; break; }
        for (int ph = 3; ph < orbitfix::kPhases; ph++)
            for (int lane = 0; lane < orbitfix::kLanes; lane++) group_phase(*m, ph, lane);
    }
    delete m;
    return count;
}

#endif

}  // namespace exactfix
}  // namespace mc
