// The reference orbit's multi-limb arithmetic in lane-parallel form: one iteration of host_loop (mandel_orbit.cpp)
// as six phases over 1024 lanes.  The same source runs as the threads of one workgroup on the device (mandel_orbit_device.hip, a barrier
// after each phase) and as lane loops on the host (lanes 0 .. 1023 in order, phase by phase), so a CPU build can be stepped and tested
// without a GPU.  Pure integer arithmetic up to the final (double)mant * 2^e, which is exact: the results equal FixOps bit for bit.
//
//  * a number: sign and magnitude, H = 2 (k + 1) half-limbs of 32 bits, least significant first (a Fix limb is two of them).
//  * a product: every lane sums whole columns of 32 x 32 -> 64 partial products, column c together with column c + H (c + 1 and H - 1 - c
//    terms: H per lane), each into 96 bits; the three words of a column land on three neighbouring positions, which gives one digit below
//    2^34 per position, the rounding bit 2^(64k - 1) added to its own; one carry resolution then yields the 2H half-limbs, of which the
//    H from position 2k on are the rounded product (nothing is truncated before the carries are known).
//  * a signed sum: V and -V at once in two's complement over H + 1 positions (a term is its half-limbs or their complement, plus one per
//    complemented term at position 0); whichever has a clear top bit is the magnitude, and V = 0 picks +0 as FixOps does.
//  * carry resolution (resolve_p1 / resolve_p2): digits below 2^34 -> t = low 32 bits + the neighbour's high bits, below 2^32 + 4, so each
//    position generates (t >= 2^32) or propagates (t = 2^32 - 1) a carry of one, never both; the two masks go to one 64-bit word per 64
//    positions (a wave's ballot), and carry-in of every position = (A + B + cin) ^ A ^ B with A = G | P, B = G, chained over the words.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MC_ORBIT_HD __host__ __device__ inline
#else
#define MC_ORBIT_HD inline
#endif

namespace mc {
namespace orbitfix {

constexpr int kMaxFrac = 130;                   // fractional limbs (FixOps)
constexpr int kMaxHalf = 2 * (kMaxFrac + 1);    // 262 half-limbs
constexpr int kHalfPad = 264;
constexpr int kLanes = 1024;                    // the workgroup: four waves per SIMD of one CU, which hide the LDS latency of the columns
constexpr int kSums = 5, kProds = 3;
constexpr int kWords = 27;                      // ballot words: 3 products x ceil(524 / 64) (the sums: 5 x ceil(263 / 64) = 25)
constexpr int kDigits = 64 * kWords;

enum { kNegZx = 0, kNegZy = 1, kNegPr = 2, kNegCx = 3, kNegCy = 4 };
enum { kRunning = 0, kEscaped = 1, kTiny = 2 };  // the status word: running / escaped, j = L / tiny entry Z_(j+1)

// One orbit's working set: LDS on the device, the heap on the host.
struct Mem {
    int k, H;
    uint32_t zx[kHalfPad], zy[kHalfPad], sx[kHalfPad], sy[kHalfPad], pr[kHalfPad], cx[kHalfPad], cy[kHalfPad];   // pr = zx zy, rounded
    uint32_t neg[8];
    uint32_t status, j;
    uint32_t w[kProds][3][2 * kHalfPad];   // product columns: the three 32-bit words of each
    uint32_t R[kSums][kHalfPad];           // the sums: V_x, -V_x, V_y, -V_y, sx + sy
    uint32_t tl[kDigits];                  // low words between the two resolve phases
    unsigned long long G[kWords], P[kWords];
    int top[2];                            // highest set bit of zx, zy (-1: zero)
    uint32_t sticky[2], efrac;
};

MC_ORBIT_HD uint32_t term(const uint32_t* a, int H, int h, bool neg) {
    const uint32_t v = h < H ? a[h] : 0u;
    return neg ? ~v : v;
}

// Digit h of sum `inst` (H + 1 positions).  0 / 1: +-(sx - sy + cx); 2 / 3: +-(pr + pr + cy); 4: sx + sy.
MC_ORBIT_HD uint64_t sum_digit(const Mem& m, int inst, int h) {
    const int H = m.H;
    if (inst == 4) return (uint64_t)term(m.sx, H, h, false) + term(m.sy, H, h, false);
    const bool flip = (inst & 1) != 0;
    const bool x = inst < 2;
    const uint32_t* a0 = x ? m.sx : m.pr;
    const uint32_t* a1 = x ? m.sy : m.pr;
    const uint32_t* a2 = x ? m.cx : m.cy;
    const bool n0 = (x ? false : m.neg[kNegPr] != 0) != flip;
    const bool n1 = (x ? true : m.neg[kNegPr] != 0) != flip;
    const bool n2 = (m.neg[x ? kNegCx : kNegCy] != 0) != flip;
    uint64_t d = (uint64_t)term(a0, H, h, n0) + term(a1, H, h, n1) + term(a2, H, h, n2);
    if (h == 0) d += (uint64_t)n0 + (uint64_t)n1 + (uint64_t)n2;
    return d;
}

// Digit h of product `inst` (2H positions): the low word of column h, the middle word of column h - 1, the high word of column h - 2,
// and the first dropped bit's weight at position 2k - 1.
MC_ORBIT_HD uint64_t prod_digit(const Mem& m, int inst, int h) {
    uint64_t d = m.w[inst][0][h];
    if (h >= 1) d += m.w[inst][1][h - 1];
    if (h >= 2) d += m.w[inst][2][h - 2];
    if (h == 2 * m.k - 1) d += 0x80000000u;
    return d;
}

MC_ORBIT_HD void put_bits(Mem& m, int pos, bool g, bool p) {
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long gm = __ballot(g), pm = __ballot(p);   // pos >> 6 is uniform over the wave
    if ((pos & 63) == 0) { m.G[pos >> 6] = gm; m.P[pos >> 6] = pm; }
#else
    if ((pos & 63) == 0) { m.G[pos >> 6] = 0; m.P[pos >> 6] = 0; }   // lane 0 of a word comes first in the host's lane loop
    m.G[pos >> 6] |= (unsigned long long)g << (pos & 63);
    m.P[pos >> 6] |= (unsigned long long)p << (pos & 63);
#endif
}

template <bool PROD>
MC_ORBIT_HD void resolve_p1(Mem& m, int lane, int ninst) {
    const int N = PROD ? 2 * m.H : m.H + 1;
    const int span = ((N + 63) >> 6) << 6;
    for (int base = 0; base < ninst * span; base += kLanes) {
        const int pos = base + lane;
        if (pos >= ninst * span) continue;   // whole waves: span is a multiple of 64
        const int inst = pos / span, h = pos - inst * span;
        bool g = false, p = false;
        if (h < N) {
            const uint64_t d = PROD ? prod_digit(m, inst, h) : sum_digit(m, inst, h);
            const uint64_t c = h > 0 ? (PROD ? prod_digit(m, inst, h - 1) : sum_digit(m, inst, h - 1)) >> 32 : 0u;
            const uint64_t t = (d & 0xffffffffu) + c;
            m.tl[pos] = (uint32_t)t;
            g = (t >> 32) != 0;
            p = (uint32_t)t == 0xffffffffu;
        }
        put_bits(m, pos, g, p);
    }
}

MC_ORBIT_HD void note_top(Mem& m, int which, int bit) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax(&m.top[which], bit);
#else
    if (bit > m.top[which]) m.top[which] = bit;
#endif
}

template <bool PROD>
MC_ORBIT_HD void resolve_p2(Mem& m, int lane, int ninst) {
    const int N = PROD ? 2 * m.H : m.H + 1;
    const int W = (N + 63) >> 6, span = W << 6;
    for (int base = 0; base < ninst * span; base += kLanes) {
        const int pos = base + lane;
        if (pos >= ninst * span) continue;
        const int inst = pos / span, h = pos - inst * span;
        if (h >= N) continue;
        const int w = pos >> 6;
        unsigned long long cin = 0, carries = 0;
        for (int ww = inst * W; ww <= w; ww++) {
            const unsigned long long A = m.G[ww] | m.P[ww], B = m.G[ww];
            const unsigned long long s = A + B, s2 = s + cin;
            if (ww == w) carries = s2 ^ A ^ B;
            cin = (unsigned long long)(s < A) | (unsigned long long)(s2 < s);
        }
        const uint32_t v = m.tl[pos] + (uint32_t)((carries >> (pos & 63)) & 1u);
        if (PROD) {
            uint32_t* dst = inst == 0 ? m.pr : inst == 1 ? m.sx : m.sy;
            if (h >= 2 * m.k && h < 2 * m.k + m.H) dst[h - 2 * m.k] = v;
        } else {
            m.R[inst][h] = v;
            if (inst == 4 && h < 2 * m.k && v) m.efrac = 1u;
        }
    }
}

MC_ORBIT_HD bool any_lane(bool pred) {   // over the wave on the device; the host's lane loop takes each lane's own answer (same sums)
#if defined(__HIP_DEVICE_COMPILE__)
    return __any(pred) != 0;
#else
    return pred;
#endif
}

// The three products of the new Z: zx zy -> pr, zx^2 -> sx, zy^2 -> sy.  One unit = column c and column c + H of one product: the lane
// walks i = 0 .. H - 1 once, multiplying a[i] by b[(c - i) mod H]; the terms up to i = c are column c, which is set aside when the index
// wraps, the rest column c + H.  Blocks of 8 steps: a block in which no lane of the wave wraps runs without the per-step tests (24 of 33
// blocks at H = 262).  The numbers are zero from H up to the next multiple of 8, so the last block needs no bound on i.
MC_ORBIT_HD void prod_columns(Mem& m, int lane, int nprod) {
    const int H = m.H, Hp = (H + 7) & ~7;
    for (int u0 = 0; u0 < nprod * H; u0 += kLanes) {   // whole waves take every trip (any_lane)
        const int u = u0 + lane;
        const bool live = u < nprod * H;
        const int inst = live ? u / H : 0, c = live ? u - inst * H : 0;
        const uint32_t* a = inst == 2 ? m.zy : m.zx;
        const uint32_t* b = inst == 1 ? m.zx : m.zy;
        uint64_t lo = 0, slo = 0;
        uint32_t hi = 0, shi = 0;
        for (int i0 = 0; i0 < Hp; i0 += 8) {
            const int w = c + 1 - i0;   // the wrap falls in this block if 0 <= w < 8
            if (any_lane((w >= 0 && w < 8) || i0 + 8 > H)) {
#pragma unroll
                for (int t = 0; t < 8; t++) {
                    const int i = i0 + t;
                    if (i == c + 1) { slo = lo; shi = hi; lo = 0; hi = 0; }
                    int idx = c - i;
                    if (idx < 0) idx += H;
                    if (idx < 0) idx = 0;   // i >= H: a[i] = 0
                    const uint64_t p = (uint64_t)a[i] * b[idx];
                    lo += p;
                    hi += lo < p;
                }
            } else {
                const uint32_t* bb = b + (w > 0 ? c - i0 : c - i0 + H);   // all 8 terms on one side of the wrap: indices bb[0] down to bb[-7]
#pragma unroll
                for (int t = 0; t < 8; t++) {
                    const uint64_t p = (uint64_t)a[i0 + t] * bb[-t];
                    lo += p;
                    hi += lo < p;
                }
            }
        }
        if (c + 1 >= Hp) { slo = lo; shi = hi; lo = 0; hi = 0; }   // the last column of an unpadded number never wrapped
        if (live) {
            m.w[inst][0][c] = (uint32_t)slo; m.w[inst][1][c] = (uint32_t)(slo >> 32); m.w[inst][2][c] = shi;
            m.w[inst][0][c + H] = (uint32_t)lo; m.w[inst][1][c + H] = (uint32_t)(lo >> 32); m.w[inst][2][c + H] = hi;
        }
    }
}

// FixOps::to_double's rounding position from the highest set bit.
MC_ORBIT_HD int round_shift(int k, int top) {
    const int F = 64 * k;
    int shift = top - 52;
    if (shift < F - 1074) shift = F - 1074;
    return shift;
}

// The lane's share of top-bit search and sticky bit of number `which` (zx, zy).
MC_ORBIT_HD void top_scan(Mem& m, int which, int lane) {
    const uint32_t* a = which ? m.zy : m.zx;
    for (int h = lane; h < m.H; h += kLanes)
        if (a[h]) note_top(m, which, 32 * h + 31 - __builtin_clz(a[h]));
}
MC_ORBIT_HD void sticky_scan(Mem& m, int which, int lane) {
    const int top = m.top[which];
    if (top < 0) return;
    const int pos = round_shift(m.k, top) - 1;   // any bit below pos
    const uint32_t* a = which ? m.zy : m.zx;
    for (int h = lane; h < m.H && 32 * h < pos; h += kLanes) {
        const int in = pos - 32 * h;
        const uint32_t mask = in >= 32 ? 0xffffffffu : ((1u << in) - 1u);
        if (a[h] & mask) m.sticky[which] = 1u;
    }
}

// bits [lo, lo + cnt) of the magnitude, cnt <= 64, lo >= 0
MC_ORBIT_HD uint64_t bits_at(const uint32_t* a, int H, int lo, int cnt) {
    if (cnt <= 0) return 0;
    const int q = lo >> 5, r = lo & 31;
    const uint64_t w0 = q < H ? a[q] : 0u, w1 = q + 1 < H ? a[q + 1] : 0u, w2 = q + 2 < H ? a[q + 2] : 0u;
    const uint64_t lo64 = w0 | (w1 << 32);
    const uint64_t v = r ? (lo64 >> r) | (w2 << (64 - r)) : lo64;
    return cnt >= 64 ? v : v & ((1ull << cnt) - 1ull);
}

// 2^e for e in [-1074, 1023]
MC_ORBIT_HD double pow2(int e) {
    const uint64_t u = e >= -1022 ? (uint64_t)(e + 1023) << 52 : 1ull << (e + 1074);
    return __builtin_bit_cast(double, u);
}

// FixOps::to_double from the top bit and the sticky bit.  mant < 2^53 + 1 and mant * 2^(shift - F) is a double by construction (the
// shift is clamped at the subnormal quantum), so the one floating-point multiplication is exact; shift - F lies in [-1074, 11].
MC_ORBIT_HD double to_double(const uint32_t* a, int k, int top, bool sticky, bool neg) {
    if (top < 0) return 0.0;
    const int H = 2 * (k + 1), F = 64 * k;
    int shift = round_shift(k, top);
    uint64_t mant;
    if (shift <= 0) {
        mant = bits_at(a, H, 0, top + 1);
        shift = 0;
    } else {
        mant = bits_at(a, H, shift, top - shift + 1);
        const bool half = bits_at(a, H, shift - 1, 1) != 0;
        if (half && (sticky || (mant & 1u))) mant++;
    }
    const double v = (double)mant * pow2(shift - F);
    return neg ? -v : v;
}

// ---- one iteration: phases 0 .. 5, a barrier after each --------------------------------------------------------------------------
// State on entry: Z_j in (zx, zy), its products (sx, sy, pr), whose escape test is still open (it rides on this iteration's sums).
//   0  digits of the five sums, first resolve phase; the flags of this iteration cleared
//   1  second resolve phase
//   2  escape test of Z_j on sx + sy (then nothing else happens); Z_(j+1) selected from +-V, top bits
//   3  sticky bits; product columns of Z_(j+1)
//   4  lane 0: the two doubles, the tiny-entry test, the table entry, j + 1; all: first resolve phase of the products
//   5  second resolve phase: sx, sy, pr of Z_(j+1)
constexpr int kPhases = 6;

MC_ORBIT_HD bool escaped(const Mem& m) {   // FixOps::above_two on the exact sum (valid after phase 1)
    const uint64_t ip = (uint64_t)m.R[4][2 * m.k] | ((uint64_t)m.R[4][2 * m.k + 1] << 32);
    return ip > 2u || (ip == 2u && m.efrac != 0u);
}

// out: the table slice of this launch, (re, im) per entry; j0: the j its first entry belongs to (entry Z_(j+1) at out[2 (j - j0)]).
MC_ORBIT_HD void orbit_phase(Mem& m, int phase, int lane, bool deep, double* out, uint32_t j0) {
    const int H = m.H;
    switch (phase) {
        case 0:
            if (lane == 0) { m.top[0] = m.top[1] = -1; m.sticky[0] = m.sticky[1] = 0u; m.efrac = 0u; }
            resolve_p1<false>(m, lane, kSums);
            break;
        case 1:
            resolve_p2<false>(m, lane, kSums);
            break;
        case 2: {
            if (escaped(m)) {
                if (lane == 0) m.status = kEscaped;
                break;
            }
            const bool xneg = (m.R[0][H] >> 31) != 0, yneg = (m.R[2][H] >> 31) != 0;
            const uint32_t* srcx = m.R[xneg ? 1 : 0];
            const uint32_t* srcy = m.R[yneg ? 3 : 2];
            for (int h = lane; h < H; h += kLanes) {
                const uint32_t vx = srcx[h], vy = srcy[h];
                m.zx[h] = vx;
                m.zy[h] = vy;
                if (vx) note_top(m, 0, 32 * h + 31 - __builtin_clz(vx));
                if (vy) note_top(m, 1, 32 * h + 31 - __builtin_clz(vy));
            }
            if (lane == 0) { m.neg[kNegZx] = xneg; m.neg[kNegZy] = yneg; m.neg[kNegPr] = xneg != yneg; }
            break;
        }
        case 3:
            sticky_scan(m, 0, lane);
            sticky_scan(m, 1, lane);
            prod_columns(m, lane, kProds);
            break;
        case 4:
            if (lane == 0) {
                const double dx = to_double(m.zx, m.k, m.top[0], m.sticky[0] != 0u, m.neg[kNegZx] != 0u);
                const double dy = to_double(m.zy, m.k, m.top[1], m.sticky[1] != 0u, m.neg[kNegZy] != 0u);
                const double tiny = pow2(-960);
                if (deep && __builtin_fabs(dx) < tiny && __builtin_fabs(dy) < tiny && !(m.top[0] < 0 && m.top[1] < 0)) {
                    m.status = kTiny;
                } else {
                    out[2 * (size_t)(m.j - j0)] = dx;
                    out[2 * (size_t)(m.j - j0) + 1] = dy;
                    m.j = m.j + 1u;
                }
            }
            resolve_p1<true>(m, lane, kProds);
            break;
        default:
            resolve_p2<true>(m, lane, kProds);
            break;
    }
}

// The rounded product alone, for the tests: a in zx, b in zy, the result in pr.  Three phases.
MC_ORBIT_HD void mul_phase(Mem& m, int phase, int lane) {
    if (phase == 0) prod_columns(m, lane, 1);
    else if (phase == 1) resolve_p1<true>(m, lane, 1);
    else resolve_p2<true>(m, lane, 1);
}

}  // namespace orbitfix
}  // namespace mc
