// The histogram kernel's body and launch geometry, shared by the two planes the library histograms: a plane of integer counts
// (MC_MANDEL_COLOUR_EQUALISED, mandel_histogram.hip) and a plane of smooth counts keyed by q >> 8 (MC_MANDEL_COLOUR_SMOOTH_EQUALISED,
// mandel_smooth_equalise.hip).  The scheme — wave combining, block-private LDS tables over ranges of bins, one global add per non-zero bin
// at the flush, the global-table route for very long tables — is described at the top of mandel_histogram.hip and measured in DESIGN.md
// §3.10.  A Key maps a stored word to the value whose bin it counts in, before the clamp to max_iter:
//   KeyCount   the word itself (a count n)
//   KeySmooth  word >> 8 (a 24.8 fixed-point smooth count q: its integer part)
#pragma once
#include <algorithm>
#include <cstdint>

#include "mandel_equalise.h"

namespace mc {
namespace hist {

constexpr int kCombineRounds = 4;

struct KeyCount {
    static __device__ __forceinline__ uint32_t of(uint32_t v) { return v; }
};
struct KeySmooth {
    static __device__ __forceinline__ uint32_t of(uint32_t v) { return v >> 8; }
};

template <bool LDS>
__device__ __forceinline__ void table_add(uint32_t* tab, uint32_t bin, uint32_t count) {
    if (LDS)
        (void)__hip_atomic_fetch_add(tab + bin, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else
        (void)__hip_atomic_fetch_add(tab + bin, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One word per lane (pending == false: the lane has none), called by the whole wave.
template <bool LDS>
__device__ __forceinline__ void wave_combine_add(uint32_t* tab, uint32_t v, bool pending, uint32_t lane) {
#pragma unroll
    for (int r = 0; r < kCombineRounds; r++) {
        const unsigned long long act = __ballot(pending);
        if (!act) return;   // wave-uniform
        const uint32_t leader = (uint32_t)__ffsll((long long)act) - 1u;
        const uint32_t lv = (uint32_t)__builtin_amdgcn_readlane((int)v, (int)leader);
        const bool mine = pending && v == lv;
        const unsigned long long same = __ballot(mine);
        if (lane == leader) table_add<LDS>(tab, lv, (uint32_t)__popcll(same));
        pending = pending && !mine;
    }
    if (pending) table_add<LDS>(tab, v, 1u);
}

template <class T>
struct Words;
template <>
struct Words<uint32_t> {
    static constexpr int kPer = 4;
    static __device__ __forceinline__ uint32_t get(const uint4& q, int j) { return j == 0 ? q.x : j == 1 ? q.y : j == 2 ? q.z : q.w; }
};
template <>
struct Words<uint16_t> {
    static constexpr int kPer = 8;
    static __device__ __forceinline__ uint32_t get(const uint4& q, int j) {
        const uint32_t w = (j >> 1) == 0 ? q.x : (j >> 1) == 1 ? q.y : (j >> 1) == 2 ? q.z : q.w;
        return (j & 1) ? (w >> 16) : (w & 0xffffu);
    }
};

// head: values in front of the first 16-B boundary, nvec: whole 16-B vectors, tail: values behind them (head, tail < kPer).
// Block b owns the bins [lo, lo + bins) of range b % n_ranges and share b / n_ranges of the plane (gridDim.x is a multiple of n_ranges);
// LDS == false: one range, the global table itself.
// The kernel is a macro, not a function that two kernels inline: NAME<T, LDS> is defined where the macro is expanded (a translation unit's
// own unnamed namespace), with KEY's mapping, from ONE text — and mandel_histogram.hip's expansion is token for token the kernel that
// stood there, so its listings are what they were (a shared __device__ body, inlined, scheduled the loop differently).
// Notes on the text (a macro holds no line comments):
//  * the main loop's trip count is the same for every lane of a wave: the ballots see whole waves.  Lane 0 of a wave is active in every
//    trip (base < nvec), and inactive lanes sit above the active ones.
//  * w[j] is the key clamped to max_iter (the clamp of mandelbrot_assemble_kernel) less the range's first bin: in this block's range
//    exactly when w[j] < bins (a key below lo wraps to a large value), and nothing is added outside [0, bins).
//  * a wave whose lanes all hold one value issues one add; the plane's head and tail, fewer than 2 * kPer values, are counted one per lane
//    by the first block of every range.
#define MC_HISTOGRAM_KERNEL(NAME, KEY)                                                                                                                \
template <class T, bool LDS>                                                                                                                          \
__global__ void __launch_bounds__(256) NAME(const T* __restrict__ in, uint32_t head, uint64_t nvec, uint32_t tail, uint32_t max_iter,                 \
                                            uint32_t range_bins, uint32_t n_ranges, uint32_t* __restrict__ hist) {                                    \
    extern __shared__ uint32_t lds_tab[];                                                                                                             \
    constexpr int kPer = ::mc::hist::Words<T>::kPer;                                                                                                  \
    const uint32_t range = blockIdx.x % n_ranges, share = blockIdx.x / n_ranges, shares = gridDim.x / n_ranges;                                       \
    const uint32_t lo = range * range_bins;                                                                                                           \
    const uint32_t bins = max_iter - lo < range_bins ? max_iter - lo + 1u : range_bins;                                                               \
    uint32_t* tab = LDS ? lds_tab : hist;                                                                                                             \
    if (LDS) {                                                                                                                                        \
        for (uint32_t i = threadIdx.x; i < bins; i += 256u) lds_tab[i] = 0u;                                                                          \
        __syncthreads();                                                                                                                              \
    }                                                                                                                                                 \
    const uint32_t lane = threadIdx.x & 63u;                                                                                                          \
    const uint4* __restrict__ vec = reinterpret_cast<const uint4*>(in + head);                                                                        \
    const uint64_t stride = (uint64_t)shares * 256u;                                                                                                  \
    for (uint64_t base = (uint64_t)share * 256u + (threadIdx.x & ~63u); base < nvec; base += stride) {                                                \
        const uint64_t i = base + lane;                                                                                                               \
        const bool active = i < nvec;                                                                                                                 \
        uint4 q = make_uint4(0u, 0u, 0u, 0u);                                                                                                         \
        if (active) q = vec[i];                                                                                                                       \
        uint32_t w[kPer];                                                                                                                             \
_Pragma("unroll")                                                                                                                                     \
        for (int j = 0; j < kPer; j++) {                                                                                                              \
            const uint32_t v = KEY::of(::mc::hist::Words<T>::get(q, j));                                                                              \
            w[j] = (v > max_iter ? max_iter : v) - lo;                                                                                                \
        }                                                                                                                                             \
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)w[0]);                                                                   \
        bool flat = true;                                                                                                                             \
_Pragma("unroll")                                                                                                                                     \
        for (int j = 0; j < kPer; j++) flat = flat && w[j] == first;                                                                                  \
        const unsigned long long act = __ballot(active);                                                                                              \
        if (__ballot(active && !flat) == 0ull) {                                                                                                      \
            if (lane == 0u && first < bins) ::mc::hist::table_add<LDS>(tab, first, (uint32_t)__popcll(act) * (uint32_t)kPer);                         \
            continue;                                                                                                                                 \
        }                                                                                                                                             \
_Pragma("unroll")                                                                                                                                     \
        for (int j = 0; j < kPer; j++) ::mc::hist::wave_combine_add<LDS>(tab, w[j], active && w[j] < bins, lane);                                     \
    }                                                                                                                                                 \
    if (share == 0u && threadIdx.x < head + tail) {                                                                                                   \
        const uint64_t at = threadIdx.x < head ? (uint64_t)threadIdx.x : (uint64_t)head + nvec * kPer + (threadIdx.x - head);                         \
        uint32_t v = KEY::of((uint32_t)in[at]);                                                                                                       \
        v = (v > max_iter ? max_iter : v) - lo;                                                                                                       \
        if (v < bins) ::mc::hist::table_add<LDS>(tab, v, 1u);                                                                                         \
    }                                                                                                                                                 \
    if (LDS) {                                                                                                                                        \
        __syncthreads();                                                                                                                              \
        for (uint32_t i = threadIdx.x; i < bins; i += 256u) {                                                                                         \
            const uint32_t c = lds_tab[i];                                                                                                            \
            if (c) ::mc::hist::table_add<false>(hist, lo + i, c);                                                                                     \
        }                                                                                                                                             \
    }                                                                                                                                                 \
}

// The launch of one histogram over n_values words of word_bytes each at address addr (aligned to word_bytes), n_values > 0.
struct Geometry {
    bool lds;              // the LDS-range kernel; false: the global-table kernel
    uint32_t head, tail;   // values in front of the first 16-B boundary and behind the last whole vector
    uint64_t nvec;
    uint32_t range_bins, ranges;   // the kernel's range_bins and n_ranges arguments
    uint32_t grid;                 // blocks of 256 lanes
    size_t shared;                 // dynamic LDS bytes
};
inline Geometry geometry(uintptr_t addr, uint32_t word_bytes, uint64_t n_values, uint32_t max_iter, uint32_t cus) {
    Geometry g;
    const uint64_t all_bins = (uint64_t)max_iter + 1u;
    const uint32_t range_bins = (uint32_t)std::min<uint64_t>(all_bins, kHistRangeBins);
    const uint32_t n_ranges = (uint32_t)((all_bins + range_bins - 1u) / range_bins);
    g.lds = n_ranges <= kHistMaxRanges;
    const uint32_t per = 16u / word_bytes;
    g.head = (uint32_t)(((16u - addr % 16u) % 16u) / word_bytes);
    if (g.head > n_values) g.head = (uint32_t)n_values;
    g.nvec = (n_values - g.head) / per;
    g.tail = (uint32_t)(n_values - g.head - g.nvec * per);
    // 8 blocks of 4 waves per CU for the global table; an LDS range's size bounds the blocks a CU holds (160 KB of LDS).  Every range
    // gets the same number of blocks (its shares of the plane), at least one.
    g.shared = g.lds ? (size_t)range_bins * 4u : 0;
    const uint32_t per_cu = g.lds ? std::max<uint32_t>(1u, std::min<uint32_t>(8u, (uint32_t)((160u << 10) / g.shared))) : 8u;
    g.ranges = g.lds ? n_ranges : 1u;
    uint64_t shares = std::min<uint64_t>((g.nvec + 255u) / 256u, std::max<uint64_t>(1u, (uint64_t)cus * per_cu / g.ranges));
    if (!shares) shares = 1;
    g.grid = (uint32_t)(shares * g.ranges);
    g.range_bins = g.lds ? range_bins : (uint32_t)std::min<uint64_t>(all_bins, 0xffffffffull);
    return g;
}

}  // namespace hist
}  // namespace mc
