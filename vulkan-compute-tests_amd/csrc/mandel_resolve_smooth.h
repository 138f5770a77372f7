// MC_MANDEL_SUPERSAMPLE_SMOOTH: the resolve over fractional counts (include/mc_compute.h states the contract).
//
// One body for the host and the device.  A sample's colour is smooth::smooth_colour's expression (mandel_smooth.h) of its smooth count
// q, for the ranked form of q' = smooth_equalise::remap's expression of q (mandel_smooth_equalise.h); a pixel's colour is the pairwise
// tree of §3.11 over its s x s sample colours and one multiply by 1 / (s * s).  No new floating-point expression: sample_colour is
// smooth_colour written without a branch (both table entries are gathered for every sample and the interior case is a select), so that a
// lane's gathers can be in flight together.  mandel_resolve_smooth_kernel (mandel_resolve_smooth.hip), mc_mandelbrot_resolve_smooth and
// tools/mandel_resolve_smooth_host_check.cpp run these same functions.
// Requires -ffp-contract=off.
#pragma once
#include <cstddef>
#include <cstdint>

#include "mandel_smooth_equalise.h"

namespace mc {
namespace resolve_smooth {

struct Rgba { float r, g, b, a; };
struct Knot { uint32_t knot, step; };   // (qmap[j], qmap[j + 1] - qmap[j]): one entry of the pair table

MC_SMOOTH_FN Rgba add(const Rgba& x, const Rgba& y) { return Rgba{x.r + y.r, x.g + y.g, x.b + y.b, x.a + y.a}; }
MC_SMOOTH_FN Rgba scale(const Rgba& x, float k) { return Rgba{x.r * k, x.g * k, x.b * k, x.a * k}; }

// tree(a_0 .. a_{K-1}) of the contract, K a power of two: sums of adjacent pairs, level by level — the balanced binary tree.
template <int K>
MC_SMOOTH_FN Rgba tree(const Rgba* a) {
    if constexpr (K == 1) return a[0];
    else return add(tree<K / 2>(a), tree<K / 2>(a + K / 2));
}

// The colour of one sample.  q is clamped to 256 * max_iter BEFORE any index is formed (a count above it is interior), so the pair index
// stays <= max_iter - 1 and both colour indices stay <= max_iter whatever the plane holds.  pairs(j): entry j < max_iter of the pair
// table (read only when Ranked); lut(i): entry i <= max_iter of the colour table.
template <bool Ranked, class Pairs, class Lut>
MC_SMOOTH_FN Rgba sample_colour(uint32_t q, uint32_t max_iter, const Pairs& pairs, const Lut& lut) {
    const uint32_t top = 256u * max_iter;
    q = q < top ? q : top;
    if constexpr (Ranked) {
        const bool inside = q == top;
        const Knot k = pairs(inside ? max_iter - 1u : q >> 8);
        const uint32_t r = smooth_equalise::remap_pair(q, k.knot, k.step);
        q = inside ? top : r;
        q = q < top ? q : top;   // (checked knots never exceed the top: this only keeps the indices below inside the table regardless)
    }
    // smooth::smooth_colour(q), both of its cases evaluated and selected
    const bool interior = q == top;
    const uint32_t idx = q >> 8;   // max_iter when interior
    const Rgba a = lut(idx);
    const Rgba b = lut(interior ? max_iter : idx + 1u);
    const float w = (float)(q & 255u) * 0.00390625f;
    Rgba o;
    o.r = interior ? a.r : a.r + ((b.r - a.r) * w);
    o.g = interior ? a.g : a.g + ((b.g - a.g) * w);
    o.b = interior ? a.b : a.b + ((b.b - a.b) * w);
    o.a = interior ? a.a : 1.0f;
    return o;
}

// Table accessors over plain arrays: what the host call uses (the kernel reads the same entries as one aligned vector each).
struct PairsArray {
    const uint32_t* p;
    MC_SMOOTH_FN Knot operator()(uint32_t j) const { return Knot{p[2u * (size_t)j], p[2u * (size_t)j + 1u]}; }
};
struct LutArray {
    const float* p;
    MC_SMOOTH_FN Rgba operator()(uint32_t i) const {
        const float* e = p + 4u * (size_t)i;
        return Rgba{e[0], e[1], e[2], e[3]};
    }
};

// One pixel from its S x S smooth counts at q (sample row i at q + i * pitch): row sums, their tree, one multiply.
template <int S, bool Ranked, class Pairs, class Lut>
MC_SMOOTH_FN Rgba pixel_colour(const uint32_t* q, size_t pitch, uint32_t max_iter, const Pairs& pairs, const Lut& lut) {
    Rgba r[S];
    for (int i = 0; i < S; i++) {
        Rgba a[S];
        for (int j = 0; j < S; j++) a[j] = sample_colour<Ranked>(q[(size_t)i * pitch + j], max_iter, pairs, lut);
        r[i] = tree<S>(a);
    }
    return scale(tree<S>(r), 1.0f / (float)(S * S));
}

// rows x width pixels from the dense (rows * S) x (S * width) plane q into out (4 floats per pixel).  pairs: max_iter (knot, step)
// entries, or null for the unranked form; lut: (max_iter + 1) vec4.
template <int S>
inline void resolve_plane(uint32_t max_iter, uint32_t width, uint64_t rows, const uint32_t* q, const uint32_t* pairs, const float* lut,
                          float* out) {
    const size_t pitch = (size_t)S * width;
    const PairsArray pa{pairs};
    const LutArray la{lut};
    for (uint64_t y = 0; y < rows; y++)
        for (uint32_t x = 0; x < width; x++) {
            const uint32_t* first = q + (size_t)y * S * pitch + (size_t)x * S;
            const Rgba c = pairs ? pixel_colour<S, true>(first, pitch, max_iter, pa, la) : pixel_colour<S, false>(first, pitch, max_iter, pa, la);
            float* o = out + 4u * ((size_t)y * width + x);
            o[0] = c.r; o[1] = c.g; o[2] = c.b; o[3] = c.a;
        }
}

inline bool resolve_plane(uint32_t s, uint32_t max_iter, uint32_t width, uint64_t rows, const uint32_t* q, const uint32_t* pairs,
                          const float* lut, float* out) {
    if (s == 2u) resolve_plane<2>(max_iter, width, rows, q, pairs, lut, out);
    else if (s == 4u) resolve_plane<4>(max_iter, width, rows, q, pairs, lut, out);
    else if (s == 8u) resolve_plane<8>(max_iter, width, rows, q, pairs, lut, out);
    else return false;
    return true;
}

}  // namespace resolve_smooth
}  // namespace mc
