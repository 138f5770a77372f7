// Mandelbrot zoom sequences from COUNT keyframes: the moving map, a tap's colour and the frame (include/mc_compute.h states the contract, at
// mc_mandelbrot_zoom_compose_counts; tests/mandel_zoom_counts_ref.py restates it).
//
// One body for the host and the device.  A keyframe is a plane of uint32_t (the count n, or the smooth count q); a frame is mandel_zoom.h's
// compose, unchanged, applied to the colours of the taps: positions, source test, taps, mix and the byte conversion are that header's, the
// colours are the existing expressions (the colour table, smooth::smooth_colour, smooth_equalise::remap_pair).  Nothing here is a new
// floating-point expression.  tap_colours takes the four counts of a pixel at once: it forms every table index first, then gathers, then
// computes, so that on the device the gathers of the four taps are in flight together.  mandel_zoom_counts_kernel (mandel_zoom_counts.hip)
// and mc_mandelbrot_zoom_compose_counts run these same functions.  Requires -ffp-contract=off.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "mandel_smooth_equalise.h"
#include "mandel_zoom.h"

namespace mc {
namespace zoom_counts {

enum Mode : int { Plain = 0, Equalised = 1, Smooth = 2, SmoothEqualised = 3 };

// The largest entry blend takes: 256 * (2^24 - 1), the top knot at the largest max_iter of the smooth colourings.  Entries and weights are
// below 2^32, so a product is below 2^64; the two weights sum to S, so the sum is at most max(a, b) * S, below 2^64 as well.
constexpr uint32_t kBlendMax = 256u * 0x00ffffffu;

// One entry of the moving map: (a (S - s) + b s) / S in uint64_t, rounded down.  s <= S, S >= 1.
MC_ZOOM_FN uint32_t blend(uint32_t a, uint32_t b, uint32_t s, uint32_t S) {
    return (uint32_t)((((uint64_t)a * (uint64_t)(S - s)) + ((uint64_t)b * (uint64_t)s)) / (uint64_t)S);
}

// A smooth count as smooth::smooth_colour reads it: the two neighbouring entries of the colour table and the count's place between them,
// as a count of the two-entry table {lut[i0], lut[i1]} (256: its top, the interior).  A q at or above 256 M is the interior.
struct SmoothTap {
    uint32_t i0, i1, ql;
};
MC_ZOOM_FN SmoothTap smooth_tap(uint32_t q, uint32_t M) {
    const bool interior = q >= 256u * M;
    SmoothTap t;
    t.i0 = interior ? M : (q >> 8);
    t.i1 = interior ? M : (q >> 8) + 1u;   // (q < 256 M: at most M)
    t.ql = interior ? 256u : (q & 255u);
    return t;
}
// smooth::smooth_colour of that two-entry table: lut[i0] + ((lut[i1] - lut[i0]) * w) for an escaped count, lut[M] as it is for the interior.
MC_ZOOM_FN void smooth_tap_colour(const SmoothTap& t, const float a[3], const float b[3], float out[4]) {
    const float two[8] = {a[0], a[1], a[2], 1.0f, b[0], b[1], b[2], 1.0f};
    smooth::smooth_colour(t.ql, 1u, two, out);
}

MC_ZOOM_FN void load_rgb(const float* table, uint32_t i, float out[3]) {
    const float* e = table + 4u * (size_t)i;
    out[0] = e[0]; out[1] = e[1]; out[2] = e[2];
}

// The colours (rgb; alpha is the compose's) of a pixel's four taps.
//   Plain, Equalised   table: (M + 1) vec4, the colour table or lut[map[.]]; colour = table[min(n, M)]
//   Smooth             table: the colour table; colour = smooth_colour(q)
//   SmoothEqualised    table: the colour table; pairs: M entries (knot, step); colour = smooth_colour(remap(q))
template <int kMode>
MC_ZOOM_FN void tap_colours(const uint32_t n[4], uint32_t M, const float* table, const uint32_t* pairs, float c[4][4]) {
    if (kMode == Plain || kMode == Equalised) {
        uint32_t i[4];
        for (int k = 0; k < 4; k++) i[k] = n[k] < M ? n[k] : M;
        for (int k = 0; k < 4; k++) load_rgb(table, i[k], c[k]);
        for (int k = 0; k < 4; k++) c[k][3] = 1.0f;
        return;
    }
    uint32_t q[4];
    for (int k = 0; k < 4; k++) q[k] = n[k];
    if (kMode == SmoothEqualised) {
        const uint32_t top = 256u * M;
        uint32_t knot[4], step[4];
        for (int k = 0; k < 4; k++) {   // (an interior count reads the last pair and discards it)
            const uint32_t j = q[k] < top ? (q[k] >> 8) : M - 1u;
            knot[k] = pairs[2u * (size_t)j];
            step[k] = pairs[2u * (size_t)j + 1u];
        }
        for (int k = 0; k < 4; k++) q[k] = q[k] < top ? smooth_equalise::remap_pair(q[k], knot[k], step[k]) : top;
    }
    SmoothTap t[4];
    float a[4][3], b[4][3];
    for (int k = 0; k < 4; k++) t[k] = smooth_tap(q[k], M);
    for (int k = 0; k < 4; k++) {
        load_rgb(table, t[k].i0, a[k]);
        load_rgb(table, t[k].i1, b[k]);
    }
    for (int k = 0; k < 4; k++) smooth_tap_colour(t[k], a[k], b[k], c[k]);
}

// One output pixel: zoom::axis' geometry, the four counts, their colours, zoom::bilinear.
template <int kMode>
MC_ZOOM_FN void pixel(const zoom::Axis& ax, const zoom::Axis& ay, uint32_t W, uint32_t M, const uint32_t* wide, const uint32_t* deep,
                      const float* table, const uint32_t* pairs, float v[4]) {
    const bool from_deep = ax.in_deep && ay.in_deep;
    const uint32_t* src = from_deep ? deep : wide;
    const zoom::Tap tx = from_deep ? ax.deep : ax.wide, ty = from_deep ? ay.deep : ay.wide;
    const uint32_t* row0 = src + (size_t)ty.i0 * W;
    const uint32_t* row1 = src + (size_t)ty.i1 * W;
    const uint32_t n[4] = {row0[tx.i0], row0[tx.i1], row1[tx.i0], row1[tx.i1]};
    float c[4][4];
    tap_colours<kMode>(n, M, table, pairs, c);
    zoom::bilinear(c[0], c[1], c[2], c[3], tx.f, ty.f, v);
}

// lut[map[j]] for the rank map (entries <= M) and the pair table of the knot map: what the kernel gathers from.
inline void composed_table(uint32_t M, const float* lut, const uint32_t* map, float* table) {
    for (size_t j = 0; j <= M; j++)
        for (int c = 0; c < 4; c++) table[4 * j + c] = lut[4 * (size_t)map[j] + c];
}

// The whole frame on the host.  wide, deep (or null): W x H uint32_t; lut: (M + 1) vec4; map: M + 1 entries for the two equalised
// colourings (checked by the caller), null otherwise; out_f32 (W x H vec4) and out_u8 (W x H x 4 bytes) may each be null.
template <int kMode>
inline void compose_counts_mode(uint32_t W, uint32_t H, uint32_t M, const uint32_t* wide, const uint32_t* deep, const float* table,
                                const uint32_t* pairs, double r, float* out_f32, uint8_t* out_u8) {
    const bool have_deep = deep != nullptr;
    for (uint32_t gy = 0; gy < H; gy++) {
        const zoom::Axis ay = zoom::axis(gy, H, r, have_deep);
        for (uint32_t gx = 0; gx < W; gx++) {
            const zoom::Axis ax = zoom::axis(gx, W, r, have_deep);
            float v[4];
            pixel<kMode>(ax, ay, W, M, wide, deep, table, pairs, v);
            const size_t o = (size_t)gy * W + gx;
            if (out_f32)
                for (int c = 0; c < 4; c++) out_f32[4 * o + c] = v[c];
            if (out_u8) {
                const uint32_t b = zoom::rgba8_of(v);
                for (int c = 0; c < 4; c++) out_u8[4 * o + c] = (uint8_t)(b >> (8 * c));
            }
        }
    }
}

inline void compose_counts_host(uint32_t W, uint32_t H, uint32_t M, int mode, const uint32_t* wide, const uint32_t* deep, const float* lut,
                                const uint32_t* map, double r, float* out_f32, uint8_t* out_u8) {
    switch (mode) {
        case Plain: compose_counts_mode<Plain>(W, H, M, wide, deep, lut, nullptr, r, out_f32, out_u8); break;
        case Equalised: {
            std::vector<float> table(((size_t)M + 1) * 4);
            composed_table(M, lut, map, table.data());
            compose_counts_mode<Equalised>(W, H, M, wide, deep, table.data(), nullptr, r, out_f32, out_u8);
            break;
        }
        case Smooth: compose_counts_mode<Smooth>(W, H, M, wide, deep, lut, nullptr, r, out_f32, out_u8); break;
        default: {
            std::vector<uint32_t> pairs((size_t)M * 2);
            smooth_equalise::compose_pairs(M, map, pairs.data());
            compose_counts_mode<SmoothEqualised>(W, H, M, wide, deep, lut, pairs.data(), r, out_f32, out_u8);
            break;
        }
    }
}

// ---- the area filter (include/mc_compute.h, at mc_mandelbrot_zoom_compose_filtered): zoom::area over the colours of
// the nine counts of a deep-sourced pixel's box; a wide-sourced pixel is pixel() above.  tap_colours9 is tap_colours for nine counts, the
// same expressions per tap in the same order: every index first, then the gathers, then the colours.
template <int kMode>
MC_ZOOM_FN void tap_colours9(const uint32_t n[9], uint32_t M, const float* table, const uint32_t* pairs, float c[9][4]) {
    if (kMode == Plain || kMode == Equalised) {
        uint32_t i[9];
        for (int k = 0; k < 9; k++) i[k] = n[k] < M ? n[k] : M;
        for (int k = 0; k < 9; k++) load_rgb(table, i[k], c[k]);
        for (int k = 0; k < 9; k++) c[k][3] = 1.0f;
        return;
    }
    uint32_t q[9];
    for (int k = 0; k < 9; k++) q[k] = n[k];
    if (kMode == SmoothEqualised) {
        const uint32_t top = 256u * M;
        uint32_t knot[9], step[9];
        for (int k = 0; k < 9; k++) {   // (an interior count reads the last pair and discards it)
            const uint32_t j = q[k] < top ? (q[k] >> 8) : M - 1u;
            knot[k] = pairs[2u * (size_t)j];
            step[k] = pairs[2u * (size_t)j + 1u];
        }
        for (int k = 0; k < 9; k++) q[k] = q[k] < top ? smooth_equalise::remap_pair(q[k], knot[k], step[k]) : top;
    }
    SmoothTap t[9];
    float a[9][3], b[9][3];
    for (int k = 0; k < 9; k++) t[k] = smooth_tap(q[k], M);
    for (int k = 0; k < 9; k++) {
        load_rgb(table, t[k].i0, a[k]);
        load_rgb(table, t[k].i1, b[k]);
    }
    for (int k = 0; k < 9; k++) smooth_tap_colour(t[k], a[k], b[k], c[k]);
}

template <int kMode>
MC_ZOOM_FN void pixel_area(const zoom::AxisArea& ax, const zoom::AxisArea& ay, uint32_t W, uint32_t M, const uint32_t* wide, const uint32_t* deep,
                           const float* table, const uint32_t* pairs, float v[4]) {
    if (ax.bil.in_deep && ay.bil.in_deep) {
        uint32_t n[9];
        for (int y = 0; y < 3; y++)
            for (int x = 0; x < 3; x++) n[3 * y + x] = deep[(size_t)ay.box.i[y] * W + ax.box.i[x]];
        float c[9][4];
        tap_colours9<kMode>(n, M, table, pairs, c);
        zoom::area<4>(&c[0][0], ax.box.w, ay.box.w, v);
    } else {
        zoom::Axis bx = ax.bil, by = ay.bil;   // (pixel() chooses by in_deep: this pixel reads wide)
        bx.in_deep = false;
        by.in_deep = false;
        pixel<kMode>(bx, by, W, M, wide, deep, table, pairs, v);
    }
}

template <int kMode>
inline void compose_counts_area_mode(uint32_t W, uint32_t H, uint32_t M, const uint32_t* wide, const uint32_t* deep, const float* table,
                                     const uint32_t* pairs, double r, float* out_f32, uint8_t* out_u8) {
    const bool have_deep = deep != nullptr;
    for (uint32_t gy = 0; gy < H; gy++) {
        const zoom::AxisArea ay = zoom::axis_area(gy, H, r, have_deep);
        for (uint32_t gx = 0; gx < W; gx++) {
            const zoom::AxisArea ax = zoom::axis_area(gx, W, r, have_deep);
            float v[4];
            pixel_area<kMode>(ax, ay, W, M, wide, deep, table, pairs, v);
            const size_t o = (size_t)gy * W + gx;
            if (out_f32)
                for (int c = 0; c < 4; c++) out_f32[4 * o + c] = v[c];
            if (out_u8) {
                const uint32_t b = zoom::rgba8_of(v);
                for (int c = 0; c < 4; c++) out_u8[4 * o + c] = (uint8_t)(b >> (8 * c));
            }
        }
    }
}

// compose_counts_host with MC_MANDEL_ZOOM_FILTER_AREA: the same tables, the filtered frame.
inline void compose_counts_area_host(uint32_t W, uint32_t H, uint32_t M, int mode, const uint32_t* wide, const uint32_t* deep, const float* lut,
                                     const uint32_t* map, double r, float* out_f32, uint8_t* out_u8) {
    switch (mode) {
        case Plain: compose_counts_area_mode<Plain>(W, H, M, wide, deep, lut, nullptr, r, out_f32, out_u8); break;
        case Equalised: {
            std::vector<float> table(((size_t)M + 1) * 4);
            composed_table(M, lut, map, table.data());
            compose_counts_area_mode<Equalised>(W, H, M, wide, deep, table.data(), nullptr, r, out_f32, out_u8);
            break;
        }
        case Smooth: compose_counts_area_mode<Smooth>(W, H, M, wide, deep, lut, nullptr, r, out_f32, out_u8); break;
        default: {
            std::vector<uint32_t> pairs((size_t)M * 2);
            smooth_equalise::compose_pairs(M, map, pairs.data());
            compose_counts_area_mode<SmoothEqualised>(W, H, M, wide, deep, lut, pairs.data(), r, out_f32, out_u8);
            break;
        }
    }
}

}  // namespace zoom_counts
}  // namespace mc
