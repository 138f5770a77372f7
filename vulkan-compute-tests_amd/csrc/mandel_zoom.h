// Mandelbrot zoom sequences: a frame composed from the two keyframes that bracket it (include/mc_compute.h states the contract, at
// mc_mandelbrot_zoom_compose; tests/mandel_zoom_ref.py restates it).
//
// One body for the host and the device.  A frame whose scale is r times the wide keyframe's (r in [0.5, 1]) reads, per output pixel, the
// deep keyframe (half the wide one's scale, same centre) where the pixel falls inside it and the wide one elsewhere, through one bilinear
// tap: pure geometry in pixel units, so no precision and no colouring appears here.  axis() is one output coordinate's share of the work
// (position, source test, taps and weight for both keyframes): the kernel computes it once per row and once per lane, compose_host once
// per row and once per column.  mandel_zoom_kernel (mandel_zoom.hip) and mc_mandelbrot_zoom_compose run these same functions.
// Requires -ffp-contract=off.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MC_ZOOM_FN __host__ __device__ inline
#else
#define MC_ZOOM_FN inline
#endif

namespace mc {
namespace zoom {

// One axis of a bilinear tap: the two texel indices and the weight of the second.
struct Tap {
    uint32_t i0, i1;
    float f;
};
// One output coordinate (a column or a row): its tap in the wide keyframe, its tap in the deep one, and whether it lies inside the deep one.
struct Axis {
    Tap wide, deep;
    bool in_deep;
};

// The position of output coordinate g (of n) in a keyframe whose scale is 1 / ratio of the frame's, in that keyframe's pixels.
MC_ZOOM_FN double position(uint32_t g, uint32_t n, double ratio) { return (((double)g - 0.5 * (double)n) * ratio) + 0.5 * (double)n; }

// The tap at position X of an axis of n texels.  (For n >= 2 the clamp of i0 never acts: X is in [0, n - 1].)
MC_ZOOM_FN Tap tap_at(double X, uint32_t n) {
    int64_t i = (int64_t)__builtin_floor(X);
    const int64_t last = (int64_t)n - 1;
    i = i < 0 ? 0 : (i > last ? last : i);
    Tap t;
    t.i0 = (uint32_t)i;
    t.i1 = (uint32_t)(i + 1 < last ? i + 1 : last);
    t.f = (float)(X - (double)i);
    return t;
}

MC_ZOOM_FN Axis axis(uint32_t g, uint32_t n, double r, bool have_deep) {
    Axis a;
    a.wide = tap_at(position(g, n, r), n);
    const double r2 = r + r;
    const double X2 = position(g, n, r2);
    a.in_deep = have_deep && X2 >= 0.0 && X2 <= (double)(n - 1u);
    a.deep = a.in_deep ? tap_at(X2, n) : a.wide;
    return a;
}

// The bilinear value of the four taps a_yx (vec4 each), per component in fp32; alpha is 1.  A weight of exactly 0 takes the first tap as
// it is: a + ((b - a) * 0) would turn a -0.0f (the distance shading writes them) into +0.0f, and the contract's identities are bit for bit.
MC_ZOOM_FN float mix(float a, float b, float f) { return f == 0.0f ? a : a + ((b - a) * f); }
MC_ZOOM_FN void bilinear(const float* a00, const float* a01, const float* a10, const float* a11, float fx, float fy, float out[4]) {
    for (int c = 0; c < 3; c++) {
        const float top = mix(a00[c], a01[c], fx);
        const float bot = mix(a10[c], a11[c], fx);
        out[c] = mix(top, bot, fy);
    }
    out[3] = 1.0f;
}

// mc_convert_rgba8's conversion with scale 255 and no rotation (postprocess.hip): truncation toward zero, the low byte kept, 0 for a value
// outside int32 or NaN, alpha 255.
MC_ZOOM_FN uint32_t byte_of(float v) {
    const bool in_range = (v > -2147483648.0f) && (v < 2147483648.0f);
    const int32_t i = in_range ? (int32_t)v : (int32_t)0x80000000;
    return (uint32_t)i & 0xffu;
}
MC_ZOOM_FN uint32_t rgba8_of(const float v[4]) {
    return byte_of(255.0f * v[0]) | (byte_of(255.0f * v[1]) << 8) | (byte_of(255.0f * v[2]) << 16) | 0xff000000u;
}

// ---- the area filter of the minified deep keyframe (include/mc_compute.h, at mc_mandelbrot_zoom_compose_filtered) ----
// A deep-sourced pixel's footprint in the deep keyframe is a box of width r2 = 2 r in [1, 2] centred at its position; the filtered value is
// the box's overlap with the texel cells [k - 0.5, k + 0.5], at most three per axis, the border replicated.  A box of width 1 is the
// bilinear tap, so a wide-sourced pixel (magnified) keeps bilinear().
struct Box {
    uint32_t i[3];   // the three texel indices, clamped to the axis
    float w[3];      // their overlaps with the box, >= 0; at least one is above 0
};

// The box [X2 - r2 / 2, X2 + r2 / 2] on an axis of n texels.  k0 is the cell that holds the box's lower end (a lower end exactly on a cell
// boundary belongs to the cell above it): floor(a) and floor(a) + 0.5 are exact, so the choice is.
MC_ZOOM_FN Box box_at(double X2, double r2, uint32_t n) {
    const double h = 0.5 * r2;
    const double a = X2 - h, b = X2 + h;
    const double fl = __builtin_floor(a);
    const int64_t k0 = (int64_t)fl + (a >= fl + 0.5 ? 1 : 0);
    const int64_t last = (int64_t)n - 1;
    Box t;
    for (int j = 0; j < 3; j++) {
        const int64_t k = k0 + j;
        const double lo_cell = (double)k - 0.5, hi_cell = (double)k + 0.5;
        const double lo = a > lo_cell ? a : lo_cell;
        const double hi = b < hi_cell ? b : hi_cell;
        const double w = hi - lo;
        t.w[j] = (float)(w > 0.0 ? w : 0.0);
        t.i[j] = (uint32_t)(k < 0 ? 0 : (k > last ? last : k));
    }
    return t;
}

// One output coordinate of a filtered frame: axis()' share, and the box in the deep keyframe where the coordinate lies inside it.
struct AxisArea {
    Axis bil;
    Box box;
};
MC_ZOOM_FN AxisArea axis_area(uint32_t g, uint32_t n, double r, bool have_deep) {
    AxisArea a;
    a.bil = axis(g, n, r, have_deep);
    const double r2 = r + r;
    a.box = box_at(a.bil.in_deep ? position(g, n, r2) : 0.0, r2, n);
    return a;
}

// The box's value of the nine taps a[kStride * (3 * y + x)] (rgb each, held in registers), per component in fp32: the taps in row-major
// order, a tap whose weight wy * wx is exactly 0 skipped (0 * inf would be NaN, and -0.0f + 0.0f would lose the sign: the identities
// are bit for bit), the first tap kept initialises both sums; v = acc / sw, correctly rounded; alpha is 1.
template <int kStride>
MC_ZOOM_FN void area(const float* a, const float wx[3], const float wy[3], float out[4]) {
    float acc[3] = {0.0f, 0.0f, 0.0f}, sw = 0.0f;
    bool first = true;
    for (int y = 0; y < 3; y++)
        for (int x = 0; x < 3; x++) {
            const float p = wy[y] * wx[x];
            if (p == 0.0f) continue;
            const float* t = a + kStride * (3 * y + x);
            for (int c = 0; c < 3; c++) {
                const float m = p * t[c];
                acc[c] = first ? m : acc[c] + m;
            }
            sw = first ? p : sw + p;
            first = false;
        }
    for (int c = 0; c < 3; c++) out[c] = acc[c] / sw;
    out[3] = 1.0f;
}

// One output pixel of a filtered frame from vec4 keyframes (W texels per row).
MC_ZOOM_FN void pixel_area(const AxisArea& ax, const AxisArea& ay, uint32_t W, const float* wide, const float* deep, float v[4]) {
    if (ax.bil.in_deep && ay.bil.in_deep) {
        float a[9][3];   // (every tap is loaded, its weight 0 or not: the indices are clamped, and the loads are in flight together)
        for (int y = 0; y < 3; y++)
            for (int x = 0; x < 3; x++) {
                const float* t = deep + ((size_t)ay.box.i[y] * W + ax.box.i[x]) * 4;
                for (int c = 0; c < 3; c++) a[3 * y + x][c] = t[c];
            }
        area<3>(&a[0][0], ax.box.w, ay.box.w, v);
    } else {
        const Tap tx = ax.bil.wide, ty = ay.bil.wide;
        const float* row0 = wide + (size_t)ty.i0 * W * 4;
        const float* row1 = wide + (size_t)ty.i1 * W * 4;
        bilinear(row0 + (size_t)tx.i0 * 4, row0 + (size_t)tx.i1 * 4, row1 + (size_t)tx.i0 * 4, row1 + (size_t)tx.i1 * 4, tx.f, ty.f, v);
    }
}

inline void compose_area_host(uint32_t W, uint32_t H, const float* wide, const float* deep, double r, float* out_f32, uint8_t* out_u8) {
    const bool have_deep = deep != nullptr;
    for (uint32_t gy = 0; gy < H; gy++) {
        const AxisArea ay = axis_area(gy, H, r, have_deep);
        for (uint32_t gx = 0; gx < W; gx++) {
            const AxisArea ax = axis_area(gx, W, r, have_deep);
            float v[4];
            pixel_area(ax, ay, W, wide, deep, v);
            const size_t o = (size_t)gy * W + gx;
            if (out_f32)
                for (int c = 0; c < 4; c++) out_f32[4 * o + c] = v[c];
            if (out_u8) {
                const uint32_t b = rgba8_of(v);
                for (int c = 0; c < 4; c++) out_u8[4 * o + c] = (uint8_t)(b >> (8 * c));
            }
        }
    }
}

// The whole frame on the host: wide and deep (or null) are W x H vec4, out_f32 (W x H vec4) and out_u8 (W x H x 4 bytes) may each be null.
inline void compose_host(uint32_t W, uint32_t H, const float* wide, const float* deep, double r, float* out_f32, uint8_t* out_u8) {
    const bool have_deep = deep != nullptr;
    for (uint32_t gy = 0; gy < H; gy++) {
        const Axis ay = axis(gy, H, r, have_deep);
        for (uint32_t gx = 0; gx < W; gx++) {
            const Axis ax = axis(gx, W, r, have_deep);
            const bool from_deep = ax.in_deep && ay.in_deep;
            const float* src = from_deep ? deep : wide;
            const Tap tx = from_deep ? ax.deep : ax.wide, ty = from_deep ? ay.deep : ay.wide;
            const float* row0 = src + (size_t)ty.i0 * W * 4;
            const float* row1 = src + (size_t)ty.i1 * W * 4;
            float v[4];
            bilinear(row0 + (size_t)tx.i0 * 4, row0 + (size_t)tx.i1 * 4, row1 + (size_t)tx.i0 * 4, row1 + (size_t)tx.i1 * 4, tx.f, ty.f, v);
            const size_t o = (size_t)gy * W + gx;
            if (out_f32)
                for (int c = 0; c < 4; c++) out_f32[4 * o + c] = v[c];
            if (out_u8) {
                const uint32_t b = rgba8_of(v);
                for (int c = 0; c < 4; c++) out_u8[4 * o + c] = (uint8_t)(b >> (8 * c));
            }
        }
    }
}

}  // namespace zoom
}  // namespace mc
