// Path-tracer denoiser: first-hit guide planes and an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) guided by them
// (include/mc_compute.h states the contract, at mc_pathtrace_guides / mc_pathtrace_denoise; tests/pt_denoise_ref.py
// restates it in numpy).
//
// One body for the host and the device; nothing of HIP is needed to include this file (tools/pt_denoise_host_check.cpp compiles it with g++).
// pt_guides_kernel / pt_denoise_pass_kernel (pt_denoise.hip) and mc_pathtrace_guides / mc_pathtrace_denoise run these same functions.
// Every operation below is ONE IEEE-754 fp32 operation (+, -, *, /, sqrt correctly rounded; fma only where written as fma), in the order
// written, so the host, the device and the numpy restatement agree bit for bit.  Requires -ffp-contract=off.
//
// THE CONTRACT, guides (per pixel (gx, gy) of a W x H image; pathTracer.comp:352-362 with the sub-sample bracket replaced by 1.0):
//   cam_o = (0, 0.52, 7.4);  cam_d = normalize((0, -0.06, -1));  cx = normalize(cross(cam_d, |cam_d.y| < 0.9 ? (0,1,0) : (0,0,1)));
//   cy = cross(cx, cam_d);  lc = cam_o + cam_d * 0.035                                  (camera(): once per image, on the host)
//   sx = (((float)gx + 0.5) / (float)W - 0.5) * 0.036;   sy = (((float)gy + 0.5) / (float)H - 0.5) * 0.024
//   spos = (cam_o + cx * sx) + cy * sy;   d = normalize(lc - spos);   the ray is (lc, d)
//   with  dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z,  normalize(a) = a * (1 / sqrt(dot(a, a))),  cross as GLSL's.
//   intersect (pathTracer.comp:112-131, 316-341, the fp32 sphere test): t = 1e20, id = -1; planes i = 0 .. n_planes-1 in order:
//     denom = dot(d, n);  if (denom > 1e-7) { dd = (w - dot(o, n)) / denom;  if (dd < t) { t = dd; id = i; } }
//   then spheres i = 0 .. n_spheres-1 in order:  oc = c - o;  b = dot(oc, d);  det = (b*b - dot(oc, oc)) + r*r;  if (!(det < 0)) {
//     sq = sqrt(det);  dd = b - sq;  if (dd <= 1e-4) { dd = b + sq;  if (dd <= 1e-4) dd = 1e20; }  if (dd < t) { t = dd; id = n_planes + i; } }
//   a hit is t < 1e20.  x = o + d * t;  n = the plane's xyz, or normalize(x - c) for a sphere;  nl = dot(n, d) < 0 ? n : -n.
//   normal_t = (nl, t), position_id = (x, (float)id); a miss writes (0, 0, 0, 1e20) and (0, 0, 0, -1).
//   Both planes are in STORAGE order: pixel (gx, gy) is element (H - 1 - gy) * W + gx (pathTracer.comp:349).
//
// THE CONTRACT, filter (P passes, pass i = 0 .. P-1 with step s = 2^i, from the previous pass's plane into the next; storage coordinates):
//   kc_i = (float)4^i / (sigma_colour * sigma_colour)                                    (colour_weight(): per pass, on the host)
//   pixel p = (x, y) with id_p = position_id[p].w:  id_p < 0: out[p] = in[p], all four components.  Otherwise, with
//   sw = sr = sg = sb = 0 and the 25 taps in row-major order (b = -2 .. 2 outer, a = -2 .. 2 inner), q = (x + s*a, y + s*b):
//     skip q outside the image; skip q with id_q != id_p (compared as floats);
//     dc2 = (dr*dr + dg*dg) + db*db  with  (dr, dg, db) = in[q].rgb - in[p].rgb;
//     dn2 the same of normal_t[q].xyz - normal_t[p].xyz;  dx2 the same of position_id[q].xyz - position_id[p].xyz;
//     e = (dc2 * kc_i + dn2 * k_normal) + dx2 * k_position;   w = (h[b] * h[a]) * exp2(-e),  h = {1/16, 1/4, 3/8, 1/4, 1/16};
//     sw = sw + w;  sr = sr + w * in[q].r;  sg, sb likewise.
//   out[p].rgb = (sr, sg, sb) / sw (three divisions);  out[p].w = in[p].w.  The centre tap has e = 0 and w = 9/64: sw > 0.
//   exp2 is exp2_strict below: the library's strict mc_exp2 (mc_math.h) restated operation for operation, so that mc_math.h and with it
//   the path tracer's build id stay as they are.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MC_PTD_FN __host__ __device__ inline
#define MC_PTD_UNROLL _Pragma("unroll")
#else
#define MC_PTD_FN inline
#define MC_PTD_UNROLL
#endif

namespace mc {
namespace ptd {

struct alignas(16) vec4 {
    float x, y, z, w;
};
struct f3 {
    float x, y, z;
};

MC_PTD_FN f3 add(f3 a, f3 b) { return f3{a.x + b.x, a.y + b.y, a.z + b.z}; }
MC_PTD_FN f3 sub(f3 a, f3 b) { return f3{a.x - b.x, a.y - b.y, a.z - b.z}; }
MC_PTD_FN f3 muls(f3 a, float s) { return f3{a.x * s, a.y * s, a.z * s}; }
MC_PTD_FN f3 neg(f3 a) { return f3{-a.x, -a.y, -a.z}; }
MC_PTD_FN float dot(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
MC_PTD_FN f3 cross(f3 a, f3 b) { return f3{a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }
MC_PTD_FN f3 normalize(f3 a) { return muls(a, 1.0f / __builtin_sqrtf(dot(a, a))); }

constexpr float kEps = 1e-4f, kTriEps = 1e-7f, kInf = 1e20f;   // pathTracer.comp:103-105

// mc_math.h's strict mc_exp2, operation for operation.
MC_PTD_FN float exp2_strict(float y) {
    if (!(y >= -125.0f)) return 0.0f;
    if (y > 127.0f) return __builtin_inff();
    const float n = __builtin_rintf(y);
    const float f = y - n;
    float p = __builtin_fmaf(1.535336188319500e-4f, f, 1.339887440266574e-3f);
    p = __builtin_fmaf(p, f, 9.618437357674640e-3f);
    p = __builtin_fmaf(p, f, 5.550357105498874e-2f);
    p = __builtin_fmaf(p, f, 2.402264791363012e-1f);
    p = __builtin_fmaf(p, f, 6.931472028550421e-1f);
    p = __builtin_fmaf(p, f, 1.0f);
    const int e = (int)n + 127;
    return p * __builtin_bit_cast(float, (uint32_t)e << 23);
}

// ---- guides ---------------------------------------------------------------------------------------------------
struct Camera {
    f3 o, cx, cy, lc;
};
inline Camera camera() {
    Camera c;
    c.o = f3{0.0f, 0.52f, 7.4f};
    const f3 d = normalize(f3{0.0f, -0.06f, -1.0f});
    const f3 up = (__builtin_fabsf(d.y) < 0.9f) ? f3{0.0f, 1.0f, 0.0f} : f3{0.0f, 0.0f, 1.0f};
    c.cx = normalize(cross(d, up));
    c.cy = cross(c.cx, d);
    c.lc = add(c.o, muls(d, 0.035f));
    return c;
}

// A pixel's guides in three parts, so that a caller with another intersect() (pt_bvh_guides.h: the sphere BVH) shares the ray and the tail:
// the centre ray of pixel (gx, gy) ...
MC_PTD_FN void guide_ray(const Camera& cam, uint32_t W, uint32_t H, uint32_t gx, uint32_t gy, f3& o, f3& d) {
    const float sx = (((float)gx + 0.5f) / (float)W - 0.5f) * 0.036f;
    const float sy = (((float)gy + 0.5f) / (float)H - 0.5f) * 0.024f;
    const f3 spos = add(add(cam.o, muls(cam.cx, sx)), muls(cam.cy, sy));
    o = cam.lc;
    d = normalize(sub(cam.lc, spos));
}

// ... intersect() over the records rec (12 floats each: n_planes planes, then n_spheres spheres), every object in table order ...
MC_PTD_FN void guide_intersect_linear(f3 o, f3 d, const float* rec, uint32_t n_planes, uint32_t n_spheres, float& t, int32_t& id) {
    t = kInf;
    id = -1;   // (the entry points refuse more than 2^20 objects)
    for (uint32_t i = 0; i < n_planes; i++) {
        const float* pl = rec + 12 * (size_t)i;
        const f3 n{pl[0], pl[1], pl[2]};
        const float denom = dot(d, n);
        if (denom > kTriEps) {
            const float dd = (pl[3] - dot(o, n)) / denom;
            if (dd < t) { t = dd; id = (int32_t)i; }
        }
    }
    for (uint32_t i = 0; i < n_spheres; i++) {
        const float* sp = rec + 12 * ((size_t)n_planes + i);
        const f3 oc = sub(f3{sp[0], sp[1], sp[2]}, o);
        const float b = dot(oc, d);
        const float det = (b * b - dot(oc, oc)) + sp[3] * sp[3];
        if (!(det < 0.0f)) {
            const float sq = __builtin_sqrtf(det);
            float dd = b - sq;
            if (dd <= kEps) {
                dd = b + sq;
                if (dd <= kEps) dd = kInf;
            }
            if (dd < t) { t = dd; id = (int32_t)(n_planes + i); }
        }
    }
}

// ... and the two vec4s of the first hit (id, t): a miss is !(t < 1e20); rec[12 * id + 0 .. 2] is the plane's normal or the sphere's centre.
MC_PTD_FN void guide_tail(f3 o, f3 d, float t, int32_t id, const float* rec, uint32_t n_planes, vec4& normal_t, vec4& position_id) {
    if (!(t < kInf)) {
        normal_t = vec4{0.0f, 0.0f, 0.0f, kInf};
        position_id = vec4{0.0f, 0.0f, 0.0f, -1.0f};
        return;
    }
    const float* obj = rec + 12 * (size_t)id;
    const f3 x = add(o, muls(d, t));
    const f3 geo{obj[0], obj[1], obj[2]};
    const f3 n = id >= (int32_t)n_planes ? normalize(sub(x, geo)) : geo;
    const f3 nl = dot(n, d) < 0.0f ? n : neg(n);
    normal_t = vec4{nl.x, nl.y, nl.z, t};
    position_id = vec4{x.x, x.y, x.z, (float)id};
}

// The centre ray of pixel (gx, gy) against the records rec (12 floats each: n_planes planes, then n_spheres spheres).
MC_PTD_FN void guide_pixel(const Camera& cam, uint32_t W, uint32_t H, uint32_t gx, uint32_t gy, const float* rec, uint32_t n_planes,
                           uint32_t n_spheres, vec4& normal_t, vec4& position_id) {
    f3 o, d;
    guide_ray(cam, W, H, gx, gy, o, d);
    float t;
    int32_t id;
    guide_intersect_linear(o, d, rec, n_planes, n_spheres, t, id);
    guide_tail(o, d, t, id, rec, n_planes, normal_t, position_id);
}

inline void guides_host(uint32_t W, uint32_t H, const float* rec, uint32_t n_planes, uint32_t n_spheres, vec4* normal_t, vec4* position_id) {
    const Camera cam = camera();
    for (uint32_t gy = 0; gy < H; gy++)
        for (uint32_t gx = 0; gx < W; gx++) {
            const size_t gid = (size_t)(H - 1u - gy) * W + gx;
            guide_pixel(cam, W, H, gx, gy, rec, n_planes, n_spheres, normal_t[gid], position_id[gid]);
        }
}

// ---- filter ---------------------------------------------------------------------------------------------------
constexpr uint32_t kMaxPasses = 8;

inline float colour_weight(uint32_t pass, float sigma_colour) { return (float)(1u << (2u * pass)) / (sigma_colour * sigma_colour); }

MC_PTD_FN float dist2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// One pixel of one pass: the centre's colour cp, normal np and position / id pp are the caller's (held in registers by the kernel).
MC_PTD_FN vec4 filter_pixel(uint32_t W, uint32_t H, uint32_t x, uint32_t y, uint32_t step, float kc, float kn, float kx, const vec4* rgba,
                            const vec4* normal_t, const vec4* position_id, vec4 cp, vec4 np, vec4 pp) {
    if (pp.w < 0.0f) return cp;
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
MC_PTD_UNROLL
    for (int b = -2; b <= 2; b++) {
        const int64_t qy = (int64_t)y + (int64_t)step * b;
        if (qy < 0 || qy >= (int64_t)H) continue;
MC_PTD_UNROLL
        for (int a = -2; a <= 2; a++) {
            const int64_t qx = (int64_t)x + (int64_t)step * a;
            if (qx < 0 || qx >= (int64_t)W) continue;
            const size_t q = (size_t)qy * W + (size_t)qx;
            const vec4 pq = position_id[q];
            if (pq.w != pp.w) continue;
            const vec4 cq = rgba[q];
            const vec4 nq = normal_t[q];
            const float dc2 = dist2(cq.x, cq.y, cq.z, cp.x, cp.y, cp.z);
            const float dn2 = dist2(nq.x, nq.y, nq.z, np.x, np.y, np.z);
            const float dx2 = dist2(pq.x, pq.y, pq.z, pp.x, pp.y, pp.z);
            const float e = (dc2 * kc + dn2 * kn) + dx2 * kx;
            const float w = (h[b + 2] * h[a + 2]) * exp2_strict(-e);
            sw = sw + w;
            sr = sr + w * cq.x;
            sg = sg + w * cq.y;
            sb = sb + w * cq.z;
        }
    }
    return vec4{sr / sw, sg / sw, sb / sw, cp.w};
}

inline void filter_pass_host(uint32_t W, uint32_t H, uint32_t step, float kc, float kn, float kx, const vec4* in, const vec4* normal_t,
                             const vec4* position_id, vec4* out) {
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++) {
            const size_t p = (size_t)y * W + x;
            out[p] = filter_pixel(W, H, x, y, step, kc, kn, kx, in, normal_t, position_id, in[p], normal_t[p], position_id[p]);
        }
}

// The whole filter on the host: out may be rgba itself.  passes in 1 .. kMaxPasses.
inline void denoise_host(uint32_t W, uint32_t H, uint32_t passes, float sigma_colour, float kn, float kx, const vec4* rgba, const vec4* normal_t,
                         const vec4* position_id, vec4* out) {
    const size_t npix = (size_t)W * H;
    std::vector<vec4> tmp[2];
    const vec4* src = rgba;
    for (uint32_t i = 0; i < passes; i++) {
        std::vector<vec4>& dst = tmp[i & 1u];
        dst.resize(npix);
        filter_pass_host(W, H, 1u << i, colour_weight(i, sigma_colour), kn, kx, src, normal_t, position_id, dst.data());
        src = dst.data();
    }
    for (size_t p = 0; p < npix; p++) out[p] = src[p];
}

}  // namespace ptd
}  // namespace mc
