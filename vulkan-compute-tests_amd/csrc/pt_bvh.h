// Path tracer: a bounding-volume hierarchy over a scene's spheres, and intersect() through it (include/mc_compute.h states the
// contract, at mc_pathtrace_accel; tests/pt_bvh_ref.py restates the linear loop in numpy).
//
// One body for the host and the device; nothing of HIP is needed to include this file (tools/pt_bvh_host_check.cpp compiles it with
// g++).  pt_bvh_kernel.h (the kernels) and mc_pathtrace_accel_intersect (pt_bvh_host.cpp) run intersect_bvh below.
// Requires -ffp-contract=off.
//
// WHAT IS COMPUTED.  intersect() of pathTracer.comp:112-131, 316-341 with the fp32 sphere test (pathtrace_kernel.h, intersect()):
//   t = 1e20, id = -1; planes i = 0 .. np-1 in order:  denom = dot(d, n);  if (denom > 1e-7) { dd = (w - dot(o, n)) / denom;
//     if (dd < t) { t = dd; id = i; } }
//   spheres i = 0 .. ns-1 in order:  oc = c - o;  b = dot(oc, d);  det = (b*b - dot(oc, oc)) + r*r;  if (!(det < 0)) { sq = sqrt(det);
//     dd = b - sq;  if (dd <= 1e-4) { dd = b + sq;  if (dd <= 1e-4) dd = 1e20; }  if (dd < t) { t = dd; id = np + i; } }
//   a hit is t < 1e20.
// A sphere's dd depends on the ray and that sphere alone, so the loop returns the smallest dd, ties going to the lowest id (planes before
// spheres).  A traversal that tests a SUBSET of the spheres in ANY order returns the same (id, t), bit for bit, when it
//   (1) accepts a candidate if  dd < t  or  (dd == t and its id is lower than the holder's), and
//   (2) never leaves out a sphere the loop would have accepted given the t it holds at that moment.
// (1) is accept() below.  (2) is the cull, proved next.
//
// THE STRUCTURE (built on the host, pt_bvh_host.cpp; deterministic: the same tables give the same bytes).
//   planes       stay a linear list, tested first, in table order: they are unbounded.
//   unboxed      spheres whose fp32 box cannot be formed — a centre or radius that is not finite, a box edge that overflows — stay a second
//                linear list tested for every ray, in table order.  Such scenes stay bit-identical instead of being refused.
//   boxed        every other sphere: box = [c - |r|, c + |r|] per axis, each edge rounded OUTWARD by one ulp, so the box contains the ball.
//   nodes        a binary tree over the boxed spheres in DEPTH-FIRST order: median split of the centres along the widest axis of their
//                bounds (ties by table index), leaves of at most 4 spheres, depth at most 19 for 2^20.  A node is 32 B:
//                (lo.xyz, skip) (hi.xyz, leaf):  skip = the node that follows this node's subtree (n_nodes ends the walk), leaf = 0 for an
//                inner node, whose first child is the next node, else (first << 3) | count into the leaf arrays.
//   leaf arrays  (c.xyz, r) and the table index of each boxed sphere in leaf order, table order within a leaf.
// The walk needs no stack:  node = pass(node) ? (leaf ? skip : node + 1) : skip.
//
// THE CULL AND ITS PROOF.  u = 2^-24.  Let the fp32 test of a sphere (c, r) accept a root for the ray (o, d): dd finite, dd > 1e-4.
// Claim: the point P = o + dd * d (real arithmetic) satisfies
//        |P - c| <= |r| + eta * Lambda,   Lambda = |c - o| + |r|,   eta = sqrt(28 u + 1.28 delta) + 16 u,   delta = | |d|^2 - 1 | <= 0.01.
// Proof.  v = fl(c - o) componentwise (|v - (c - o)| <= u |c - o|), B = v.d, Q = |v|^2, D = |d|^2 = 1 + delta', all real.  The code forms
//   b = fl(dot(v, d)):        |b - B| <= 3.03 u |v| |d|                          (three products, two sums)
//   q = fl(dot(v, v)) = Q (1 + th), |th| <= 3.03 u;   r2 = r^2 (1 + e);   det = ((b^2 (1 + e) - q)(1 + e) + r2)(1 + e), each |e| <= u,
//   so det = b^2 - Q + r^2 + E1 with |E1| <= 1.01 u (3 b^2 + 5 Q + 2 r^2).  sq = sqrt(det)(1 + e), tau0 = b -+ sq, dd = tau0 (1 + e1).
//   (tau0 - b)^2 = det (1 + e2), |e2| <= 2.01 u, hence  h := tau0^2 - 2 tau0 b + Q - r^2 = E1 + e2 det,  |h| <= 1.01 u (5 b^2 + 7 Q + 4 r^2).
//   The squared distance of P from c' = o + v, less r^2, is  g = dd^2 D - 2 dd B + Q - r^2, and
//   g - h = tau0^2 delta' + 2 e1 tau0^2 (1 + delta') + 2 tau0 (b - B) - 2 e1 tau0 B          (second-order terms in the 1.01 factors).
//   Magnitudes, with |d| <= 1.005 and Lam = |v| + |r|:  |b| <= 1.006 |v|;  sq^2 <= 1.001 (b^2 - Q + r^2) + ... <= 0.013 Q + 1.001 r^2, so
//   |tau0| <= 1.13 Lam, tau0^2 <= 1.28 Lam^2, 5 b^2 + 7 Q + 4 r^2 <= 12.1 Lam^2.  Together
//   |g| <= u Lam^2 (12.2 + 2.6 + 6.9 + 2.3) + 1.28 delta Lam^2 = (24 u + 1.28 delta) Lam^2 =: kappa Lam^2.
//   |P - c'|^2 <= r^2 + kappa Lam^2 gives |P - c'| <= |r| + sqrt(kappa) Lam; c' is within u |c - o| of c and Lam <= (1 + u) Lambda.   QED
// Overflow: an infinite b*b, dot(oc, oc) or r*r makes dd a NaN, +-inf or 1e20, none of which is ever accepted.  Underflow of a product adds at
// most 2^-146 to |g|, i.e. 2^-73 to the distance, while an accepted root has Lambda (1 + eta) >= |P - o| >= 0.99e-4: far inside the slack below.
//
// The ray's delta is MEASURED, so the domain is every ray: with D2 = fl(dot(d, d)) (|D2 - |d|^2| <= 3.1 u) and dh = |D2 - 1|,
//   eta_ray = (sqrt(2e-6 + 1.3 dh) + 1e-6) * 1.01            (2e-6 > 28 u + 1.28 * 3.1 u; the 1 % is the slack the rounding of the cull uses)
//   dh <= 0.01: the cull runs with eta_ray; otherwise — a direction that is not near unit length, a NaN — NOTHING is culled: every node
//   passes and the walk tests every sphere, as the linear loop does.  A direction normalised in fp32 (|d|^2 within 9 u of 1, dh <= 12.1 u)
//   has eta_ray = 1.73e-3 < 2^-9; 2^-9 holds up to | |d|^2 - 1 | <= 2^-20.  (Sampled: 6.1e-4 over 32 M near-tangent rays.)
// Per node, with m_a = max(|lo_a - o_a|, |hi_a - o_a|) and L = m_x + m_y + m_z:  every sphere of the node has its centre in the box, so
// |c - o| <= sqrt(m.m), and |r| <= min m_a (the box holds [c_a - |r|, c_a + |r|]); sqrt(x^2 + y^2 + z^2) + z <= x + y + z for z = min, so
// Lambda <= L.  P therefore lies in the node's box grown by pad = eta_ray * L on every side, at ray parameter dd: with [tn, tf] the ray's
// parameter interval inside the grown box, tn <= dd <= tf.  The node is skipped only if tn > tf, tf < 0 or tn > t — then every dd the node
// could yield is absent or above t, which accept() refuses.  Rounding of the slab test: (lo - o) - pad and (hi - o) + pad are formed in
// that order (errors relative to L, not to |lo|), times fl(1 / d_a): a relative error of 3 u in a plane's parameter equals moving that plane by
// at most 3.5 u L, and L itself is low by at most 3 u L — together under 1e-5 of pad's 1 % slack (0.01 * 1.4e-3 L).  d_a = 0 makes both of
// an axis' parameters infinite with the same sign (outside the slab: the node is rightly skipped) or 0 * inf = NaN (on the slab's face:
// min / max drop the NaN, no constraint — right again).  An origin that is not finite makes L infinite or NaN and the node passes.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MC_BVH_FN __host__ __device__ inline
#else
#define MC_BVH_FN inline
#endif

namespace mc {
namespace bvh {

constexpr float kEps = 1e-4f, kTriEps = 1e-7f, kInf = 1e20f;   // pathTracer.comp:103-105
constexpr uint32_t kLeafSize = 4;
constexpr uint32_t kMaxObjects = 1u << 20;

struct f3 {
    float x, y, z;
};
struct alignas(16) f4 {
    float x, y, z, w;
};
// (lo.xyz, skip) (hi.xyz, leaf): two 16-byte loads
struct alignas(16) Node {
    float lo[3];
    int32_t skip;
    float hi[3];
    int32_t leaf;
};
static_assert(sizeof(Node) == 32, "a node is 32 bytes");

// What intersect_bvh reads: host pointers in mc_pathtrace_accel_intersect, device pointers in the kernels.
struct View {
    const Node* nodes;
    const f4* leaf_sphere;          // (c.xyz, r) of the boxed spheres, leaf order
    const uint32_t* leaf_index;     // their table indices
    const uint32_t* unboxed;        // table indices of the spheres tested for every ray, ascending
    const float* rec;               // 12-float records, planes then spheres (slots 0 .. 3 are read here)
    uint32_t n_nodes, n_unboxed, n_planes, n_spheres;
};

// IEEE division and square root, correctly rounded: the host's, and hipcc's default for device code.  The kernels pass the tier's own.
struct IeeeOps {
    static MC_BVH_FN float div(float a, float b) { return a / b; }
    static MC_BVH_FN float sqrt(float a) { return __builtin_sqrtf(a); }
};

MC_BVH_FN float dot(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
MC_BVH_FN float fmin2(float a, float b) { return __builtin_fminf(a, b); }
MC_BVH_FN float fmax2(float a, float b) { return __builtin_fmaxf(a, b); }

// (1) above: the candidate g with parameter dd against the holder (id, t).  id >= np: only a sphere gives way to a lower sphere.
MC_BVH_FN void accept(float dd, int32_t g, int32_t np, float& t, int32_t& id) {
    if (dd < t || (dd == t && id >= np && g < id)) { t = dd; id = g; }
}

// pathtrace_kernel.h:559-569 for one sphere (c.xyz, r): the existing operations in the existing order.
template <class Ops> MC_BVH_FN void test_sphere(f4 s, int32_t g, int32_t np, f3 o, f3 d, float& t, int32_t& id) {
    const f3 oc{s.x - o.x, s.y - o.y, s.z - o.z};                        // :317
    const float b = dot(oc, d);                                          // :318
    const float det = (b * b - dot(oc, oc)) + s.w * s.w;
    if (!(det < 0.0f)) {                                                 // :319
        const float sq = Ops::sqrt(det);
        float dd = b - sq;                                               // :322,324
        if (dd <= kEps) {                                                // :325
            dd = b + sq;                                                 // :323,326
            if (dd <= kEps) dd = kInf;                                   // :327
        }
        accept(dd, g, np, t, id);                                        // :333
    }
}

// The ray's relative inflation eta_ray (see the proof); a negative value: cull nothing.
MC_BVH_FN float ray_eta(f3 d) {
    const float dh = __builtin_fabsf(dot(d, d) - 1.0f);
    if (!(dh <= 0.01f)) return -1.0f;
    return (__builtin_sqrtf(2e-6f + 1.3f * dh) + 1e-6f) * 1.01f;
}

template <class Ops = IeeeOps> MC_BVH_FN int32_t intersect_bvh(const View& v, f3 o, f3 d, float& t_out) {
    const int32_t np = (int32_t)v.n_planes;
    float t = kInf;
    int32_t id = -1;
    for (int32_t i = 0; i < np; i++) {
        const float* pl = v.rec + 12 * (size_t)i;
        const f3 n{pl[0], pl[1], pl[2]};
        const float denom = dot(d, n);                                   // :118
        if (denom > kTriEps) {                                           // :119
            const float dd = Ops::div(pl[3] - dot(o, n), denom);         // :120
            if (dd < t) { t = dd; id = i; }                              // :121
        }
    }
    for (uint32_t k = 0; k < v.n_unboxed; k++) {
        const uint32_t i = v.unboxed[k];
        const float* sp = v.rec + 12 * ((size_t)v.n_planes + i);
        test_sphere<Ops>(f4{sp[0], sp[1], sp[2], sp[3]}, np + (int32_t)i, np, o, d, t, id);
    }
    const float eta = ray_eta(d);
    const bool cull = eta >= 0.0f;
    const f3 inv{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
    int32_t node = 0;
    const int32_t n_nodes = (int32_t)v.n_nodes;
    while (node < n_nodes) {
        const f4 n0 = reinterpret_cast<const f4*>(v.nodes)[2 * (size_t)node];
        const f4 n1 = reinterpret_cast<const f4*>(v.nodes)[2 * (size_t)node + 1];
        const int32_t skip = __builtin_bit_cast(int32_t, n0.w), leaf = __builtin_bit_cast(int32_t, n1.w);
        const float lx = n0.x - o.x, ly = n0.y - o.y, lz = n0.z - o.z;
        const float hx = n1.x - o.x, hy = n1.y - o.y, hz = n1.z - o.z;
        const float L = (fmax2(__builtin_fabsf(lx), __builtin_fabsf(hx)) + fmax2(__builtin_fabsf(ly), __builtin_fabsf(hy))) +
                        fmax2(__builtin_fabsf(lz), __builtin_fabsf(hz));
        bool pass = true;
        if (cull && L <= 3.0e38f) {   // (an origin that is not finite: L is infinite or a NaN, the node passes)
            const float pad = eta * L;
            const float ax = (lx - pad) * inv.x, bx = (hx + pad) * inv.x;
            const float ay = (ly - pad) * inv.y, by = (hy + pad) * inv.y;
            const float az = (lz - pad) * inv.z, bz = (hz + pad) * inv.z;
            const float tn = fmax2(fmax2(fmin2(ax, bx), fmin2(ay, by)), fmin2(az, bz));
            const float tf = fmin2(fmin2(fmax2(ax, bx), fmax2(ay, by)), fmax2(az, bz));
            if (tn > tf || tf < 0.0f || tn > t) pass = false;
        }
        if (pass && leaf != 0) {
            const uint32_t first = (uint32_t)leaf >> 3, count = (uint32_t)leaf & 7u;
            for (uint32_t k = 0; k < count; k++)
                test_sphere<Ops>(v.leaf_sphere[first + k], np + (int32_t)v.leaf_index[first + k], np, o, d, t, id);
        }
        node = (pass && leaf == 0) ? node + 1 : skip;
    }
    t_out = t;
    return (t < kInf) ? id : -1;                                         // :336
}

// ---- the host's object ----------------------------------------------------------------------------------------
struct Tree {
    std::vector<Node> nodes;
    std::vector<f4> leaf_sphere;
    std::vector<uint32_t> leaf_index;
    std::vector<uint32_t> unboxed;
    uint32_t depth = 0, leaves = 0;
};
// Builds the tree over the n_spheres records of `spheres` (pt_bvh_host.cpp).
void build(const float* spheres, uint32_t n_spheres, Tree& out);

}  // namespace bvh
}  // namespace mc

// mc_pathtrace_accel (include/mc_compute.h): the tables it was made from, the tree, and what the kernels read beside them.
struct mc_pathtrace_accel {
    uint32_t n_planes = 0, n_spheres = 0;
    std::vector<float> rec;            // the records as given, planes then spheres
    std::vector<float> rec_derived;    // the same with the kernels' derived slots ([7] = max colour component, [11] = floor(m + 0.5))
    std::vector<uint32_t> lights;      // indices of the emissive spheres, in order (pathTracer.comp:407)
    mc::bvh::Tree tree;
    mc::bvh::View host_view() const {
        return mc::bvh::View{tree.nodes.data(), tree.leaf_sphere.data(), tree.leaf_index.data(), tree.unboxed.data(), rec.data(),
                             (uint32_t)tree.nodes.size(), (uint32_t)tree.unboxed.size(), n_planes, n_spheres};
    }
};
