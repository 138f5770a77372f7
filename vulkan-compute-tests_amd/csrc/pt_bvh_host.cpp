// Path tracer BVH, host side: the build and the host-only entry points (mc_pathtrace_accel_create / _destroy / _info / _intersect /
// _guides).
// Plain C++17, no HIP header; built with the library's floating-point flags (-ffp-contract=off), since intersect_bvh's results are
// results.  The structure, the cull and its proof: pt_bvh.h.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <set>

#include "pt_bvh_guides.h"
#include "pt_bvh_host.h"

namespace mc {
namespace bvh {

namespace {

struct Builder {
    const std::vector<float>& lo;   // 3 per boxed candidate, by table index
    const std::vector<float>& hi;
    const float* spheres;
    std::vector<uint32_t>& idx;
    Tree& out;

    void emit(uint32_t begin, uint32_t end, uint32_t depth) {
        const uint32_t me = (uint32_t)out.nodes.size();
        out.nodes.push_back(Node{});
        out.depth = std::max(out.depth, depth);
        float blo[3], bhi[3], clo[3], chi[3];
        for (int a = 0; a < 3; a++) {
            blo[a] = clo[a] = INFINITY;
            bhi[a] = chi[a] = -INFINITY;
        }
        for (uint32_t k = begin; k < end; k++) {
            const uint32_t i = idx[k];
            for (int a = 0; a < 3; a++) {
                blo[a] = std::min(blo[a], lo[3 * (size_t)i + a]);
                bhi[a] = std::max(bhi[a], hi[3 * (size_t)i + a]);
                const float c = spheres[12 * (size_t)i + a];
                clo[a] = std::min(clo[a], c);
                chi[a] = std::max(chi[a], c);
            }
        }
        int32_t leaf = 0;
        if (end - begin <= kLeafSize) {
            std::sort(idx.begin() + begin, idx.begin() + end);   // table order within a leaf
            const uint32_t first = (uint32_t)out.leaf_sphere.size();
            for (uint32_t k = begin; k < end; k++) {
                const float* sp = spheres + 12 * (size_t)idx[k];
                out.leaf_sphere.push_back(f4{sp[0], sp[1], sp[2], sp[3]});
                out.leaf_index.push_back(idx[k]);
            }
            leaf = (int32_t)((first << 3) | (end - begin));
            out.leaves++;
        } else {
            int axis = 0;   // the widest axis of the centres' bounds, the lowest axis on a tie
            for (int a = 1; a < 3; a++)
                if (chi[a] - clo[a] > chi[axis] - clo[axis]) axis = a;
            const uint32_t mid = begin + (end - begin) / 2u;
            // (centre, table index) is a total order: the lower half is the same SET whatever the selection algorithm does inside
            std::nth_element(idx.begin() + begin, idx.begin() + mid, idx.begin() + end, [&](uint32_t x, uint32_t y) {
                const float cx = spheres[12 * (size_t)x + axis], cy = spheres[12 * (size_t)y + axis];
                return cx < cy || (cx == cy && x < y);
            });
            emit(begin, mid, depth + 1u);
            emit(mid, end, depth + 1u);
        }
        Node& n = out.nodes[me];
        for (int a = 0; a < 3; a++) { n.lo[a] = blo[a]; n.hi[a] = bhi[a]; }
        n.skip = (int32_t)out.nodes.size();
        n.leaf = leaf;
    }
};

}  // namespace

void build(const float* spheres, uint32_t n_spheres, Tree& out) {
    out = Tree{};
    std::vector<float> lo(3 * (size_t)n_spheres), hi(3 * (size_t)n_spheres);
    std::vector<uint32_t> idx;
    for (uint32_t i = 0; i < n_spheres; i++) {
        const float* sp = spheres + 12 * (size_t)i;
        const float r = std::fabs(sp[3]);
        bool ok = std::isfinite(r);
        for (int a = 0; a < 3 && ok; a++) {
            const float l = std::nextafterf(sp[a] - r, -INFINITY), h = std::nextafterf(sp[a] + r, INFINITY);   // outward: the box holds the ball
            ok = std::isfinite(sp[a]) && std::isfinite(l) && std::isfinite(h);
            lo[3 * (size_t)i + a] = l;
            hi[3 * (size_t)i + a] = h;
        }
        if (ok) idx.push_back(i);
        else out.unboxed.push_back(i);
    }
    if (idx.empty()) return;
    out.nodes.reserve(idx.size());
    out.leaf_sphere.reserve(idx.size());
    out.leaf_index.reserve(idx.size());
    Builder b{lo, hi, spheres, idx, out};
    b.emit(0u, (uint32_t)idx.size(), 1u);
}

}  // namespace bvh

namespace {

std::mutex g_mu;
std::set<const mc_pathtrace_accel*> g_live;

int refuse(const char* who, const char* what, int rc = MC_ERR_INVALID_ARGUMENT) {
    set_error_detail(std::string(who) + ": " + what);
    return rc;
}

}  // namespace

bool pt_accel_live(const mc_pathtrace_accel* a) {
    std::lock_guard<std::mutex> lock(g_mu);
    return a && g_live.count(a) != 0;
}

}  // namespace mc

extern "C" {

int mc_pathtrace_accel_create(const float* planes, uint32_t n_planes, const float* spheres, uint32_t n_spheres, mc_pathtrace_accel** out) {
    const char* who = "mc_pathtrace_accel_create";
    if (!out) return mc::refuse(who, "out is NULL");
    *out = nullptr;
    if ((!planes && n_planes) || (!spheres && n_spheres)) return mc::refuse(who, "a scene table is NULL although its count is not 0");
    if ((size_t)n_planes + n_spheres > mc::bvh::kMaxObjects) return mc::refuse(who, "more than 2^20 objects", MC_ERR_UNSUPPORTED);
    try {
        mc_pathtrace_accel* a = new mc_pathtrace_accel;
        a->n_planes = n_planes;
        a->n_spheres = n_spheres;
        a->rec.resize(12 * ((size_t)n_planes + n_spheres));
        if (n_planes) std::memcpy(a->rec.data(), planes, sizeof(float) * 12 * n_planes);
        if (n_spheres) std::memcpy(a->rec.data() + 12 * (size_t)n_planes, spheres, sizeof(float) * 12 * n_spheres);
        // the kernels' derived slots (pathtrace_kernel.h, stage_records) and the emissive list (pathTracer.comp:407): the same fp32 operations
        a->rec_derived = a->rec;
        for (size_t k = 0; k < (size_t)n_planes + n_spheres; k++) {
            float* o = a->rec_derived.data() + 12 * k;
            const float m01 = (o[8] < o[9]) ? o[9] : o[8];
            o[7] = (m01 < o[10]) ? o[10] : m01;
            o[11] = std::floor(o[11] + 0.5f);
            if (k >= n_planes && (o[4] * o[4] + o[5] * o[5]) + o[6] * o[6] > 0.0f) a->lights.push_back((uint32_t)(k - n_planes));
        }
        mc::bvh::build(a->rec.data() + 12 * (size_t)n_planes, n_spheres, a->tree);
        std::lock_guard<std::mutex> lock(mc::g_mu);
        mc::g_live.insert(a);
        *out = a;
    } catch (const std::bad_alloc&) {
        return mc::refuse(who, "out of host memory", MC_ERR_OUT_OF_MEMORY);
    }
    return MC_OK;
}

int mc_pathtrace_accel_destroy(mc_pathtrace_accel* a) {
    if (!a) return MC_OK;
    if (!mc::pt_accel_live(a)) return mc::refuse("mc_pathtrace_accel_destroy", "not a live mc_pathtrace_accel (destroyed already?)");
    mc::pt_accel_release_device(a);
    {
        std::lock_guard<std::mutex> lock(mc::g_mu);
        mc::g_live.erase(a);
    }
    delete a;
    return MC_OK;
}

int mc_pathtrace_accel_info(const mc_pathtrace_accel* a, mc_pathtrace_accel_stats* out) {
    const char* who = "mc_pathtrace_accel_info";
    if (!a || !out) return mc::refuse(who, "a NULL pointer");
    if (!mc::pt_accel_live(a)) return mc::refuse(who, "not a live mc_pathtrace_accel (destroyed already?)");
    const mc::bvh::Tree& t = a->tree;
    out->n_planes = a->n_planes;
    out->n_spheres = a->n_spheres;
    out->nodes = (uint32_t)t.nodes.size();
    out->depth = t.depth;
    out->leaves = t.leaves;
    out->boxed = (uint32_t)t.leaf_index.size();
    out->unboxed = (uint32_t)t.unboxed.size();
    out->device_copies = mc::pt_accel_device_copies(a);
    out->bytes = (uint64_t)t.nodes.size() * sizeof(mc::bvh::Node) + (uint64_t)t.leaf_sphere.size() * 20u + (uint64_t)t.unboxed.size() * 4u;
    return MC_OK;
}

int mc_pathtrace_accel_copy(const mc_pathtrace_accel* a, void* out_bytes, uint64_t capacity) {
    const char* who = "mc_pathtrace_accel_copy";
    if (!a || !out_bytes) return mc::refuse(who, "a NULL pointer");
    if (!mc::pt_accel_live(a)) return mc::refuse(who, "not a live mc_pathtrace_accel (destroyed already?)");
    const mc::bvh::Tree& t = a->tree;
    const size_t n0 = t.nodes.size() * sizeof(mc::bvh::Node), n1 = t.leaf_sphere.size() * 16u, n2 = t.leaf_index.size() * 4u,
                 n3 = t.unboxed.size() * 4u;
    if (capacity < n0 + n1 + n2 + n3) return mc::refuse(who, "capacity is below mc_pathtrace_accel_stats.bytes");
    char* p = static_cast<char*>(out_bytes);
    if (n0) std::memcpy(p, t.nodes.data(), n0);
    if (n1) std::memcpy(p + n0, t.leaf_sphere.data(), n1);
    if (n2) std::memcpy(p + n0 + n1, t.leaf_index.data(), n2);
    if (n3) std::memcpy(p + n0 + n1 + n2, t.unboxed.data(), n3);
    return MC_OK;
}

int mc_pathtrace_accel_intersect(const mc_pathtrace_accel* a, uint64_t n_rays, const float* origins, const float* dirs, int32_t* out_id,
                                 float* out_t) {
    const char* who = "mc_pathtrace_accel_intersect";
    if (!a || !out_id || !out_t || ((!origins || !dirs) && n_rays)) return mc::refuse(who, "a NULL pointer");
    if (!mc::pt_accel_live(a)) return mc::refuse(who, "not a live mc_pathtrace_accel (destroyed already?)");
    const mc::bvh::View v = a->host_view();
    for (uint64_t k = 0; k < n_rays; k++) {
        const mc::bvh::f3 o{origins[3 * k], origins[3 * k + 1], origins[3 * k + 2]}, d{dirs[3 * k], dirs[3 * k + 1], dirs[3 * k + 2]};
        out_id[k] = mc::bvh::intersect_bvh<mc::bvh::IeeeOps>(v, o, d, out_t[k]);
    }
    return MC_OK;
}

// The guide planes of mc_pathtrace_guides for the object's tables, through the tree (pt_bvh_guides.h).
int mc_pathtrace_accel_guides(const mc_pathtrace_accel* a, uint32_t width, uint32_t height, float* out_normal_t, float* out_position_id) {
    using mc::ptd::vec4;
    const char* who = "mc_pathtrace_accel_guides";
    if (!a) return mc::refuse(who, "a NULL pointer");
    if (!mc::pt_accel_live(a)) return mc::refuse(who, "not a live mc_pathtrace_accel (destroyed already?)");
    if (!width || !height) return mc::refuse(who, "width and height must be above 0");
    if (!out_normal_t || !out_position_id) return mc::refuse(who, "an output plane is NULL");
    const size_t npix = (size_t)width * height;
    // a plane of the caller's that is not aligned to 16 bytes is written through a copy (vec4 is alignas(16))
    auto misaligned = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16u != 0u; };
    try {
        std::vector<vec4> s_nt(misaligned(out_normal_t) ? npix : 0u), s_pid(misaligned(out_position_id) ? npix : 0u);
        vec4* nt = s_nt.empty() ? reinterpret_cast<vec4*>(out_normal_t) : s_nt.data();
        vec4* pid = s_pid.empty() ? reinterpret_cast<vec4*>(out_position_id) : s_pid.data();
        mc::ptd::guides_bvh_host(width, height, a->host_view(), nt, pid);
        if (!s_nt.empty()) std::memcpy(out_normal_t, s_nt.data(), npix * 16);
        if (!s_pid.empty()) std::memcpy(out_position_id, s_pid.data(), npix * 16);
    } catch (const std::bad_alloc&) {
        return mc::refuse(who, "out of host memory", MC_ERR_OUT_OF_MEMORY);
    }
    return MC_OK;
}

}  // extern "C"
