// Host side of the BVH path tracer launch: the request's checks, the camera basis, the sample-parallel width, the device
// copy of an mc_pathtrace_accel per context, and the device-form entry points of the render and of the list render (§3.24; the guides
// through the tree: pt_bvh_guides.hip).  Device code: pt_bvh_kernel.h; the structure: pt_bvh.h;
// the build and the host-only entry points: pt_bvh_host.cpp; the blocking entry points: api.hip, beside the calls whose skeleton they use.
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "pt_bvh_device.h"
#include "pt_bvh_kernel.h"

namespace mc {

using pt::BvhArgs;
using pt::PTArgs;
using pt::v3;

namespace {

// camera — pathTracer.comp:352-353,360 with the shader's fp32 operations (pathtrace.hip's set_camera, restated: that file stays as it is)
inline v3 h_add(v3 a, v3 b) { return v3{a.x + b.x, a.y + b.y, a.z + b.z}; }
inline v3 h_muls(v3 a, float s) { return v3{a.x * s, a.y * s, a.z * s}; }
inline float h_dot(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
inline v3 h_cross(v3 a, v3 b) { return v3{a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }
inline v3 h_normalize(v3 a) { return h_muls(a, 1.0f / sqrtf(h_dot(a, a))); }
void set_camera(PTArgs& a) {
    a.cam_o = v3{0.0f, 0.52f, 7.4f};
    a.cam_d = h_normalize(v3{0.0f, -0.06f, -1.0f});
    v3 up = (fabsf(a.cam_d.y) < 0.9f) ? v3{0, 1, 0} : v3{0, 0, 1};
    a.cx = h_normalize(h_cross(a.cam_d, up));
    a.cy = h_cross(a.cx, a.cam_d);
    a.lc = h_add(a.cam_o, h_muls(a.cam_d, 0.035f));
}

// Sample-parallel width: the round-synchronous kernels' rule (pathtrace.hip, choose_S).
int choose_S(uint64_t pixels, uint32_t samples) {
    const uint64_t target_waves = 65536;
    if (pixels / 64 >= target_waves || samples < 4) return 1;
    if (pixels * 4 / 64 >= target_waves || samples < 16) return 4;
    return 16;
}

int refuse(const char* who, const std::string& what, int rc = MC_ERR_INVALID_ARGUMENT) {
    set_error_detail(std::string(who) + ": " + what);
    return rc;
}

struct Plan {
    int S = 1, tail_S = 0;
    uint32_t math_mode = MC_PT_MATH_STRICT;
};

int plan_request(const mc_pathtrace_accel* a, const mc_pathtrace_params* p, const char* who, Plan& plan) {
    if (!a || !p) return refuse(who, "a NULL pointer");
    if (!pt_accel_live(a)) return refuse(who, "not a live mc_pathtrace_accel (destroyed already?)");
    if (!p->width || !p->height || !p->spp || p->row_end > p->height || p->row_begin >= p->row_end || p->sample_end > p->spp ||
        p->sample_begin >= p->sample_end)
        return refuse(who, "an empty image, row range or sample range");
    if (p->math_mode != MC_PT_MATH_STRICT && p->math_mode != MC_PT_MATH_FAST && p->math_mode != MC_PT_MATH_FAST_CAREFUL)
        return refuse(who, "math_mode is not one of MC_PT_MATH_*");
    if (p->row_stride && (!p->row_block || p->row_block > p->row_stride)) return refuse(who, "row_block must be in 1 .. row_stride");
    const uint32_t prec = (p->flags >> 16) & 0xfu;   // MC_PT_PRECISION(x)
    if (prec != 0u && (p->flags & ~0xf0000u) == 0u) {
        static const char* const kNames[] = {"", "MC_PT_PREC_FP64", "MC_PT_PREC_DS", "MC_PT_PREC_DF64"};
        return refuse(who, std::string("the extended sphere test ") + (prec <= 3u ? kNames[prec] : "(unknown MC_PT_PRECISION)") +
                               " has no BVH kernel: MC_PT_PREC_F32 only", MC_ERR_UNSUPPORTED);
    }
    if (p->flags) return refuse(who, "flags must be 0");
    plan.math_mode = p->math_mode == MC_PT_MATH_STRICT ? (uint32_t)MC_PT_MATH_STRICT : (uint32_t)MC_PT_MATH_FAST_CAREFUL;
    const uint32_t row_block = p->row_stride ? p->row_block : 0u;
    const uint32_t rows = tile_rows(p->row_begin, p->row_end, row_block, p->row_stride);
    const uint32_t n_samples = p->sample_end - p->sample_begin;
    plan.S = choose_S((uint64_t)rows * p->width, n_samples);
    // a ragged sample count: the full rounds, then the rest as a continuation at a narrower width (pathtrace.hip, choose_kernel: the
    // accumulator round-trips through the buffer unchanged, so the sum and its order are the same)
    const uint32_t rest = n_samples % (uint32_t)plan.S;
    if (plan.S > 1 && rest != 0u && n_samples > (uint32_t)plan.S) plan.tail_S = rest >= 4u ? 4 : 1;
    return MC_OK;
}

// ---- device copies: one per (accel, context), made on first use -------------------------------------------------
struct DeviceCopy {
    mc_context* ctx;
    DeviceBuffer buf;
    bvh::View view;              // device pointers
    const uint32_t* d_lights;
};
std::mutex g_mu;
std::map<const mc_pathtrace_accel*, std::vector<DeviceCopy>> g_copies;

size_t align16(size_t n) { return (n + 15u) & ~(size_t)15u; }

int device_copy(mc_context* ctx, const mc_pathtrace_accel* a, hipStream_t s, DeviceCopy& out) {
    std::lock_guard<std::mutex> lock(g_mu);
    std::vector<DeviceCopy>& list = g_copies[a];
    for (const DeviceCopy& c : list)
        if (c.ctx == ctx) { out = c; return MC_OK; }
    const bvh::Tree& t = a->tree;
    const size_t n_nodes = t.nodes.size() * sizeof(bvh::Node), n_sph = t.leaf_sphere.size() * sizeof(bvh::f4),
                 n_idx = t.leaf_index.size() * 4u, n_unb = t.unboxed.size() * 4u, n_rec = a->rec_derived.size() * 4u,
                 n_lights = a->lights.size() * 4u;
    const size_t at_sph = align16(n_nodes), at_idx = at_sph + align16(n_sph), at_unb = at_idx + align16(n_idx), at_rec = at_unb + align16(n_unb),
                 at_lights = at_rec + align16(n_rec), total = at_lights + align16(n_lights) + 16u;
    std::vector<char> blob(total, 0);
    if (n_nodes) std::memcpy(blob.data(), t.nodes.data(), n_nodes);
    if (n_sph) std::memcpy(blob.data() + at_sph, t.leaf_sphere.data(), n_sph);
    if (n_idx) std::memcpy(blob.data() + at_idx, t.leaf_index.data(), n_idx);
    if (n_unb) std::memcpy(blob.data() + at_unb, t.unboxed.data(), n_unb);
    if (n_rec) std::memcpy(blob.data() + at_rec, a->rec_derived.data(), n_rec);
    if (n_lights) std::memcpy(blob.data() + at_lights, a->lights.data(), n_lights);
    DeviceCopy c{};
    c.ctx = ctx;
    if (int rc = c.buf.reserve(total)) return rc;
    hipError_t e = hipMemcpyAsync(c.buf.ptr, blob.data(), total, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // pageable source `blob` (a local): staged before this returns
    if (e != hipSuccess) {
        c.buf.release();
        set_error_detail(std::string("mc_pathtrace_accel: upload: ") + hipGetErrorString(e));
        return MC_ERR_HIP;
    }
    const char* base = static_cast<const char*>(c.buf.ptr);
    c.view = bvh::View{reinterpret_cast<const bvh::Node*>(base), reinterpret_cast<const bvh::f4*>(base + at_sph),
                       reinterpret_cast<const uint32_t*>(base + at_idx), reinterpret_cast<const uint32_t*>(base + at_unb),
                       reinterpret_cast<const float*>(base + at_rec), (uint32_t)t.nodes.size(), (uint32_t)t.unboxed.size(), a->n_planes,
                       a->n_spheres};
    c.d_lights = reinterpret_cast<const uint32_t*>(base + at_lights);
    list.push_back(c);
    out = c;
    return MC_OK;
}

// Before a copy is freed: the launches of its context that may still read it (never the whole device).
void free_copy(DeviceCopy& c) {
    (void)hipSetDevice(c.ctx->device);
    (void)c.ctx->drain_launch_streams();
    c.buf.release();
}

}  // namespace

void pt_accel_release_device(const mc_pathtrace_accel* a) {
    std::lock_guard<std::mutex> lock(g_mu);
    auto it = g_copies.find(a);
    if (it == g_copies.end()) return;
    for (DeviceCopy& c : it->second) free_copy(c);
    g_copies.erase(it);
}

uint32_t pt_accel_device_copies(const mc_pathtrace_accel* a) {
    std::lock_guard<std::mutex> lock(g_mu);
    auto it = g_copies.find(a);
    return it == g_copies.end() ? 0u : (uint32_t)it->second.size();
}

void pt_accel_release_context(mc_context* ctx) {
    std::lock_guard<std::mutex> lock(g_mu);
    for (auto& entry : g_copies) {
        std::vector<DeviceCopy>& list = entry.second;
        for (size_t k = 0; k < list.size();) {
            if (list[k].ctx == ctx) { free_copy(list[k]); list.erase(list.begin() + (long)k); }
            else k++;
        }
    }
}

int pathtrace_accel_select(const mc_pathtrace_accel* a, const mc_pathtrace_params* p, mc_pathtrace_kernel_info* out, const char* who) {
    if (!out) return refuse(who, "out is NULL");
    Plan plan;
    if (int rc = plan_request(a, p, who, plan)) return rc;
    out->kernel = MC_PT_KERNEL_BVH;
    out->lanes_per_pixel = (uint32_t)plan.S;
    out->math_mode = plan.math_mode;
    out->launches = plan.tail_S ? 2u : 1u;
    return MC_OK;
}

namespace {

// The kernels' arguments of request p on the device copy `copy` (the output plane is the caller's to set).
void fill_args(const mc_pathtrace_accel* a, const mc_pathtrace_params* p, const DeviceCopy& copy, BvhArgs& k) {
    std::memset(&k, 0, sizeof(k));
    PTArgs& args = k.a;
    args.W = p->width; args.H = p->height; args.spp = p->spp;
    args.sample_begin = p->sample_begin; args.sample_end = p->sample_end;
    args.max_depth = p->max_depth; args.row_begin = p->row_begin; args.row_end = p->row_end;
    args.row_block = p->row_stride ? p->row_block : 0u; args.row_stride = p->row_stride;
    set_camera(args);
    args.inv_W = 1.0f / (float)p->width; args.inv_H = 1.0f / (float)p->height; args.inv_spp = 1.0f / (float)p->spp;
    args.scene.n_planes = a->n_planes; args.scene.n_spheres = a->n_spheres;
    args.scene.n_emissive = (uint32_t)a->lights.size();
    args.scene.d_obj = args.scene.d_obj_derived = copy.view.rec;
    args.scene.d_emissive = copy.d_lights;
    k.view = copy.view;
}

}  // namespace

int pt_accel_device_view(mc_context* ctx, const mc_pathtrace_accel* a, hipStream_t s, bvh::View& view) {
    DeviceCopy copy{};
    if (int rc = device_copy(ctx, a, s, copy)) return rc;
    view = copy.view;
    return MC_OK;
}

int pathtrace_accel_launch(mc_context* ctx, const mc_pathtrace_accel* a, const mc_pathtrace_params* p, void* d_rgba, hipStream_t s,
                           const char* who) {
    if (!ctx || !d_rgba) return refuse(who, "a NULL pointer");
    Plan plan;
    if (int rc = plan_request(a, p, who, plan)) return rc;
    DeviceCopy copy{};
    if (int rc = device_copy(ctx, a, s, copy)) return rc;
    BvhArgs k;
    fill_args(a, p, copy, k);
    PTArgs& args = k.a;
    args.out = (float4*)d_rgba;
    const uint32_t rows = tile_rows(p->row_begin, p->row_end, args.row_block, args.row_stride);
    auto launch = [&](const BvhArgs& ka, int width) {
        return plan.math_mode == MC_PT_MATH_STRICT ? pt::launch_bvh_tier<0>(ka, width, rows, s) : pt::launch_bvh_tier<2>(ka, width, rows, s);
    };
    int rc;
    if (plan.tail_S) {
        const uint32_t rest = (p->sample_end - p->sample_begin) % (uint32_t)plan.S;
        BvhArgs head = k, tail = k;
        head.a.sample_end = tail.a.sample_begin = args.sample_end - rest;
        if ((rc = launch(head, plan.S))) return rc;
        if ((rc = launch(tail, plan.tail_S))) return rc;
    } else {
        if ((rc = launch(k, plan.S))) return rc;
    }
    MC_HIP_TRY(hipGetLastError());
    return ctx->note_launch(s);   // the kernels read the cached device copy
}

// The list render: pt_budget_list_render's checks in its order and words (the object's and plan_request's in place of the tables'), then
// pathtrace_bvh_list_kernel at the width choose_S gives for n_list ENTRIES and the range's samples.  A ragged sample count takes the
// two launches plan_request plans for a render; the prescale is the FIRST launch's alone: the tail continues (sample_begin > 0) what
// the head has already scaled and stored, and gets 1.0f.
int pathtrace_accel_list_render(mc_context* ctx, const mc_pathtrace_accel* a, const mc_pathtrace_params* p, const void* d_list, uint32_t n_list,
                                float prescale, void* d_acc, const char* who, hipStream_t s) {
    auto misaligned = [](const void* q, uintptr_t to) { return reinterpret_cast<uintptr_t>(q) % to != 0u; };
    if (!p) return refuse(who, "the render parameters are NULL");
    if (!p->width || !p->height) return refuse(who, "width and height must be above 0");
    if ((uint64_t)p->width * p->height > (1ull << 31)) return refuse(who, "more than 2^31 pixels: a list holds 32-bit storage indices");
    if (!whole_image(p) || p->row_block)
        return refuse(who, "whole-image addressing only (row_begin = 0, row_end = height, no interleave): an entry is a storage index of the image");
    Plan plan;
    if (int rc = plan_request(a, p, who, plan)) return rc;   // (the object, the ranges, the math mode, the flags; an MC_PT_PRECISION variant by name)
    if (!d_acc || (!d_list && n_list)) return refuse(who, "the accumulator plane or the list is NULL");
    if (misaligned(d_acc, 16u)) return refuse(who, "the accumulator plane must be aligned to 16 bytes");
    if (misaligned(d_list, 4u)) return refuse(who, "the list must be aligned to 4 bytes");
    if (n_list > (1u << 31)) return refuse(who, "more than 2^31 entries");
    {
        const uintptr_t x = reinterpret_cast<uintptr_t>(d_acc), y = reinterpret_cast<uintptr_t>(d_list);
        const size_t na = (size_t)p->width * p->height * 16, nb = (size_t)n_list * 4;
        if (d_list && x < y + nb && y < x + na) return refuse(who, "the accumulator plane overlaps the list");
    }
    if (!ctx) return refuse(who, "the context is NULL");
    if (!n_list) return MC_OK;
    // the width for the ENTRIES (plan_request's is the image's), and its tail
    const uint32_t n_samples = p->sample_end - p->sample_begin;
    const int S = choose_S(n_list, n_samples);
    const uint32_t rest = n_samples % (uint32_t)S;
    const int tail_S = (S > 1 && rest != 0u && n_samples > (uint32_t)S) ? (rest >= 4u ? 4 : 1) : 0;
    DeviceCopy copy{};
    if (int rc = device_copy(ctx, a, s, copy)) return rc;
    BvhArgs k;
    fill_args(a, p, copy, k);
    k.a.out = (float4*)d_acc;
    auto launch = [&](const BvhArgs& ka, float scale, int width) {
        const pt::BvhListArgs l{(const uint32_t*)d_list, n_list, scale};
        return plan.math_mode == MC_PT_MATH_STRICT ? pt::launch_bvh_list_tier<0>(ka, l, width, s) : pt::launch_bvh_list_tier<2>(ka, l, width, s);
    };
    int rc;
    if (tail_S) {
        BvhArgs head = k, tail = k;
        head.a.sample_end = tail.a.sample_begin = p->sample_end - rest;
        if ((rc = launch(head, prescale, S))) return rc;
        if ((rc = launch(tail, 1.0f, tail_S))) return rc;
    } else {
        if ((rc = launch(k, prescale, S))) return rc;
    }
    MC_HIP_TRY(hipGetLastError());
    return ctx->note_launch(s);
}

}  // namespace mc

extern "C" {

int mc_pathtrace_accel_select_kernel(const mc_pathtrace_accel* a, const mc_pathtrace_params* p, mc_pathtrace_kernel_info* out) {
    return mc::pathtrace_accel_select(a, p, out, "mc_pathtrace_accel_select_kernel");
}

int mc_pathtrace_render_accel_device_async(mc_context* ctx, const mc_pathtrace_accel* a, const mc_pathtrace_params* p, void* d_rgba_f32,
                                           void* stream) {
    const char* who = "mc_pathtrace_render_accel_device_async";
    if (!ctx) return mc::refuse(who, "the context is NULL");
    MC_HIP_TRY(hipSetDevice(ctx->device));
    return mc::pathtrace_accel_launch(ctx, a, p, d_rgba_f32, stream ? (hipStream_t)stream : ctx->stream, who);
}

int mc_pathtrace_render_accel_list_device_async(mc_context* ctx, const mc_pathtrace_accel* a, const mc_pathtrace_params* p, const void* d_list,
                                                uint32_t n_list, float prescale, void* d_acc, void* stream) {
    const char* who = "mc_pathtrace_render_accel_list_device_async";
    // (a NULL context is refused after the arguments: every refusal of theirs shows on a machine without a device)
    if (ctx) MC_HIP_TRY(hipSetDevice(ctx->device));
    return mc::pathtrace_accel_list_render(ctx, a, p, d_list, n_list, prescale, d_acc, who, stream ? (hipStream_t)stream : ctx ? ctx->stream : nullptr);
}

}  // extern "C"
