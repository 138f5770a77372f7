// Path tracer for gfx950 (MI355X) through the sphere BVH of pt_bvh.h — included by pt_bvh_strict.hip / pt_bvh_careful.hip, one tier each.
//
// The sample body and the kernel skeleton are those of the generic round-synchronous kernel that leaves the scene in memory
// (pathtrace_kernel.h: trace_sample / pathtrace_kernel with NP = NS = -2, Slab = false, Prec = 0), RESTATED here with intersect() replaced by
// bvh::intersect_bvh, so that pathtrace_kernel.h — and with it the existing kernels' code and the build id's pt= part — stays untouched.
// Everything else is that header's own: rand01, camera_ray, light_sample_direction, cosine_bounce, specular_bounce_general, divs*, the
// derived record slots, the ordered fold.  Strict sums are therefore the oracle's, and sample ranges and row tiles compose bit for bit
// with one another and with the linear kernels'.
//
// MI355X mapping: S lanes per pixel (1, 4, 16), as there.  The plane list and the unboxed list are read with wave-uniform indices (scalar
// loads); the walk is PER LANE — after the first bounce a wave's rays diverge — so a node is two 16-byte vector loads, a leaf sphere one 16-byte
// and one 4-byte vector load.  The walk is stackless (depth-first order, one skip link per node): no private array, no scratch.  No LDS, no
// atomics, no inline assembly beyond the empty register barriers the skeleton already uses.
//
// Two kernels share the sample body: pathtrace_bvh_kernel (a lane group per pixel of the launch grid; §3.18) and pathtrace_bvh_list_kernel
// (a lane group per entry of a list of storage indices, the accumulator left linear: the budgeted chain's rounds; §3.24).
#pragma once
#include "pathtrace_kernel.h"
#include "pt_bvh.h"

namespace mc {
namespace pt {

struct BvhArgs {
    PTArgs a;        // a.scene: n_planes, n_spheres, n_emissive, d_obj_derived, d_emissive; the rest of SceneArgs is unused
    bvh::View view;  // device pointers; view.rec = a.scene.d_obj_derived (slots 0 .. 3 are the records' own)
};

// The tier's division and square root inside the shared body: the helpers the linear kernels of the same tier use.
template <int Fast> struct TierOps {
    static __device__ __forceinline__ float div(float a, float b) { return dm::fdiv<Fast>(a, b); }
    static __device__ __forceinline__ float sqrt(float a) { return dm::fsqrt<Fast>(a); }
};

template <int Fast> __device__ __forceinline__ int intersect_accel(const bvh::View& v, v3 o, v3 d, float& t) {
    MC_PT_DECISION_FP
    return bvh::intersect_bvh<TierOps<Fast>>(v, bvh::f3{o.x, o.y, o.z}, bvh::f3{d.x, d.y, d.z}, t);
}

// One sample: returns accrad (pathTracer.comp:356-449) — trace_sample<Fast, -2, -2, false, 0>, restated.
template <int Fast>
__device__ __forceinline__ v3 trace_sample_bvh(const BvhArgs& k, uint32_t gx, uint32_t gy, uint32_t samp) {
    const PTArgs& a = k.a;
    const SceneArgs& sc = a.scene;
    const float* __restrict__ rec = sc.d_obj_derived;
    const uint32_t* __restrict__ lights = sc.d_emissive;
    const int np = (int)sc.n_planes;
    v3 accrad{0.0f, 0.0f, 0.0f}, accmat{1.0f, 1.0f, 1.0f};               // :361
    v3 ro = a.lc, rd = camera_ray<Fast>(a, gx, gy, samp);                 // :362
    float emissive = 1.0f;                                                // :365
    for (uint32_t depth = 0; depth < a.max_depth; depth++) {              // :367
        float t;
        const int id = intersect_accel<Fast>(k.view, ro, rd, t);
        if (id < 0) break;                                                // :369
        v3 x = ro + rd * t;                                               // :374
        const float* obj = rec + 12 * (size_t)id;                         // per-lane fetch
        const bool is_sphere = id >= np;
        v3 geo{obj[0], obj[1], obj[2]};
        v3 col{obj[8], obj[9], obj[10]};
        const int mat = (int)obj[11];                                     // = int(floor(m + 0.5)), :378/:384
        const float p = obj[7];                                           // = max(max(c.x, c.y), c.z), :394
        v3 n = is_sphere ? normalize<Fast>(x - geo) : geo;                // :381/:387
        float dot_n_rd = 0.0f;
        v3 nl;                                                            // :390
        if constexpr (Fast) {
            dot_n_rd = dot(n, rd);
            const uint32_t flip = ~dm::as_uint(dot_n_rd) & 0x80000000u;
            nl = v3{dm::as_float(dm::as_uint(n.x) ^ flip), dm::as_float(dm::as_uint(n.y) ^ flip), dm::as_float(dm::as_uint(n.z) ^ flip)};
        } else {
            nl = dot(n, rd) < 0.0f ? n : -n;
        }
        {
            v3 emi{obj[4], obj[5], obj[6]};
            accrad = accrad + (accmat * emi) * emissive;                  // :391
        }
        accmat = accmat * col;                                            // :392
        v3 rnd = rand01(gx, gy, samp * a.max_depth + depth);              // :393
        if (depth > 5) {                                                  // :395
            if (rnd.z >= p) break;                                        // :396
            accmat = divs<Fast>(accmat, p);                               // :397
        }
        if (mat == 1) {                                                   // :400 diffuse
            const int n_lights = (int)sc.n_emissive;
            v3 accmat_over_pi{0.0f, 0.0f, 0.0f};
            if constexpr (!Fast) accmat_over_pi = divs_recip<Fast>(accmat, kPi, kInvPi);
            for (int kk = 0; kk < n_lights; kk++) {                       // :403
                const int i = (int)lights[kk];                            // host-built list of the spheres passing :407
                const float* ls = rec + 12 * (size_t)(np + i);
                const float lr2 = ls[3] * ls[3];
                const v3 lc{ls[0], ls[1], ls[2]};
                const v3 le{ls[4], ls[5], ls[6]};
                const v3 xc = lc - x;                                     // :408
                const float xcc = dot(xc, xc);
                float cos_a_max;
                v3 l = light_sample_direction<Fast>(xc, xcc, lr2, rnd, cos_a_max);   // :409-:413
                float tne;
                const bool reached = intersect_accel<Fast>(k.view, x, l, tne) == np + i;   // :420: the NEAREST hit is sphere i
                if (reached) {
                    float omega = (2.0f * kPi) * (1.0f - cos_a_max);      // :421
                    if constexpr (Fast) {
                        const float scale = __builtin_fmaxf(dot(l, nl), 0.0f) * (2.0f - (cos_a_max + cos_a_max));
                        accrad = accrad + (accmat * le) * scale;
                    } else {
                        accrad = accrad + ((accmat_over_pi * dm::gmax(dot(l, nl), 0.0f)) * le) * omega;   // :422
                    }
                }
            }
            rd = cosine_bounce<Fast, false>(nl, rnd);                     // :426-:428
            ro = x;
            emissive = 0.0f;                                              // :429
        } else if (mat == 2 || mat == 3) {                                // :432 mirror, :437 glass
            MC_PT_DECISION_FP
            rd = specular_bounce_general<Fast, false>(mat, rd, n, nl, dot_n_rd, rnd.x, accmat);
            ro = x;
            emissive = 1.0f;                                              // :447
        }
    }
    return accrad;
}

template <int Fast, int S>
__global__ void __launch_bounds__(256) pathtrace_bvh_kernel(BvhArgs k) {
    const PTArgs& a = k.a;
    constexpr uint32_t TW = WaveTile<S>::w, TH = WaveTile<S>::h;
    // (lane coordinates derived afresh where needed, through an opaque copy: dead inside the bounce loop — see pathtrace_kernel)
    struct LaneCoords { uint32_t j, gx, gy; size_t idx; bool valid; };
    auto lane_coords = [&]() {
        uint32_t tid = threadIdx.x, row_block = a.row_block;
        asm volatile("" : "+v"(tid));
        asm volatile("" : "+s"(row_block));
        const uint32_t lane = tid & 63u, wave = tid >> 6;
        LaneCoords c;
        c.j = lane % (uint32_t)S;
        const uint32_t pix = lane / (uint32_t)S;
        c.gx = blockIdx.x * (2u * TW) + (wave & 1u) * TW + (pix % TW);
        const uint32_t ty = blockIdx.y * (2u * TH) + (wave >> 1) * TH + (pix / TW);   // tile-local storage row
        const uint32_t r = tile_row_to_storage(ty, a.row_begin, row_block, a.row_stride);
        c.valid = c.gx < a.W && r < a.row_end;                                  // pathTracer.comp:348
        c.gy = a.H - 1u - (c.valid ? r : 0u);                                   // :349
        c.idx = c.valid ? (size_t)ty * a.W + c.gx : 0;
        return c;
    };
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (a.sample_begin > 0) {   // progressive continuation (samps.x protocol)
        const LaneCoords c = lane_coords();
        if (c.valid) acc = a.out[c.idx];
    }
    const float fspp = (float)a.spp;
    for (uint32_t base = a.sample_begin; base < a.sample_end; base += (uint32_t)S) {
        const LaneCoords c = lane_coords();
        const uint32_t s = base + c.j;
        v3 q{0.0f, 0.0f, 0.0f};
        if (c.valid && s < a.sample_end) {
            v3 rad = trace_sample_bvh<Fast>(k, c.gx, c.gy, s);
            q = Fast ? rad * a.inv_spp : divs_recip<Fast>(rad, fspp, a.inv_spp);      // :452
        }
        // the round's S samples into the accumulator in sample order (every lane of the group performs the same additions)
        const uint32_t count = min((uint32_t)S, a.sample_end - base);           // wave-uniform
        if (S == 1) {
            acc.x += q.x; acc.y += q.y; acc.z += q.z; acc.w += 0.0f;
        } else {
            uint32_t tid = threadIdx.x;
            asm volatile("" : "+v"(tid));
            const uint32_t first = (tid & 63u) - (tid & 63u) % (uint32_t)S;
            auto from_lane = [](float v, uint32_t src) {
                return __int_as_float(__builtin_amdgcn_ds_bpermute((int)(src << 2), __float_as_int(v)));
            };
            for (uint32_t kk = 0; kk < count; kk++) {
                const uint32_t src = first + kk;
                acc.x += from_lane(q.x, src); acc.y += from_lane(q.y, src); acc.z += from_lane(q.z, src); acc.w += 0.0f;
            }
        }
    }
    const LaneCoords c = lane_coords();
    if (a.sample_end == a.spp) {                                                // :453 after sample spp-1
        acc.x = dm::fpow<Fast>(dm::gmin(dm::gmax(acc.x, 0.0f), 1.0f), 0.45f) * 255.0f + 0.5f;
        acc.y = dm::fpow<Fast>(dm::gmin(dm::gmax(acc.y, 0.0f), 1.0f), 0.45f) * 255.0f + 0.5f;
        acc.z = dm::fpow<Fast>(dm::gmin(dm::gmax(acc.z, 0.0f), 1.0f), 0.45f) * 255.0f + 0.5f;
    }
    if (c.valid && c.j == 0) a.out[c.idx] = acc;
}

// ---- the LIST RENDER through the tree (include/mc_compute.h, mc_pathtrace_render_accel_list_device_async) -----------
// pathtrace_list_kernel of pt_budget_kernel.h — an S-lane group takes one ENTRY of a list of storage indices, its accumulator is read
// from the plane, scaled by `prescale`, continued over [sample_begin, sample_end) in sample order and stored back LINEAR (never :453) —
// RESTATED with trace_sample_bvh as the sample, as pathtrace_bvh_kernel above restates pathtrace_kernel.  The scene stays in memory (the
// NP = -2 family): nothing is staged, no LDS.  Bounds: an entry is read only below `count`; an entry >= W * H is skipped (no load, no
// trace, no store).  Entries must be distinct.
struct BvhListArgs {
    const uint32_t* __restrict__ list;   // storage indices row * W + gx, any order, distinct
    uint32_t count;                      // entries, > 0
    float prescale;                      // the stored accumulator is multiplied by this before the range is added (sample_begin > 0)
};

// Waves per SIMD the list kernel's register budget is set for: what pathtrace_bvh_kernel of the same tier and width gets on its own (7 in the
// careful tier and at S = 1, 6 in the strict tier at S = 4 and 16), so that a round never runs at a lower occupancy than the render it continues.
// (Left to itself the strict S = 1 list kernel takes 73 VGPRs, one above the 72 that seven waves allow.)
template <int Fast, int S> constexpr int bvh_list_waves() { return (Fast || S == 1) ? 7 : 6; }

template <int Fast, int S>
__global__ void __launch_bounds__(256, (bvh_list_waves<Fast, S>())) pathtrace_bvh_list_kernel(BvhArgs k, BvhListArgs l) {
    const PTArgs& a = k.a;
    // (a lane's entry, pixel and sample slot derived afresh where needed, through an opaque copy: see pathtrace_list_kernel)
    struct LaneCoords { uint32_t j, gx, gy, idx; bool valid; };
    auto lane_coords = [&]() {
        uint32_t tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        LaneCoords c;
        c.j = tid % (uint32_t)S;                                                        // (S divides 64: the slot within the wave's group)
        const uint32_t entry = blockIdx.x * (256u / (uint32_t)S) + tid / (uint32_t)S;   // a wave's groups are adjacent entries
        const bool listed = entry < l.count;
        const uint32_t idx = l.list[listed ? entry : 0u];
        c.valid = listed && idx < a.W * a.H;            // (the host refuses images of more than 2^31 pixels)
        c.idx = c.valid ? idx : 0u;
        const uint32_t row = c.idx / a.W;
        c.gx = c.idx - row * a.W;
        c.gy = a.H - 1u - row;                          // pathTracer.comp:349
        return c;
    };
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (a.sample_begin > 0) {
        const LaneCoords c = lane_coords();
        if (c.valid) {
            acc = a.out[c.idx];
            acc.x = acc.x * l.prescale; acc.y = acc.y * l.prescale; acc.z = acc.z * l.prescale; acc.w = acc.w * l.prescale;
        }
    }
    const float fspp = (float)a.spp;
    for (uint32_t base = a.sample_begin; base < a.sample_end; base += (uint32_t)S) {
        const LaneCoords c = lane_coords();
        const uint32_t s = base + c.j;
        v3 q{0.0f, 0.0f, 0.0f};
        if (c.valid && s < a.sample_end) {
            v3 rad = trace_sample_bvh<Fast>(k, c.gx, c.gy, s);
            q = Fast ? rad * a.inv_spp : divs_recip<Fast>(rad, fspp, a.inv_spp);      // :452, as pathtrace_bvh_kernel
        }
        // the round's S samples into the accumulator in sample order (pathtrace_bvh_kernel's fold)
        const uint32_t count = min((uint32_t)S, a.sample_end - base);
        if (S == 1) {
            acc.x += q.x; acc.y += q.y; acc.z += q.z; acc.w += 0.0f;
        } else {
            uint32_t tid = threadIdx.x;
            asm volatile("" : "+v"(tid));
            const uint32_t first = (tid & 63u) - (tid & 63u) % (uint32_t)S;
            auto from_lane = [](float v, uint32_t src) {
                return __int_as_float(__builtin_amdgcn_ds_bpermute((int)(src << 2), __float_as_int(v)));
            };
            for (uint32_t kk = 0; kk < count; kk++) {
                const uint32_t src = first + kk;
                acc.x += from_lane(q.x, src); acc.y += from_lane(q.y, src); acc.z += from_lane(q.z, src); acc.w += 0.0f;
            }
        }
    }
    const LaneCoords c = lane_coords();
    if (c.valid && c.j == 0u) a.out[c.idx] = acc;   // linear: no :453 here, whatever sample_end is
}

// The launchers of one tier (Fast = 0 strict, 2 careful), instantiated by the tier's own translation unit.
template <int Fast> int launch_bvh_tier(const BvhArgs& k, int S, uint32_t tile_rows, hipStream_t s);
template <int Fast> int launch_bvh_list_tier(const BvhArgs& k, const BvhListArgs& l, int S, hipStream_t s);

template <int Fast> int launch_bvh_list_tier_impl(const BvhArgs& k, const BvhListArgs& l, int S, hipStream_t s) {
    return dispatch<1, 4, 16>(S, [&](auto W) {
        constexpr int Sv = decltype(W)::value;
        constexpr uint32_t per_block = 256u / (uint32_t)Sv;
        hipLaunchKernelGGL((pathtrace_bvh_list_kernel<Fast, Sv>), dim3((l.count + per_block - 1u) / per_block), dim3(256), 0, s, k, l);
        return (int)MC_OK;
    });
}

template <int Fast> int launch_bvh_tier_impl(const BvhArgs& k, int S, uint32_t tile_rows, hipStream_t s) {
    return dispatch<1, 4, 16>(S, [&](auto W) {
        constexpr int Sv = decltype(W)::value;
        dim3 grid((k.a.W + block_w<Sv>() - 1u) / block_w<Sv>(), (tile_rows + block_h<Sv>() - 1u) / block_h<Sv>());
        hipLaunchKernelGGL((pathtrace_bvh_kernel<Fast, Sv>), grid, dim3(256), 0, s, k);
        return (int)MC_OK;
    });
}

}  // namespace pt
}  // namespace mc
