// Path tracer, per-pixel sample budgets: the LIST RENDER (include/mc_compute.h, mc_pathtrace_render_list_device_async).
// Included by pt_budget_strict.hip / pt_budget_careful.hip / pt_budget_fast.hip, one tier each, as pathtrace_kernel.h is by the plain tiers.
//
// pathtrace_kernel of pathtrace_kernel.h with the pixel of a lane group taken from a LIST of storage indices instead of the launch grid:
// an S-lane group (S = 1, 4, 16) takes one entry, a wave 64 / S entries, a block of four waves 256 / S.  The accumulator of a listed pixel
// is read from the plane, scaled by `prescale` (1 or 0.5: exact), continued over [sample_begin, sample_end) in sample order exactly as
// pathtrace_kernel folds a round (:451-:452) and stored back LINEAR: the :453 encode is never applied, the resolve does it (pt_budget.h).
// One sample is trace_sample of pathtrace_kernel.h, unchanged; the families are the round-synchronous ones: slab (NP = 6, NS = 1 .. 8),
// generic with the records staged in LDS (-1) or read from memory (-2).
//
// Bounds: an entry is read only below `count`; an entry >= W * H is skipped (no load, no trace, no store), so a bad list cannot reach
// memory outside the plane.  Entries must be distinct: two groups on one pixel would race on its accumulator.
#pragma once
#include "pathtrace_kernel.h"

namespace mc {
namespace pt {

struct ListArgs {
    const uint32_t* __restrict__ list;   // storage indices row * W + gx, any order, distinct
    uint32_t count;                      // entries, > 0
    float prescale;                      // the stored accumulator is multiplied by this before the range is added (sample_begin > 0)
};

template <int Fast, int NP, int NS, bool Slab, int S>
__global__ void __launch_bounds__(256, (rounds_waves<Fast, Slab, NS>())) pathtrace_list_kernel(PTArgs a, ListArgs l) {
    extern __shared__ float lds_dyn[];
    float* lds_obj = lds_dyn;
    const uint32_t n_rec = (a.scene.n_planes + a.scene.n_spheres) * 12u;
    uint32_t* lds_emissive = reinterpret_cast<uint32_t*>(lds_dyn + n_rec);
    if (NP == -2) {          // generic, scene left in memory (pathtrace_kernel has the reasons)
        lds_obj = const_cast<float*>(a.scene.d_obj_derived);
        lds_emissive = const_cast<uint32_t*>(a.scene.d_emissive);
    } else if (NP < 0) {     // generic: stage from the device buffer
        for (uint32_t i = threadIdx.x; i < a.scene.n_emissive; i += blockDim.x) lds_emissive[i] = a.scene.d_emissive[i];
        stage_records(lds_obj, a.scene.d_obj, a.scene.n_planes + a.scene.n_spheres, false);
    } else {                 // slab: stage the kernel-argument copy for the per-lane material fetch
        stage_records(lds_obj, a.scene.obj, a.scene.n_planes + a.scene.n_spheres, Slab);
    }
    // A lane's entry, pixel and sample slot: derived afresh from the thread id and the list wherever they are needed, through an opaque copy,
    // as pathtrace_kernel's lane_coords and for its reason — carried through the bounce loop they spill.  The entry is re-read from the
    // list (4 bytes per group and round, out of the cache after the first) rather than kept.
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
    HotSlabN<slab_spheres<Slab, NS>()> hot;
    if constexpr (Slab) hot.template load<(NS <= 3)>(a.scene);
    for (uint32_t base = a.sample_begin; base < a.sample_end; base += (uint32_t)S) {
        const LaneCoords c = lane_coords();
        const uint32_t s = base + c.j;
        v3 q{0.0f, 0.0f, 0.0f};
        if (c.valid && s < a.sample_end) {
            v3 rad = trace_sample<Fast, NP, NS, Slab, 0, false>(a, lds_obj, lds_emissive, hot, c.gx, c.gy, s);
            q = Fast ? rad * a.inv_spp : divs_recip<Fast>(rad, fspp, a.inv_spp);      // :452, as pathtrace_kernel
        }
        // the round's S samples into the accumulator in sample order (pathtrace_kernel's fold)
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
            for (uint32_t k = 0; k < count; k++) {
                const uint32_t src = first + k;
                acc.x += from_lane(q.x, src); acc.y += from_lane(q.y, src); acc.z += from_lane(q.z, src); acc.w += 0.0f;
            }
        }
    }
    const LaneCoords c = lane_coords();
    if (c.valid && c.j == 0u) a.out[c.idx] = acc;   // linear: no :453 here, whatever sample_end is
}

template <int Fast, int NP, int NS, bool Slab, int S>
inline int launch_list_one(const PTArgs& a, const ListArgs& l, hipStream_t s) {
    constexpr uint32_t per_block = 256u / (uint32_t)S;
    const dim3 grid((l.count + per_block - 1u) / per_block);
    const size_t lds = NP == -2 ? 0u : scene_lds_bytes(a);
    auto kern = pathtrace_list_kernel<Fast, NP, NS, Slab, S>;
    if (lds > 48u * 1024u) {   // beyond the default dynamic-LDS window (launch_one)
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            set_error_detail(std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") + hipGetErrorString(e));
            return MC_ERR_HIP;
        }
    }
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, a, l);
    return MC_OK;
}

// One tier's list launcher (Fast = the MC_PT_MATH_* value that runs), specialised by the tier's translation unit so that the kernels are
// compiled under that unit's floating-point settings.  kernel: MC_PT_KERNEL_SLAB, _GENERIC or _GENERIC_MEMORY; S: 1, 4, 16.
template <int Fast> int launch_list_tier(const PTArgs& a, const ListArgs& l, int kernel, int S, hipStream_t s);
template <> int launch_list_tier<0>(const PTArgs& a, const ListArgs& l, int kernel, int S, hipStream_t s);
template <> int launch_list_tier<1>(const PTArgs& a, const ListArgs& l, int kernel, int S, hipStream_t s);
template <> int launch_list_tier<2>(const PTArgs& a, const ListArgs& l, int kernel, int S, hipStream_t s);

template <int Fast> inline int launch_list_tier_impl(const PTArgs& a, const ListArgs& l, int kernel, int S, hipStream_t s) {
    switch (kernel) {
        case MC_PT_KERNEL_SLAB:
            return dispatch_spheres(a.scene.n_spheres, [&](auto NS) {
                return dispatch<1, 4, 16>(S, [&](auto W) { return launch_list_one<Fast, 6, NS, true, W>(a, l, s); });
            });
        case MC_PT_KERNEL_GENERIC_MEMORY: return dispatch<1, 4, 16>(S, [&](auto W) { return launch_list_one<Fast, -2, -2, false, W>(a, l, s); });
        case MC_PT_KERNEL_GENERIC: return dispatch<1, 4, 16>(S, [&](auto W) { return launch_list_one<Fast, -1, -1, false, W>(a, l, s); });
        default: return MC_ERR_INVALID_ARGUMENT;
    }
}

}  // namespace pt
}  // namespace mc
