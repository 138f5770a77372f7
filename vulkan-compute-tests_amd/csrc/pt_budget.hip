// Path tracer, per-pixel sample budgets for gfx950 (MI355X): levels from the noise plane, the bucketed pixel lists, the resolve, and the
// entry point of the list render.  Contract in include/mc_compute.h, restated in tests/pt_budget_ref.py; scheme and measurements in
// DESIGN.md §3.20.  The arithmetic is pt_budget.h, the same source mc_pathtrace_budget_levels and mc_pathtrace_budget_resolve run on the
// host.  Built like pt_noise.hip: no contraction.
//
// Four small kernels, a lane on ONE pixel, blocks of 256 lanes on 256 adjacent pixels of the plane; vector loads and stores only.
//  * pt_budget_levels_kernel: a 4-B load, at most eight multiplications by 0.5, a 1-B store.
//  * pt_budget_count_kernel / pt_budget_scatter_kernel: the list as §3.12 builds its list — a ballot per level, a vector atomic for the
//    wave's share, plain C++ — in two passes, since the buckets' starts are only known once every pixel is counted.  A block walks four
//    tiles of 256 pixels and gathers its sixteen (tile, wave) groups in LDS, so that ONE global atomic per block and level reaches memory
//    (the first form, one returning atomic per wave and level on a handful of addresses, took 0.27 ms at 900 x 600: longer than a round).
//    The scatter pass takes the block's slot in a level's bucket from a cursor, a group's place in the slot from the LDS table and a
//    lane's place in its group from the ballot.  Buckets lie highest level first: a round's pixels are a prefix.  The order of the
//    blocks' slots inside a bucket follows the atomics' and is not specified.
//  * pt_budget_resolve_kernel: a 16-B load, a 1-B load, three strict pow(x, 0.45), a 16-B store; in place allowed (a lane reads its pixel
//    before it writes it and no other).
#include <cmath>
#include <vector>

#include "pt_budget_host.h"

namespace mc {

namespace {

using ptd::vec4;
using namespace ptdh;

__global__ void __launch_bounds__(256) pt_budget_levels_kernel(const float* __restrict__ variance, uint8_t* __restrict__ levels, uint32_t n,
                                                               float tau2, uint32_t max_level) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p < n) levels[p] = ptd::budget_level(variance[p], tau2, max_level);
}

// A lane's level, or an impossible one past the plane's end (every lane of a wave reaches every ballot).
__device__ __forceinline__ uint32_t lane_level(const uint8_t* __restrict__ levels, uint32_t p, uint32_t n, uint32_t max_level) {
    if (p >= n) return 0xffffffffu;
    const uint32_t l = levels[p];
    return l < max_level ? l : max_level;
}

constexpr uint32_t kListTiles = 4;                      // tiles of 256 pixels a block of the two list kernels walks
constexpr uint32_t kListBlock = 256u * kListTiles;      // pixels per block
constexpr uint32_t kLevels = ptd::kMaxBudgetLevel + 1u;

__global__ void __launch_bounds__(256) pt_budget_count_kernel(const uint8_t* __restrict__ levels, uint32_t n, uint32_t max_level,
                                                              uint32_t* __restrict__ counts) {
    __shared__ uint32_t block_counts[kLevels];
    if (threadIdx.x < kLevels) block_counts[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t tile = 0; tile < kListTiles; tile++) {
        const uint32_t l = lane_level(levels, blockIdx.x * kListBlock + tile * 256u + threadIdx.x, n, max_level);
        for (uint32_t k = 0; k <= max_level; k++) {
            const unsigned long long m = __ballot(l == k);
            if (m != 0ull && lane == (uint32_t)(__ffsll((long long)m) - 1)) atomicAdd(&block_counts[k], (uint32_t)__popcll(m));
        }
    }
    __syncthreads();
    if (threadIdx.x <= max_level && block_counts[threadIdx.x] != 0u) atomicAdd(&counts[threadIdx.x], block_counts[threadIdx.x]);
}

// A block's pixels of one level take ONE slot of that level's bucket (one global atomic per block and level: lane k of the block asks for
// level k); inside the slot the (tile, wave) groups lie in order, and a lane's place in its group is its rank in the ballot.
__global__ void __launch_bounds__(256) pt_budget_scatter_kernel(const uint8_t* __restrict__ levels, uint32_t n, uint32_t max_level,
                                                                const uint32_t* __restrict__ counts, uint32_t* __restrict__ cursors,
                                                                uint32_t* __restrict__ list) {
    __shared__ uint32_t group_at[kListTiles * 4u][kLevels];   // first a group's count per level, then where the group starts in the list
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t l[kListTiles], rank[kListTiles];
    for (uint32_t tile = 0; tile < kListTiles; tile++) {
        l[tile] = lane_level(levels, blockIdx.x * kListBlock + tile * 256u + threadIdx.x, n, max_level);
        rank[tile] = 0u;
        for (uint32_t k = 0; k <= max_level; k++) {
            const unsigned long long m = __ballot(l[tile] == k);
            if (l[tile] == k) rank[tile] = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (lane == 0u) group_at[tile * 4u + wave][k] = (uint32_t)__popcll(m);
        }
    }
    __syncthreads();
    if (threadIdx.x <= max_level) {
        const uint32_t k = threadIdx.x;
        uint32_t total = 0u, bucket = 0u;   // the bucket of level k starts behind the counts of the levels above it
        for (uint32_t g = 0; g < kListTiles * 4u; g++) total += group_at[g][k];
        for (uint32_t j = k + 1u; j <= max_level; j++) bucket += counts[j];
        uint32_t at = bucket + (total != 0u ? atomicAdd(&cursors[k], total) : 0u);
        for (uint32_t g = 0; g < kListTiles * 4u; g++) {
            const uint32_t c = group_at[g][k];
            group_at[g][k] = at;
            at += c;
        }
    }
    __syncthreads();
    for (uint32_t tile = 0; tile < kListTiles; tile++) {
        if (l[tile] > max_level) continue;   // past the plane's end
        const uint32_t at = group_at[tile * 4u + wave][l[tile]] + rank[tile];
        if (at < n) list[at] = blockIdx.x * kListBlock + tile * 256u + threadIdx.x;   // (always, for counts of this plane: the guard keeps a stale count from reaching past the list)
    }
}

__global__ void __launch_bounds__(256) pt_budget_resolve_kernel(const vec4* acc, const uint8_t* __restrict__ levels, vec4* out, uint32_t n) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p < n) out[p] = ptd::budget_resolve(acc[p], levels ? (uint32_t)levels[p] : 0u);
}

bool misaligned4(const void* p) { return reinterpret_cast<uintptr_t>(p) % 4u != 0u; }
dim3 pixel_grid(size_t n) { return dim3((uint32_t)((n + 255u) / 256u)); }
dim3 list_grid(size_t n) { return dim3((uint32_t)((n + kListBlock - 1u) / kListBlock)); }

}  // namespace

int pt_budget_check(float target, uint32_t max_level, const char* who) {
    if (max_level > ptd::kMaxBudgetLevel) return refuse(who, "max_level = " + std::to_string(max_level) + " is above 8");
    if (!(target > 0.0f) || !std::isfinite(target) || !std::isfinite(target * target))
        return refuse(who, "target must be finite and above 0, and its fp32 square finite");
    return MC_OK;
}

int pt_budget_check_size(uint32_t W, uint32_t H, const char* who) {
    if (!W || !H) return refuse(who, "width and height must be above 0");
    if ((uint64_t)W * H > (1ull << 31)) return refuse(who, "more than 2^31 pixels: a list holds 32-bit storage indices");
    return MC_OK;
}

int pt_budget_levels_launch(mc_context* ctx, uint32_t W, uint32_t H, const void* d_variance, float target, uint32_t max_level, void* d_levels,
                            const char* who, hipStream_t s) {
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    if (int rc = pt_budget_check_size(W, H, who)) return rc;
    if (int rc = pt_budget_check(target, max_level, who)) return rc;
    if (!d_variance || !d_levels) return refuse(who, "a plane is NULL");
    if (misaligned4(d_variance)) return refuse(who, "the variance plane must be aligned to 4 bytes");
    const size_t npix = (size_t)W * H;
    if (overlaps(d_levels, npix, d_variance, npix * 4)) return refuse(who, "the level plane overlaps the variance plane");
    hipLaunchKernelGGL(pt_budget_levels_kernel, pixel_grid(npix), dim3(256), 0, s, (const float*)d_variance, (uint8_t*)d_levels, (uint32_t)npix,
                       target * target, max_level);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

int pt_budget_lists_launch(mc_context* ctx, uint32_t W, uint32_t H, const void* d_levels, uint32_t max_level, void* d_list, void* d_counts,
                           void* d_cursors, const char* who, hipStream_t s) {
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    if (int rc = pt_budget_check_size(W, H, who)) return rc;
    if (max_level > ptd::kMaxBudgetLevel) return refuse(who, "max_level = " + std::to_string(max_level) + " is above 8");
    if (!d_levels || !d_list || !d_counts || !d_cursors) return refuse(who, "a plane, the list or the counts are NULL");
    if (misaligned4(d_list) || misaligned4(d_counts)) return refuse(who, "the list and the counts must be aligned to 4 bytes");
    const size_t npix = (size_t)W * H, counts_bytes = 4u * (ptd::kMaxBudgetLevel + 1u);
    if (overlaps(d_list, npix * 4, d_levels, npix) || overlaps(d_counts, counts_bytes, d_levels, npix) || overlaps(d_counts, counts_bytes, d_list, npix * 4))
        return refuse(who, "the list, the counts and the level plane overlap");
    MC_HIP_TRY(hipMemsetAsync(d_counts, 0, counts_bytes, s));
    MC_HIP_TRY(hipMemsetAsync(d_cursors, 0, counts_bytes, s));
    hipLaunchKernelGGL(pt_budget_count_kernel, list_grid(npix), dim3(256), 0, s, (const uint8_t*)d_levels, (uint32_t)npix, max_level, (uint32_t*)d_counts);
    MC_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(pt_budget_scatter_kernel, list_grid(npix), dim3(256), 0, s, (const uint8_t*)d_levels, (uint32_t)npix, max_level,
                       (const uint32_t*)d_counts, (uint32_t*)d_cursors, (uint32_t*)d_list);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

int pt_budget_resolve_launch(mc_context* ctx, uint32_t W, uint32_t H, const void* d_acc, const void* d_levels, void* d_out, const char* who,
                             hipStream_t s) {
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    if (int rc = pt_budget_check_size(W, H, who)) return rc;
    if (!d_acc || !d_out) return refuse(who, "a plane is NULL");
    if (misaligned(d_acc) || misaligned(d_out)) return refuse(who, "the vec4 planes must be aligned to 16 bytes");
    const size_t npix = (size_t)W * H;
    if (overlaps(d_out, npix * 16, d_levels, npix) || (d_out != d_acc && overlaps(d_out, npix * 16, d_acc, npix * 16)))
        return refuse(who, "the output overlaps the level plane, or the input without being the input (d_out == d_acc is the in-place form)");
    hipLaunchKernelGGL(pt_budget_resolve_kernel, pixel_grid(npix), dim3(256), 0, s, (const vec4*)d_acc, (const uint8_t*)d_levels, (vec4*)d_out,
                       (uint32_t)npix);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

int pt_budget_list_render(mc_context* ctx, const mc_pathtrace_params* p, const float* planes, uint32_t n_planes, const float* spheres,
                          uint32_t n_spheres, const void* d_list, uint32_t n_list, float prescale, void* d_acc, const char* who, hipStream_t s) {
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    if (!p) return refuse(who, "the render parameters are NULL");
    if (int rc = pt_budget_check_size(p->width, p->height, who)) return rc;
    if (!whole_image(p) || p->row_block)
        return refuse(who, "whole-image addressing only (row_begin = 0, row_end = height, no interleave): an entry is a storage index of the image");
    if ((p->flags >> 16) & 0xfu) return refuse(who, "the MC_PT_PRECISION variants have no list kernels");
    mc_pathtrace_kernel_info info;
    if (int rc = pathtrace_select_kernel(p, planes, n_planes, spheres, n_spheres, &info)) return rc;   // (validates like the render)
    if (!d_acc || (!d_list && n_list)) return refuse(who, "the accumulator plane or the list is NULL");
    if (misaligned(d_acc)) return refuse(who, "the accumulator plane must be aligned to 16 bytes");
    if (misaligned4(d_list)) return refuse(who, "the list must be aligned to 4 bytes");
    if (n_list > (1u << 31)) return refuse(who, "more than 2^31 entries");
    if (overlaps(d_acc, (size_t)p->width * p->height * 16, d_list, (size_t)n_list * 4)) return refuse(who, "the accumulator plane overlaps the list");
    if (!n_list) return MC_OK;
    return pathtrace_list_launch(ctx, p, planes, n_planes, spheres, n_spheres, (const uint32_t*)d_list, n_list, prescale, d_acc, s);
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_pathtrace_budget_default_params(mc_pathtrace_budget_params* b) {
    if (!b) return MC_ERR_INVALID_ARGUMENT;
    b->max_level = 4u;
    b->target = 32.0f;  // DESIGN.md section 3.20 has the sweep it comes from
    b->radius = 3u;     // mc_pathtrace_noise_default_params'
    b->flags = 0u;
    return MC_OK;
}

int mc_pathtrace_budget_levels(uint32_t width, uint32_t height, const float* variance, float target, uint32_t max_level, uint8_t* out_levels) {
    const char* who = "mc_pathtrace_budget_levels";
    if (int rc = pt_budget_check_size(width, height, who)) return rc;
    if (int rc = pt_budget_check(target, max_level, who)) return rc;
    if (!variance || !out_levels) return refuse(who, "a plane is NULL");
    const size_t npix = (size_t)width * height;
    const float tau2 = target * target;
    for (size_t q = 0; q < npix; q++) out_levels[q] = ptd::budget_level(variance[q], tau2, max_level);
    return MC_OK;
}

int mc_pathtrace_budget_resolve(uint32_t width, uint32_t height, const float* acc, const uint8_t* levels, float* out) {
    const char* who = "mc_pathtrace_budget_resolve";
    if (int rc = pt_budget_check_size(width, height, who)) return rc;
    if (!acc || !levels || !out) return refuse(who, "a plane is NULL");
    const size_t npix = (size_t)width * height;
    std::vector<vec4> s_acc;
    const vec4* a = aligned_in(acc, npix, s_acc);
    AlignedOut o(out, npix);
    vec4* dst = o.ptr();
    for (size_t q = 0; q < npix; q++) dst[q] = ptd::budget_resolve(a[q], levels[q]);
    o.finish();
    return MC_OK;
}

int mc_pathtrace_budget_levels_device_async(mc_context* ctx, uint32_t width, uint32_t height, const void* d_variance, float target,
                                            uint32_t max_level, void* d_levels, void* stream) {
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    MC_HIP_TRY(hipSetDevice(ctx->device));
    return pt_budget_levels_launch(ctx, width, height, d_variance, target, max_level, d_levels, "mc_pathtrace_budget_levels_device_async",
                                   stream ? (hipStream_t)stream : ctx->stream);
}

int mc_pathtrace_budget_lists_device_async(mc_context* ctx, uint32_t width, uint32_t height, const void* d_levels, uint32_t max_level,
                                           void* d_list, void* d_counts, void* stream) {
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    MC_HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = ctx->scratch_iters.reserve(kBudgetCountsBytes)) return rc;
    return pt_budget_lists_launch(ctx, width, height, d_levels, max_level, d_list, d_counts, ctx->scratch_iters.ptr,
                                  "mc_pathtrace_budget_lists_device_async", stream ? (hipStream_t)stream : ctx->stream);
}

int mc_pathtrace_budget_resolve_device_async(mc_context* ctx, uint32_t width, uint32_t height, const void* d_acc, const void* d_levels,
                                             void* d_out, void* stream) {
    const char* who = "mc_pathtrace_budget_resolve_device_async";
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    if (!d_levels) return refuse(who, "a plane is NULL");
    MC_HIP_TRY(hipSetDevice(ctx->device));
    return pt_budget_resolve_launch(ctx, width, height, d_acc, d_levels, d_out, who, stream ? (hipStream_t)stream : ctx->stream);
}

int mc_pathtrace_render_list_device_async(mc_context* ctx, const mc_pathtrace_params* p, const float* planes, uint32_t n_planes,
                                          const float* spheres, uint32_t n_spheres, const void* d_list, uint32_t n_list, float prescale,
                                          void* d_acc, void* stream) {
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    MC_HIP_TRY(hipSetDevice(ctx->device));
    return pt_budget_list_render(ctx, p, planes, n_planes, spheres, n_spheres, d_list, n_list, prescale, d_acc,
                                 "mc_pathtrace_render_list_device_async", stream ? (hipStream_t)stream : ctx->stream);
}

int mc_context_last_budget(mc_context* ctx, uint64_t per_level[9], double* mean_spp) {
    if (!ctx || !ctx->budget.valid) return MC_ERR_INVALID_ARGUMENT;
    if (per_level) for (int k = 0; k < 9; k++) per_level[k] = ctx->budget.per_level[k];
    if (mean_spp) *mean_spp = ctx->budget.mean_spp;
    return MC_OK;
}

}  // extern "C"
