// Atom domains on gfx950 (MI355X): the entry points of the period plane (its kernels are the atom instantiations of mandel_kernels.h, in
// mandelbrot.hip and mandel_perturb.hip) and the domains of a plane.  Contract in include/mc_compute.h ("atom domains"), restated in
// tests/mandel_atom_ref.py; scheme and measurements in DESIGN.md §3.33.
//
// The domains of a plane are three tables over the periods v in [0, max_iter]:
//  * count[v]: mc_mandelbrot_histogram_device_async's histogram of the period plane (mandel_histogram.hip), reused as it is.
//  * amin[v]: a non-negative double's bit pattern orders as a uint64_t, so pass 1 is a 64-bit atomic min per period at agent scope.  Lanes of
//    a wave that hold the same period are combined first, by hist::wave_combine_add's election (the lowest pending lane leads, the lanes
//    holding its period are balloted) with a wave-wide min of their keys in place of the population count: a plane of one period costs one
//    atomic per wave.  The table only ever falls, so a plain load that already shows a value no larger than the key proves the atomic
//    would change nothing, and it is skipped.
//  * pixel[v]: pass 2, a 32-bit atomic min of the linear index by the pixels whose amin equals their period's minimum.
// Min and add commute: the tables are bit-reproducible whatever the arrival order.  Vector atomics and vector stores only.
#include <algorithm>

#include "mandel_atom.h"
#include "mandel_equalise.h"
#include "mandel_histogram_kernel.h"
#include "mc_internal.h"

namespace mc {

namespace {

constexpr uint32_t kDomainBlocksPerCu = 8u;   // the grid cap: blocks of 256 lanes per CU; the loops below stride over the rest

__global__ void __launch_bounds__(256) atom_domains_init_kernel(uint32_t entries, uint32_t* __restrict__ count, uint64_t* __restrict__ amin,
                                                                uint32_t* __restrict__ pixel) {
    for (uint32_t v = blockIdx.x * 256u + threadIdx.x; v < entries; v += gridDim.x * 256u) {
        count[v] = 0u;
        amin[v] = atom::kInfBits;
        pixel[v] = atom::kNoPixel;
    }
}

// The smallest key of the wave's lanes (every lane gets it).  Six butterfly steps on 64-bit words.
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t k) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)k, d, 64);
        k = o < k ? o : k;
    }
    return k;
}

__device__ __forceinline__ void table_min(uint64_t* tab, uint32_t v, uint64_t key) {
    if (key < __hip_atomic_load(tab + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        (void)__hip_atomic_fetch_min(tab + v, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Pass 1.  One pixel per lane and trip; a wave's trip count is the same for all its lanes (the ballots and butterflies see whole waves).
// pending: the lane holds a pixel whose period is in the table and whose key can be a minimum (at most +inf's pattern).
__global__ void __launch_bounds__(256) atom_domains_min_kernel(const uint32_t* __restrict__ period, const uint64_t* __restrict__ amin,
                                                               uint64_t n, uint32_t max_iter, uint64_t* __restrict__ tab) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t base = (uint64_t)blockIdx.x * 256u + (threadIdx.x & ~63u); base < n; base += stride) {
        const uint64_t i = base + lane;
        uint32_t v = 0u;
        uint64_t key = ~0ull;
        if (i < n) { v = period[i]; key = amin[i]; }
        bool pending = i < n && v <= max_iter && key <= atom::kInfBits;
#pragma unroll
        for (int r = 0; r < hist::kCombineRounds; r++) {
            const unsigned long long act = __ballot(pending);
            if (!act) break;   // wave-uniform
            const uint32_t leader = (uint32_t)__ffsll((long long)act) - 1u;
            const uint32_t lv = (uint32_t)__builtin_amdgcn_readlane((int)v, (int)leader);
            const bool mine = pending && v == lv;
            const uint64_t low = wave_min_u64(mine ? key : ~0ull);
            if (lane == leader) table_min(tab, lv, low);
            pending = pending && !mine;
        }
        if (pending) table_min(tab, v, key);   // (periods spread over more than kCombineRounds values in this wave)
    }
}

// Pass 2, after pass 1 has completed: the pixels attaining their period's minimum.
__global__ void __launch_bounds__(256) atom_domains_arg_kernel(const uint32_t* __restrict__ period, const uint64_t* __restrict__ amin,
                                                               uint64_t n, uint32_t max_iter, const uint64_t* __restrict__ tab,
                                                               uint32_t* __restrict__ pixel) {
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride) {
        const uint32_t v = period[i];
        if (v > max_iter) continue;
        if (amin[i] != tab[v]) continue;
        const uint32_t idx = (uint32_t)i;
        if (idx < __hip_atomic_load(pixel + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            (void)__hip_atomic_fetch_min(pixel + v, idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace

// (mandelbrot_histogram_launch: mandel_histogram.hip, declared in mandel_equalise.h)
int atom_domains_launch(mc_context* ctx, const void* d_period, const void* d_amin, uint64_t n_pixels, uint32_t max_iter, void* d_count,
                        void* d_amin_table, void* d_pixel, hipStream_t s) {
    const std::string fn = "mc_mandelbrot_atom_domains_device_async";
    auto refuse = [&](const std::string& why) {
        set_error_detail(fn + ": " + why);
        return (int)MC_ERR_INVALID_ARGUMENT;
    };
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    if (!d_period || !d_amin || !d_count || !d_amin_table || !d_pixel) return refuse("NULL argument");
    if (n_pixels > 0xffffffffull) return refuse("pixel indices are uint32_t: n_pixels must stay below 2^32");
    if (!max_iter || max_iter == 0xffffffffu) return refuse("max_iter must be in [1, 2^32 - 2]");
    if (reinterpret_cast<uintptr_t>(d_period) % 4u || reinterpret_cast<uintptr_t>(d_count) % 4u || reinterpret_cast<uintptr_t>(d_pixel) % 4u ||
        reinterpret_cast<uintptr_t>(d_amin) % 8u || reinterpret_cast<uintptr_t>(d_amin_table) % 8u)
        return refuse("a plane or table is not aligned to its element size");
    const uint32_t entries = max_iter + 1u;
    const uint32_t cap = (uint32_t)ctx->props.multiProcessorCount * kDomainBlocksPerCu;
    const uint32_t init_blocks = std::min<uint32_t>(cap, (entries + 255u) / 256u);
    hipLaunchKernelGGL(atom_domains_init_kernel, dim3(init_blocks), dim3(256), 0, s, entries, (uint32_t*)d_count, (uint64_t*)d_amin_table,
                       (uint32_t*)d_pixel);
    MC_HIP_TRY(hipGetLastError());
    if (!n_pixels) return MC_OK;
    if (int rc = mandelbrot_histogram_launch(ctx, d_period, 4u, n_pixels, max_iter, d_count, s)) return rc;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(cap, (n_pixels + 255u) / 256u);
    hipLaunchKernelGGL(atom_domains_min_kernel, dim3(blocks), dim3(256), 0, s, (const uint32_t*)d_period, (const uint64_t*)d_amin, n_pixels,
                       max_iter, (uint64_t*)d_amin_table);
    MC_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(atom_domains_arg_kernel, dim3(blocks), dim3(256), 0, s, (const uint32_t*)d_period, (const uint64_t*)d_amin, n_pixels,
                       max_iter, (const uint64_t*)d_amin_table, (uint32_t*)d_pixel);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_mandelbrot_render_atom_device_async(mc_context* ctx, const mc_mandelbrot_params* p, void* d_iters, void* d_period, void* d_amin,
                                           void* stream) {
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    MC_HIP_TRY(hipSetDevice(ctx->device));
    return mandelbrot_atom_launch(ctx, p, d_iters, d_period, d_amin, stream ? (hipStream_t)stream : ctx->stream);
}

// Blocking, on the context's stream.  The three planes live in the context's count scratch: amin | n | period, each on a 256-byte boundary.
int mc_mandelbrot_render_atom(mc_context* ctx, const mc_mandelbrot_params* p, uint32_t* out_iters, uint32_t* out_period, double* out_amin) {
    if (!ctx || !p) return MC_ERR_INVALID_ARGUMENT;
    MC_HIP_TRY(hipSetDevice(ctx->device));
    const size_t npix = (size_t)p->width * p->height;
    auto plane = [](size_t bytes) { return (bytes + 255u) & ~(size_t)255u; };
    const size_t off_n = plane(npix * 8u), off_p = off_n + plane(npix * 4u), total = off_p + plane(npix * 4u);
    if (!npix) return mandelbrot_atom_launch(ctx, p, out_iters, out_period, out_amin, ctx->stream);   // (refused there: nothing is launched)
    if (out_iters || out_period || out_amin)
        if (int rc = ctx->scratch_iters.reserve(total)) return rc;
    char* base = (char*)ctx->scratch_iters.ptr;
    void* d_a = out_amin ? base : nullptr;
    void* d_n = out_iters ? base + off_n : nullptr;
    void* d_p = out_period ? base + off_p : nullptr;
    if (int rc = mandelbrot_atom_launch(ctx, p, d_n, d_p, d_a, ctx->stream)) return rc;
    if (d_a) MC_HIP_TRY(hipMemcpyAsync(out_amin, d_a, npix * 8u, hipMemcpyDeviceToHost, ctx->stream));
    if (d_n) MC_HIP_TRY(hipMemcpyAsync(out_iters, d_n, npix * 4u, hipMemcpyDeviceToHost, ctx->stream));
    if (d_p) MC_HIP_TRY(hipMemcpyAsync(out_period, d_p, npix * 4u, hipMemcpyDeviceToHost, ctx->stream));
    MC_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MC_OK;
}

int mc_mandelbrot_atom_domains_device_async(mc_context* ctx, const void* d_period, const void* d_amin, uint64_t n_pixels, uint32_t max_iter,
                                            void* d_count, void* d_amin_table, void* d_pixel, void* stream) {
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    MC_HIP_TRY(hipSetDevice(ctx->device));
    return atom_domains_launch(ctx, d_period, d_amin, n_pixels, max_iter, d_count, d_amin_table, d_pixel, stream ? (hipStream_t)stream : ctx->stream);
}

}  // extern "C"
