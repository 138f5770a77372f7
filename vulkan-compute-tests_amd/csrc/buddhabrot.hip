// Buddhabrot for gfx950 (MI355X): the orbit-density plane by scattered integer atomics, and its tone-map gather.
// The project's own addition; contract in include/mc_compute.h, restated in tests/buddhabrot_ref.py; sizing, the two forms below, their
// resource usage and the measurements that chose between them in DESIGN.md §3.26.  The arithmetic of a sample is buddhabrot.h's, the
// text the host call compiles too.
//
//  * plain form (MC_BUDDHA_KERNEL_PLAIN): one sample per lane, a grid-stride loop over k: skip test, classify, replay.  A wave waits
//    for its longest orbit in each loop, twice per trip.
//  * pooled form (MC_BUDDHA_KERNEL_POOLED): each wave owns a contiguous run of sample indices.  A lane whose sample is finished
//    (skipped, never escaped, fully plotted) takes the run's next index through a ballot and a prefix count — the plane cannot depend
//    on the assignment, so scheduling needs no atomics.  ONE loop body serves both phases: the fp64 step, then the escape test while
//    classifying or the bin and the add while plotting, so lanes in different phases share the step's issue slots.  A wave refills once
//    kPoolRefillLanes of its lanes are idle: the refill's hash and interior test are issued for the whole wave however few lanes take
//    a sample.  The default form: 2.7 and 5.5 times the plain form's rate on the two gate configurations.
//  * the add is a relaxed, agent-scope atomic whose result is unused (global_atomic_add_u32 without return); integer adds commute, so the
//    plane is bit-reproducible whatever the schedule.  Statistics are reduced per wave, then per block in LDS, and added once per block.
//  * the importance map and the guided samples are template parameters of the two forms, not further kernels.
//  Vector atomics and vector stores only.
#include <cstring>

#include "buddhabrot.h"
#include "mandel_side_record.h"
#include "mc_internal.h"

namespace mc {

namespace {

using buddha::Args;

constexpr uint32_t kBlock = 256, kWavesPerBlock = kBlock / 64;
constexpr uint32_t kBlocksPerCu = 8;       // 8 waves per SIMD: the scattered adds' latency is hidden by other waves' fp64 steps
constexpr uint64_t kPoolMinRun = 512;      // samples a pooled wave owns at least (eight refills of its 64 lanes)
// Idle lanes a pooled wave waits for before it refills (the refill's hash, window and interior test are issued for the whole wave
// whatever the number of lanes that take a sample; DESIGN.md §3.26 has the measured sweep behind the value).
#ifndef MC_BUDDHA_REFILL_LANES
#define MC_BUDDHA_REFILL_LANES 16
#endif
constexpr uint32_t kPoolRefillLanes = MC_BUDDHA_REFILL_LANES;

__device__ __forceinline__ void plane_add(uint32_t* plane, uint32_t bin, uint32_t v) {
    (void)__hip_atomic_fetch_add(plane + bin, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The three things a launch can be, as template parameters of both forms: kMap, the importance call, adds a sample's
// added count to its cell's map word at the end of its plot phase; kPlane false, the pilot's normal use, issues no plane add and still
// counts `added`; kGuided takes the sample's cell from the list and adds gd.weight per point.  <false, true, false> is the uniform call,
// whose instructions are what they were before the parameters existed.

// (base + off) mod n for base < n and off <= 64: a guided wave's k mod n_cells moves by increments, never by a 64-bit division.
__device__ __forceinline__ uint32_t add_mod(uint32_t base, uint32_t off, uint32_t n) {
    const uint64_t t = (uint64_t)base + off;
    if (n > 64u) return (uint32_t)(t >= n ? t - n : t);
    return (uint32_t)t % n;   // t < 128
}
// Sample k's c (and, for the map, its cell): the uniform hash, or the hash's high bits inside cell cells[j] of the list.  A list entry
// beyond the grid is the caller's broken precondition; it is clamped, so the words stay what a cell of the grid gives.
template <bool kMap, bool kGuided>
__device__ __forceinline__ void take_sample(const Args& a, const buddha::Guide& gd, uint64_t k, uint32_t j, double& cx, double& cy,
                                            uint32_t& cell) {
    if constexpr (!kMap && !kGuided) {
        buddha::sample_c(a, k, cx, cy);
    } else {
        uint32_t ux, uy;
        buddha::hash_words(a.seed, k, ux, uy);
        if constexpr (kGuided) {
            const uint32_t top = (1u << (2u * gd.g)) - 1u, c = gd.cells[j];
            buddha::guided_words(c > top ? top : c, gd.g, ux, uy);
        }
        if constexpr (kMap) cell = buddha::cell_of(ux, uy, gd.g);
        buddha::c_of_words(a, ux, uy, cx, cy);
    }
}

// The five per-lane counts of a block into d_stats: a wave sum by shuffles, the block's in LDS, one global add per field and block.
__device__ __forceinline__ void stats_flush(uint64_t* __restrict__ d_stats, uint64_t (&st)[buddha::kStats]) {
    __shared__ unsigned long long block_sum[buddha::kStats];
    if (threadIdx.x < buddha::kStats) block_sum[threadIdx.x] = 0ull;
    __syncthreads();
#pragma unroll
    for (int f = 0; f < buddha::kStats; f++) {
        unsigned long long v = st[f];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63u) == 0u && v) atomicAdd(&block_sum[f], v);
    }
    __syncthreads();
    if (d_stats && threadIdx.x < buddha::kStats && block_sum[threadIdx.x])
        atomicAdd(reinterpret_cast<unsigned long long*>(d_stats) + threadIdx.x, block_sum[threadIdx.x]);
}

template <bool kMap, bool kPlane, bool kGuided>
__global__ void __launch_bounds__(kBlock) buddhabrot_plain_kernel(Args a, buddha::Guide gd, uint32_t* __restrict__ plane,
                                                                  uint64_t* __restrict__ d_stats) {
    uint64_t st[buddha::kStats] = {0, 0, 0, 0, 0};
    const uint64_t samples = a.end - a.begin, stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t first = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    // guided: j = k mod n_cells by one 64-bit division per lane, then steps of stride mod n_cells
    uint32_t j = 0, j_step = 0, cell = 0;
    if constexpr (kGuided) {
        j = (uint32_t)((a.begin + first) % gd.n_cells);
        j_step = (uint32_t)(stride % gd.n_cells);
    }
    for (uint64_t at = first; at < samples; at += stride) {   // (at < 2^40: no wrap near k = 2^64)
        const uint64_t k = a.begin + at;
        st[buddha::kSamples]++;
        double cx, cy;
        take_sample<kMap, kGuided>(a, gd, k, j, cx, cy, cell);
        if constexpr (kGuided) {
            const uint64_t t = (uint64_t)j + j_step;
            j = (uint32_t)(t >= gd.n_cells ? t - gd.n_cells : t);
        }
        if (buddha::interior(cx, cy)) {
            st[buddha::kSkipped]++;
            continue;
        }
        buddha::Orbit o;
        o.reset();
        uint32_t n = a.max_iter;   // max_iter: did not escape
        for (uint32_t i = 0; i < a.max_iter; i++)
            if (o.advance(cx, cy) > 4.0) {
                n = i;
                break;
            }
        if (n == a.max_iter || n < a.min_iter) continue;
        st[buddha::kContributing]++;
        st[buddha::kPoints] += n;
        o.reset();
        uint32_t added = 0;
        for (uint32_t i = 0; i < n; i++) {
            o.advance(cx, cy);
            uint32_t bin;
            if (buddha::bin_of(a, o.zx, o.zy, bin)) {
                if constexpr (kPlane) plane_add(plane, bin, kGuided ? gd.weight : 1u);
                added++;
            }
        }
        st[buddha::kAdded] += added;
        if constexpr (kMap)
            if (added) plane_add(gd.map, cell, added);
    }
    stats_flush(d_stats, st);
}

// run: the samples each wave owns (the last waves' runs end at a.end, or are empty).
// The importance and guided instantiations ask for 8 waves per SIMD: left alone they take 65 and 66 VGPRs, one wave fewer than the
// uniform call's 63; asked, the allocator gives 46 to 52 without scratch.  The uniform instantiation is not asked and keeps its code.
template <bool kMap, bool kPlane, bool kGuided>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu((kMap || kGuided) ? 8 : 1, 8))) buddhabrot_pooled_kernel(Args a, buddha::Guide gd, uint64_t run, uint32_t* __restrict__ plane,
                                                                   uint64_t* __restrict__ d_stats) {
    enum : uint32_t { kIdle = 0, kClassify = 1, kPlot = 2 };
    uint64_t st[buddha::kStats] = {0, 0, 0, 0, 0};
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    // offsets from a.begin, all below 2^41 (run * waves < 2^40 + waves): nothing wraps however close to 2^64 the indices lie
    const uint64_t samples = a.end - a.begin;
    uint64_t next = wave * run < samples ? wave * run : samples;
    const uint64_t last = samples - next < run ? samples : next + run;
    const uint64_t below = lane ? (~0ull >> (64u - lane)) : 0ull;   // the lanes in front of this one

    double cx = 0.0, cy = 0.0;
    buddha::Orbit o;
    o.reset();
    uint32_t phase = kIdle, i = 0, n = 0, added = 0;
    // importance: the lane keeps its sample's cell (not k) across the orbit.  guided: next_j = (a.begin + next) mod n_cells, wave-uniform,
    // one 64-bit division per run; a run is contiguous in k, so every refill moves it by the lanes taken
    uint32_t cell = 0, next_j = 0;
    if constexpr (kGuided) next_j = (uint32_t)((a.begin + next) % gd.n_cells);
    for (;;) {
        // refill, once kPoolRefillLanes lanes are idle (or all of them): every idle lane takes the run's next index, in lane order,
        // until no lane is idle or the run is used up
        for (bool started = false;; started = true) {
            const unsigned long long idle = __ballot(phase == kIdle);
            if (!idle || next >= last) break;                                                            // wave-uniform, as the next
            if (!started && (uint32_t)__popcll(idle) < kPoolRefillLanes && idle != ~0ull) break;
            const uint32_t ahead = (uint32_t)__popcll(idle & below);
            const uint64_t at = next + (uint64_t)ahead;
            if (phase == kIdle && at < last) {
                st[buddha::kSamples]++;
                take_sample<kMap, kGuided>(a, gd, a.begin + at, kGuided ? add_mod(next_j, ahead, gd.n_cells) : 0u, cx, cy, cell);
                if (buddha::interior(cx, cy)) {
                    st[buddha::kSkipped]++;
                } else {
                    phase = kClassify;
                    o.reset();
                    i = 0;
                }
            }
            const uint64_t take = (uint64_t)__popcll(idle);
            next = last - next < take ? last : next + take;
            if constexpr (kGuided) next_j = add_mod(next_j, (uint32_t)take, gd.n_cells);
        }
        if (!__ballot(phase != kIdle)) break;   // the run is used up and every lane has finished: wave-uniform
        if (phase != kIdle) {
            const double r2 = o.advance(cx, cy);
            if (phase == kClassify) {
                if (r2 > 4.0) {   // escaped after i iterations
                    if (i >= a.min_iter) {
                        st[buddha::kContributing]++;
                        st[buddha::kPoints] += i;
                    }
                    if (i >= a.min_iter && i > 0u) {
                        phase = kPlot;
                        n = i;
                        i = 0;
                        added = 0;
                        o.reset();
                    } else {
                        phase = kIdle;
                    }
                } else if (++i == a.max_iter) {
                    phase = kIdle;   // never escaped
                }
            } else {   // z is z_(i+1) of the n points
                uint32_t bin;
                if (buddha::bin_of(a, o.zx, o.zy, bin)) {
                    if constexpr (kPlane) plane_add(plane, bin, kGuided ? gd.weight : 1u);
                    added++;
                }
                if (++i == n) {
                    st[buddha::kAdded] += added;
                    if constexpr (kMap)
                        if (added) plane_add(gd.map, cell, added);
                    phase = kIdle;
                }
            }
        }
    }
    stats_flush(d_stats, st);
}

// rgba[i] = (table[d0[i]'], table[E + d1[i]'], table[2 E + d2[i]'], 1), d' = min(d, L), E = L + 1: three gathers per pixel from the
// quotients the host formed (buddhabrot_tone_table), 12 B read + 16 B written, one pixel per lane.
__global__ void __launch_bounds__(256) buddhabrot_tonemap_kernel(const uint32_t* __restrict__ d0, const uint32_t* __restrict__ d1,
                                                                 const uint32_t* __restrict__ d2, const float* __restrict__ table,
                                                                 uint32_t levels, uint64_t total, float4* __restrict__ rgba) {
    const uint64_t entries = (uint64_t)levels + 1u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t a = d0[i], b = d1[i], c = d2[i];
        rgba[i] = make_float4(table[a > levels ? levels : a], table[entries + (b > levels ? levels : b)],
                              table[2u * entries + (c > levels ? levels : c)], 1.0f);
    }
}

// The device state of the feature, a side record of the context (mandel_side_record.h).
struct BuddhaState {
    DeviceBuffer plane, stats;          // mc_buddhabrot_render's
    DeviceBuffer table;                 // the tone map's quotients, 3 (levels + 1) floats: a cached device table like the colour LUT
    std::vector<uint32_t> table_maps;   // what `table` was formed from: m0 | m1 | m2
    uint32_t table_levels = 0;
    DeviceBuffer map, cells, guide_stats;   // mc_buddhabrot_render_guided's map, cell lists and the statistics of its three passes
};
SideRecords<BuddhaState> g_buddha_states;

}  // namespace

void buddhabrot_release(mc_context* ctx) {
    g_buddha_states.erase(ctx, [](BuddhaState& st) {
        st.plane.release();
        st.stats.release();
        st.table.release();
        st.map.release();
        st.cells.release();
        st.guide_stats.release();
    });
}

namespace {

// One launch of either form in one of its instantiations; the grid is the uniform call's whatever the instantiation.
template <bool kMap, bool kPlane, bool kGuided>
int launch_as(mc_context* ctx, const mc_buddhabrot_params* p, const buddha::Guide& gd, void* d_plane, void* d_stats, hipStream_t s) {
    const Args a = buddha::make_args(p);
    const uint64_t samples = a.end - a.begin;
    if (!samples) return MC_OK;
    const uint64_t cap = (uint64_t)ctx->props.multiProcessorCount * kBlocksPerCu;
    const bool plain = (p->flags & MC_BUDDHA_KERNEL_PLAIN) != 0u;   // neither bit: the pooled form
    if (plain) {
        uint64_t blocks = (samples + kBlock - 1u) / kBlock;
        if (blocks > cap) blocks = cap;
        hipLaunchKernelGGL((buddhabrot_plain_kernel<kMap, kPlane, kGuided>), dim3((uint32_t)blocks), dim3(kBlock), 0, s, a, gd,
                           (uint32_t*)d_plane, (uint64_t*)d_stats);
    } else {
        const uint64_t per_block = kPoolMinRun * kWavesPerBlock;
        uint64_t blocks = (samples + per_block - 1u) / per_block;
        if (blocks > cap) blocks = cap;
        const uint64_t waves = blocks * kWavesPerBlock;
        const uint64_t run = (samples + waves - 1u) / waves;
        hipLaunchKernelGGL((buddhabrot_pooled_kernel<kMap, kPlane, kGuided>), dim3((uint32_t)blocks), dim3(kBlock), 0, s, a, gd, run,
                           (uint32_t*)d_plane, (uint64_t*)d_stats);
    }
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

// What every device form checks of its pointers: a plane (when required or given) and the statistics, aligned.
int check_device_pointers(mc_context* ctx, void* d_plane, bool plane_required, void* d_stats, const char* who) {
    if (!ctx || (plane_required && !d_plane)) {
        set_error_detail(std::string(who) + ": ctx or d_plane is NULL");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (reinterpret_cast<uintptr_t>(d_plane) % 4u || reinterpret_cast<uintptr_t>(d_stats) % 8u) {
        set_error_detail(std::string(who) + ": d_plane must be 4-byte aligned, d_stats 8-byte aligned");
        return MC_ERR_INVALID_ARGUMENT;
    }
    return MC_OK;
}

}  // namespace

int buddhabrot_launch(mc_context* ctx, const mc_buddhabrot_params* p, void* d_plane, void* d_stats, hipStream_t s) {
    const char* who = "mc_buddhabrot_density_device_async";
    if (int rc = buddhabrot_check(p, who)) return rc;
    if (int rc = check_device_pointers(ctx, d_plane, true, d_stats, who)) return rc;
    return launch_as<false, true, false>(ctx, p, buddha::Guide{}, d_plane, d_stats, s);
}

int buddhabrot_importance_launch(mc_context* ctx, const mc_buddhabrot_params* p, uint32_t grid_log2, void* d_map, void* d_plane,
                                 void* d_stats, hipStream_t s) {
    const char* who = "mc_buddhabrot_importance_device_async";
    if (int rc = buddhabrot_check(p, who)) return rc;
    if (int rc = buddhabrot_check_grid(grid_log2, who)) return rc;
    if (int rc = check_device_pointers(ctx, d_plane, false, d_stats, who)) return rc;
    if (!d_map || reinterpret_cast<uintptr_t>(d_map) % 4u) {
        set_error_detail(std::string(who) + ": d_map is NULL or not 4-byte aligned");
        return MC_ERR_INVALID_ARGUMENT;
    }
    buddha::Guide gd{};
    gd.map = (uint32_t*)d_map;
    gd.g = grid_log2;
    return d_plane ? launch_as<true, true, false>(ctx, p, gd, d_plane, d_stats, s)
                   : launch_as<true, false, false>(ctx, p, gd, nullptr, d_stats, s);
}

int buddhabrot_guided_launch(mc_context* ctx, const mc_buddhabrot_params* p, const void* d_cells, uint32_t n_cells, uint32_t grid_log2,
                             uint32_t weight, void* d_plane, void* d_stats, hipStream_t s) {
    const char* who = "mc_buddhabrot_density_guided_device_async";
    if (int rc = buddhabrot_check(p, who)) return rc;
    if (int rc = buddhabrot_check_cell_list((const uint32_t*)d_cells, n_cells, grid_log2, weight, false, who)) return rc;
    if (int rc = check_device_pointers(ctx, d_plane, true, d_stats, who)) return rc;
    if (reinterpret_cast<uintptr_t>(d_cells) % 4u) {
        set_error_detail(std::string(who) + ": d_cells must be 4-byte aligned");
        return MC_ERR_INVALID_ARGUMENT;
    }
    buddha::Guide gd{};
    gd.cells = (const uint32_t*)d_cells;
    gd.n_cells = n_cells;
    gd.g = grid_log2;
    gd.weight = weight;
    return launch_as<false, true, true>(ctx, p, gd, d_plane, d_stats, s);
}

int buddhabrot_guide_buffers(mc_context* ctx, uint32_t grid_log2, void** d_map, void** d_cells, void** d_stats3) {
    BuddhaState* st = g_buddha_states.get(ctx);
    const size_t words = (size_t)1 << (2u * grid_log2);
    int rc;
    if ((rc = st->map.reserve(words * 4)) || (rc = st->cells.reserve(words * 4)) || (rc = st->guide_stats.reserve(3 * buddha::kStats * 8)))
        return rc;
    *d_map = st->map.ptr;
    *d_cells = st->cells.ptr;
    *d_stats3 = st->guide_stats.ptr;
    return MC_OK;
}

int buddhabrot_render_buffers(mc_context* ctx, const mc_buddhabrot_params* p, void** d_plane, void** d_stats) {
    BuddhaState* st = g_buddha_states.get(ctx);
    int rc;
    if ((rc = st->plane.reserve((size_t)p->width * p->height * 4)) || (rc = st->stats.reserve(buddha::kStats * 8))) return rc;
    *d_plane = st->plane.ptr;
    *d_stats = st->stats.ptr;
    return MC_OK;
}

int buddhabrot_tonemap_launch(mc_context* ctx, uint32_t width, uint32_t height, const void* d0, const void* d1, const void* d2,
                              uint32_t levels, const uint32_t* m0, const uint32_t* m1, const uint32_t* m2, void* d_rgba, hipStream_t s) {
    const char* who = "mc_buddhabrot_tonemap_device_async";
    if (!ctx || !d0 || !d1 || !d2 || !m0 || !m1 || !m2 || !d_rgba) {
        set_error_detail(std::string(who) + ": a pointer is NULL");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (!width || !height || (uint64_t)width * height > 0xffffffffull) {
        set_error_detail(std::string(who) + ": width or height is 0, or width * height exceeds 2^32 - 1");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (int rc = buddhabrot_check_levels(levels, who)) return rc;
    if (int rc = buddhabrot_check_maps(levels, m0, m1, m2, who)) return rc;
    BuddhaState* st = g_buddha_states.get(ctx);
    const size_t entries = (size_t)levels + 1;
    const uint32_t* maps[3] = {m0, m1, m2};
    bool cached = st->table.ptr && st->table_levels == levels && st->table_maps.size() == 3 * entries;
    for (int c = 0; cached && c < 3; c++) cached = std::memcmp(st->table_maps.data() + c * entries, maps[c], entries * 4) == 0;
    if (!cached) {
        std::vector<float> table(3 * entries);
        buddhabrot_tone_table(levels, m0, m1, m2, table.data());
        // an earlier tone map of this context may still read the old table (possibly on another stream): wait for the streams this
        // context has launched on before replacing it, as the colour tables do
        int rc = ctx->drain_launch_streams();
        if (rc) return rc;
        st->table_maps.clear();   // unusable until the copy below has completed
        if ((rc = st->table.reserve(3 * entries * 4))) return rc;
        MC_HIP_TRY(hipMemcpyAsync(st->table.ptr, table.data(), 3 * entries * 4, hipMemcpyHostToDevice, s));
        MC_HIP_TRY(hipStreamSynchronize(s));   // the host vector goes out of scope
        st->table_maps.resize(3 * entries);
        for (int c = 0; c < 3; c++) std::memcpy(st->table_maps.data() + c * entries, maps[c], entries * 4);
        st->table_levels = levels;
    }
    const uint64_t total = (uint64_t)width * height;
    uint64_t blocks = (total + 255u) / 256u;
    const uint64_t cap = (uint64_t)ctx->props.multiProcessorCount * 8u;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(buddhabrot_tonemap_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, (const uint32_t*)d0, (const uint32_t*)d1,
                       (const uint32_t*)d2, (const float*)st->table.ptr, levels, total, (float4*)d_rgba);
    MC_HIP_TRY(hipGetLastError());
    return ctx->note_launch(s);   // (reads the cached table)
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_buddhabrot_density_device_async(mc_context* ctx, const mc_buddhabrot_params* p, void* d_plane, void* d_stats, void* stream) {
    if (!ctx) {
        set_error_detail("mc_buddhabrot_density_device_async: ctx is NULL");
        return MC_ERR_INVALID_ARGUMENT;
    }
    MC_HIP_TRY(hipSetDevice(ctx->device));
    return buddhabrot_launch(ctx, p, d_plane, d_stats, stream ? (hipStream_t)stream : ctx->stream);
}

int mc_buddhabrot_importance_device_async(mc_context* ctx, const mc_buddhabrot_params* p, uint32_t grid_log2, void* d_map, void* d_plane,
                                          void* d_stats, void* stream) {
    if (!ctx) {
        set_error_detail("mc_buddhabrot_importance_device_async: ctx is NULL");
        return MC_ERR_INVALID_ARGUMENT;
    }
    MC_HIP_TRY(hipSetDevice(ctx->device));
    return buddhabrot_importance_launch(ctx, p, grid_log2, d_map, d_plane, d_stats, stream ? (hipStream_t)stream : ctx->stream);
}

int mc_buddhabrot_density_guided_device_async(mc_context* ctx, const mc_buddhabrot_params* p, const void* d_cells, uint32_t n_cells,
                                              uint32_t grid_log2, uint32_t weight, void* d_plane, void* d_stats, void* stream) {
    if (!ctx) {
        set_error_detail("mc_buddhabrot_density_guided_device_async: ctx is NULL");
        return MC_ERR_INVALID_ARGUMENT;
    }
    MC_HIP_TRY(hipSetDevice(ctx->device));
    return buddhabrot_guided_launch(ctx, p, d_cells, n_cells, grid_log2, weight, d_plane, d_stats, stream ? (hipStream_t)stream : ctx->stream);
}

int mc_buddhabrot_tonemap_device_async(mc_context* ctx, uint32_t width, uint32_t height, const void* d0, const void* d1, const void* d2,
                                       uint32_t levels, const uint32_t* m0, const uint32_t* m1, const uint32_t* m2, void* d_rgba_f32,
                                       void* stream) {
    if (!ctx) {
        set_error_detail("mc_buddhabrot_tonemap_device_async: ctx is NULL");
        return MC_ERR_INVALID_ARGUMENT;
    }
    MC_HIP_TRY(hipSetDevice(ctx->device));
    return buddhabrot_tonemap_launch(ctx, width, height, d0, d1, d2, levels, m0, m1, m2, d_rgba_f32, stream ? (hipStream_t)stream : ctx->stream);
}

}  // extern "C"
