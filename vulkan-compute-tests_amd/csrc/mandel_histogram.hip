// Histogram-equalised Mandelbrot colouring for gfx950 (MI355X): the histogram of a count plane, the rank map, the recolouring.
// The project's own addition (the reference colours by t = n / M only, mandelbrot.comp:50-56); contract in include/mc_compute.h,
// restated in tests/mandel_equalise_ref.py; scheme and measurements in DESIGN.md §3.10.
//
// The histogram kernel (the hot path: 2 or 4 B read per pixel, nothing written but the table):
//  * every lane reads 16 B (4 uint32_t or 8 uint16_t counts) per trip of a grid-stride loop; the grid is sized from the CU count.
//    The plane's unaligned head and its tail (fewer than 16 B each) are counted one value per lane by block 0.
//  * the input is as skewed as a histogram's gets: interior regions are thousands of adjacent pixels with n = M, a deep frame's
//    escaped pixels share a few hundred values.  So lanes combine inside the wave before anything reaches the table:
//      - a wave whose lanes all hold one value in all their words (interior, flat exterior) issues ONE add of its pixel count;
//      - otherwise, per word, up to kCombineRounds rounds elect the lowest pending lane, ballot the lanes that hold its value and let
//        it add their population count; lanes still pending after the rounds add 1 each (their values are spread by then).
//  * the table: a block-private LDS copy (ds_add_u32), flushed once per block with one global_atomic_add per non-zero bin.  It does not
//    fit in general (M = 200 000 is 800 KB against 160 KB of LDS per CU), so the bins are cut into RANGES of kHistRangeBins (64 KB): a
//    block owns one range and one share of the plane, and counts only the values of its range.  The plane is read once per range — it
//    is the cheap part (a K4 plane is read in 0.025 ms; profiles/mandel_equalise_probe.txt), contended global atomics are not: the same
//    wave-combined adds sent straight to the global table take 16 ms on K4's plane whatever M is.  That scheme is kept for tables of more
//    than kHistMaxRanges ranges (max_iter >= 2^20), where the passes would cost as much.
//  * integer adds commute: the table is bit-reproducible whatever the arrival order.  Vector atomics and vector stores only.
#include <algorithm>
#include <cstring>

#include "mandel_distance_host.h"
#include "mandel_equalise.h"
#include "mandel_histogram_kernel.h"
#include "mandel_resolve_smooth_host.h"
#include "mandel_side_record.h"
#include "mandel_smooth_equalise_host.h"
#include "mandel_smooth_host.h"

namespace mc {

namespace {

// mandel_histogram_kernel<T, LDS>: the kernel of mandel_histogram_kernel.h (one text, shared with the smooth plane's histogram); a count's
// key is the count itself.
MC_HISTOGRAM_KERNEL(mandel_histogram_kernel, hist::KeyCount)

// d_rgba[i] = table[min(n[i], M)], table = lut[map[.]] composed on the host: ONE gather per pixel, as mandelbrot_assemble_kernel's.
// 2-4 B read + 16 B written per pixel, one pixel per lane (the float4 stores of a wave are 1 KB contiguous).
template <class T>
__global__ void __launch_bounds__(256) mandel_recolour_kernel(const T* __restrict__ iters, const float4* __restrict__ table,
                                                              float4* __restrict__ rgba, uint64_t total, uint32_t max_iter) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256u) {
        uint32_t n = (uint32_t)iters[i];
        if (n > max_iter) n = max_iter;
        rgba[i] = table[n];
    }
}

// The device state of the feature, a side record of the context (mandel_side_record.h).
struct EqualiseState {
    DeviceBuffer hist;                 // the whole-image calls' table
    DeviceBuffer table;                // lut[map[j]], (max_iter + 1) vec4: a cached device table like the colour LUT
    std::vector<uint32_t> table_map;   // what `table` was composed from: (map, max_iter, k_color)
    uint32_t table_max_iter = 0;
    float table_kcolor[4] = {0, 0, 0, 0};
    std::vector<float> lut_host;       // mandelbrot_build_lut(lut_max_iter, lut_kcolor)
    uint32_t lut_max_iter = 0;
    float lut_kcolor[4] = {0, 0, 0, 0};
    std::vector<uint32_t> hist_host, map_host;
};
SideRecords<EqualiseState> g_eq_states;

}  // namespace

void equalise_release(mc_context* ctx) {
    g_eq_states.erase(ctx, [](EqualiseState& st) {
        st.hist.release();
        st.table.release();
    });
}

int mandelbrot_histogram_launch(mc_context* ctx, const void* d_iters, uint32_t iters_bytes, uint64_t n_pixels, uint32_t max_iter,
                                void* d_hist, hipStream_t s) {
    if (!ctx || !d_iters || !d_hist || !max_iter || (iters_bytes != 2u && iters_bytes != 4u)) return MC_ERR_INVALID_ARGUMENT;
    if (n_pixels > 0xffffffffull) {
        set_error_detail("mc_mandelbrot_histogram_device_async: the table's bins are uint32_t, an image has fewer than 2^32 pixels");
        return MC_ERR_INVALID_ARGUMENT;
    }
    const uintptr_t addr = reinterpret_cast<uintptr_t>(d_iters);
    if (addr % iters_bytes || reinterpret_cast<uintptr_t>(d_hist) % 4u) return MC_ERR_INVALID_ARGUMENT;
    if (max_iter == 0xffffffffu) return MC_ERR_INVALID_ARGUMENT;   // (max_iter + 1 bins must be countable in 32 bits)
    if (!n_pixels) return MC_OK;
    const hist::Geometry g = hist::geometry(addr, iters_bytes, n_pixels, max_iter, (uint32_t)ctx->props.multiProcessorCount);
    const dim3 grid(g.grid), block(256);
    const bool lds = g.lds;
    const size_t shared = g.shared;
    const uint32_t head = g.head, tail = g.tail, rb = g.range_bins, ranges = g.ranges;
    const uint64_t nvec = g.nvec;
    uint32_t* h = (uint32_t*)d_hist;
    if (iters_bytes == 4u) {
        const uint32_t* in = (const uint32_t*)d_iters;
        if (lds) hipLaunchKernelGGL((mandel_histogram_kernel<uint32_t, true>), grid, block, shared, s, in, head, nvec, tail, max_iter, rb, ranges, h);
        else hipLaunchKernelGGL((mandel_histogram_kernel<uint32_t, false>), grid, block, shared, s, in, head, nvec, tail, max_iter, rb, ranges, h);
    } else {
        const uint16_t* in = (const uint16_t*)d_iters;
        if (lds) hipLaunchKernelGGL((mandel_histogram_kernel<uint16_t, true>), grid, block, shared, s, in, head, nvec, tail, max_iter, rb, ranges, h);
        else hipLaunchKernelGGL((mandel_histogram_kernel<uint16_t, false>), grid, block, shared, s, in, head, nvec, tail, max_iter, rb, ranges, h);
    }
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

// map[M] = M; j < M: map[j] = (M * C(j)) / E in uint64_t, C(j) = hist[0] + ... + hist[j-1], E = C(M); E = 0: map[j] = 0.
// The total is summed in 64 bits and must stay below 2^32 (both factors of the product then are): it is NOT compared with any
// image's size — a caller may equalise over a crop or over several frames on purpose.
int mandelbrot_equalise_map(uint32_t max_iter, const uint32_t* hist, uint32_t* map) {
    if (!max_iter || !hist || !map) return MC_ERR_INVALID_ARGUMENT;
    uint64_t total = 0;
    for (uint64_t j = 0; j <= max_iter; j++) total += hist[j];
    if (total > 0xffffffffull) {
        set_error_detail("mc_mandelbrot_equalise_map: the histogram's total exceeds 2^32 - 1");
        return MC_ERR_INVALID_ARGUMENT;
    }
    const uint64_t escaped = total - hist[max_iter];
    uint64_t below = 0;
    for (uint32_t j = 0; j < max_iter; j++) {
        map[j] = escaped ? (uint32_t)(((uint64_t)max_iter * below) / escaped) : 0u;
        below += hist[j];
    }
    map[max_iter] = max_iter;
    return MC_OK;
}

// lut[map[.]] composed on the host and kept as a device table of the context (the recolouring and the supersampling resolve share it).
int mandelbrot_composed_table(mc_context* ctx, const mc_mandelbrot_params* p, const uint32_t* map, const char* who, hipStream_t s,
                              const void** d_table) {
    const uint32_t M = p->max_iter;
    for (uint32_t j = 0; j <= M; j++)
        if (map[j] > M) {
            set_error_detail(std::string(who) + ": a map entry exceeds max_iter");
            return MC_ERR_INVALID_ARGUMENT;
        }
    EqualiseState* st = g_eq_states.get(ctx);
    const size_t entries = (size_t)M + 1;
    const bool cached = st->table.ptr && st->table_max_iter == M && std::memcmp(st->table_kcolor, p->k_color, sizeof(float) * 4) == 0 &&
                        st->table_map.size() == entries && std::memcmp(st->table_map.data(), map, entries * 4) == 0;
    if (!cached) {
        if (st->lut_host.size() != entries * 4 || st->lut_max_iter != M || std::memcmp(st->lut_kcolor, p->k_color, sizeof(float) * 4) != 0) {
            st->lut_host.resize(entries * 4);
            mandelbrot_build_lut(M, p->k_color, st->lut_host.data());
            st->lut_max_iter = M;
            std::memcpy(st->lut_kcolor, p->k_color, sizeof(float) * 4);
        }
        std::vector<float> composed(entries * 4);
        for (size_t j = 0; j < entries; j++) std::memcpy(&composed[4 * j], &st->lut_host[4 * (size_t)map[j]], sizeof(float) * 4);
        // an earlier recolouring of this context may still read the old table (possibly on another stream): wait for the streams this
        // context has launched on — not the whole device — before replacing it, as the colour table does
        int rc = ctx->drain_launch_streams();
        if (rc) return rc;
        st->table_map.clear();   // unusable until the copy below has completed
        if ((rc = st->table.reserve(entries * 16))) return rc;
        MC_HIP_TRY(hipMemcpyAsync(st->table.ptr, composed.data(), entries * 16, hipMemcpyHostToDevice, s));
        MC_HIP_TRY(hipStreamSynchronize(s));   // the host vector goes out of scope
        st->table_map.assign(map, map + entries);
        st->table_max_iter = M;
        std::memcpy(st->table_kcolor, p->k_color, sizeof(float) * 4);
    }
    *d_table = st->table.ptr;
    return MC_OK;
}

int mandelbrot_recolour_launch(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_iters, uint32_t iters_bytes,
                               const uint32_t* map, void* d_rgba, hipStream_t s) {
    if (!ctx || !p || !d_iters || !map || !d_rgba || !p->max_iter || !rows_ok(p)) return MC_ERR_INVALID_ARGUMENT;
    if (iters_bytes != 2u && iters_bytes != 4u) return MC_ERR_INVALID_ARGUMENT;
    if (iters_bytes == 2u && p->max_iter > 65535u) return MC_ERR_INVALID_ARGUMENT;
    if (p->row_stride && (!p->row_block || p->row_block > p->row_stride)) return MC_ERR_INVALID_ARGUMENT;
    const uint32_t M = p->max_iter;
    const void* table = nullptr;
    if (int rc = mandelbrot_composed_table(ctx, p, map, "mc_mandelbrot_recolour_device_async", s, &table)) return rc;
    const uint64_t total = (uint64_t)tile_rows(p->row_begin, p->row_end, p->row_stride ? p->row_block : 0u, p->row_stride) * p->width;
    uint64_t blocks = (total + 255u) / 256u;
    const uint64_t cap = (uint64_t)ctx->props.multiProcessorCount * 8u;
    if (blocks > cap) blocks = cap;
    if (iters_bytes == 2u)
        hipLaunchKernelGGL(mandel_recolour_kernel<uint16_t>, dim3((uint32_t)blocks), dim3(256), 0, s, (const uint16_t*)d_iters,
                           (const float4*)table, (float4*)d_rgba, total, M);
    else
        hipLaunchKernelGGL(mandel_recolour_kernel<uint32_t>, dim3((uint32_t)blocks), dim3(256), 0, s, (const uint32_t*)d_iters,
                           (const float4*)table, (float4*)d_rgba, total, M);
    MC_HIP_TRY(hipGetLastError());
    return ctx->note_launch(s);   // (reads the cached composed table)
}

int mandelbrot_equalise_plane_map(mc_context* ctx, uint32_t max_iter, const void* d_iters, uint32_t iters_bytes, uint64_t n_values,
                                  hipStream_t s, const uint32_t** map) {
    EqualiseState* st = g_eq_states.get(ctx);
    const size_t entries = (size_t)max_iter + 1;
    int rc = st->hist.reserve(entries * 4);
    if (rc) return rc;
    st->hist_host.resize(entries);
    st->map_host.resize(entries);
    MC_HIP_TRY(hipMemsetAsync(st->hist.ptr, 0, entries * 4, s));
    if ((rc = mandelbrot_histogram_launch(ctx, d_iters, iters_bytes, n_values, max_iter, st->hist.ptr, s))) return rc;
    MC_HIP_TRY(hipMemcpyAsync(st->hist_host.data(), st->hist.ptr, entries * 4, hipMemcpyDeviceToHost, s));
    MC_HIP_TRY(hipStreamSynchronize(s));
    if ((rc = mandelbrot_equalise_map(max_iter, st->hist_host.data(), st->map_host.data()))) return rc;
    *map = st->map_host.data();
    return MC_OK;
}

int mandelbrot_equalise_whole(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_iters, void* d_rgba, hipStream_t s) {
    const uint64_t npix = (uint64_t)p->width * p->height;
    if (npix > 0xffffffffull) {
        set_error_detail("MC_MANDEL_COLOUR_EQUALISED: the histogram's bins are uint32_t, width * height must stay below 2^32");
        return MC_ERR_INVALID_ARGUMENT;
    }
    const uint32_t* map = nullptr;
    if (int rc = mandelbrot_equalise_plane_map(ctx, p->max_iter, d_iters, 4u, npix, s, &map)) return rc;
    return mandelbrot_recolour_launch(ctx, p, d_iters, 4u, map, d_rgba, s);
}

int mandelbrot_equalise_warmup(mc_context* ctx, const mc_mandelbrot_params* p, hipStream_t s) {
    // scratch_iters holds at least 64 counts (mc_context_warmup_mandelbrot); scratch_rgba at least 64 vec4
    EqualiseState* st = g_eq_states.get(ctx);
    const size_t entries = (size_t)p->max_iter + 1;
    int rc = st->hist.reserve(entries * 4);
    if (rc) return rc;
    MC_HIP_TRY(hipMemsetAsync(st->hist.ptr, 0, entries * 4, s));
    MC_HIP_TRY(hipMemsetAsync(ctx->scratch_iters.ptr, 0, 64 * 4, s));
    if ((rc = mandelbrot_histogram_launch(ctx, ctx->scratch_iters.ptr, 4u, 64, p->max_iter, st->hist.ptr, s))) return rc;
    std::vector<uint32_t> identity(entries);
    for (size_t j = 0; j < entries; j++) identity[j] = (uint32_t)j;
    mc_mandelbrot_params q = *p;
    q.width = 8; q.height = 8; q.row_begin = 0; q.row_end = 8; q.row_block = q.row_stride = 0;
    return mandelbrot_recolour_launch(ctx, &q, ctx->scratch_iters.ptr, 4u, identity.data(), ctx->scratch_rgba.ptr, s);
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_mandelbrot_histogram_device_async(mc_context* ctx, const void* d_iters, uint32_t iters_bytes, uint64_t n_pixels,
                                         uint32_t max_iter, void* d_hist, void* stream) {
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    if (!d_iters || !d_hist || !max_iter || (iters_bytes != 2u && iters_bytes != 4u)) return MC_ERR_INVALID_ARGUMENT;
    MC_HIP_TRY(hipSetDevice(ctx->device));
    return mandelbrot_histogram_launch(ctx, d_iters, iters_bytes, n_pixels, max_iter, d_hist, stream ? (hipStream_t)stream : ctx->stream);
}

int mc_mandelbrot_equalise_map(uint32_t max_iter, const uint32_t* hist, uint32_t* map) {
    return mandelbrot_equalise_map(max_iter, hist, map);
}

int mc_mandelbrot_recolour_device_async(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_iters, uint32_t iters_bytes,
                                        const uint32_t* map, void* d_rgba_f32, void* stream) {
    if (!ctx || !p || !d_iters || !map || !d_rgba_f32 || !p->max_iter || (iters_bytes != 2u && iters_bytes != 4u))
        return MC_ERR_INVALID_ARGUMENT;
    if (int rc = smooth_samples_refuse_flag(p, "mc_mandelbrot_recolour_device_async")) return rc;
    if (int rc = smooth_equalised_refuse_flag(p, "mc_mandelbrot_recolour_device_async")) return rc;
    if (int rc = smooth_refuse_flag(p, "mc_mandelbrot_recolour_device_async")) return rc;
    if (int rc = distance_refuse_flag(p, "mc_mandelbrot_recolour_device_async")) return rc;
    MC_HIP_TRY(hipSetDevice(ctx->device));
    return mandelbrot_recolour_launch(ctx, p, d_iters, iters_bytes, map, d_rgba_f32, stream ? (hipStream_t)stream : ctx->stream);
}

}  // extern "C"
