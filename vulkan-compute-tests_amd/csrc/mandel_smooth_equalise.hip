// Smooth equalised Mandelbrot colouring for gfx950 (MI355X): the histogram of a smooth plane keyed by q >> 8, the knot map, the remap and
// its colour.  The project's own addition; contract in include/mc_compute.h, restated in tests/mandel_smooth_equalise_ref.py; scheme and
// measurements in DESIGN.md §3.21.  The arithmetic is mandel_smooth_equalise.h, the same source the host calls run.
//
// The histogram kernel is mandel_histogram_kernel.h's, the text mandel_histogram.hip expands for count planes, here with the key q >> 8:
// wave combining, LDS tables over ranges of 16 384 bins, one global add per non-zero bin at the flush, the global table from 64 ranges on.
//
// The remap kernel: one lane per pixel of a grid-stride loop.  4 B read (q); ONE aligned 8-B gather from a pair table
// (qmap[j], qmap[j + 1] - qmap[j]) composed on the host and cached on the device, not two unaligned 4-B gathers of neighbouring knots;
// the smooth colour's two gathers from the L2-resident colour table (rgb of each 16-B entry); a 16-B store and / or a 4-B store of q'.  No LDS, no atomics,
// no synchronisation; vector loads and stores only.
#include <algorithm>
#include <cstring>
#include <vector>

#include "mandel_distance_host.h"
#include "mandel_histogram_kernel.h"
#include "mandel_resolve_smooth_host.h"
#include "mandel_side_record.h"
#include "mandel_smooth_equalise.h"
#include "mandel_smooth_equalise_host.h"

namespace mc {

namespace {

// mandel_smooth_histogram_kernel<uint32_t, LDS>: a smooth count's key is its integer part.
MC_HISTOGRAM_KERNEL(mandel_smooth_histogram_kernel, hist::KeySmooth)

// q: total smooth counts (a compact tile); pairs: max_iter (knot, step) entries; lut: (max_iter + 1) vec4, read only where rgba is given.
__global__ void __launch_bounds__(256) mandel_smooth_remap_kernel(const uint32_t* __restrict__ q, const uint2* __restrict__ pairs,
                                                                  const float4* __restrict__ lut, uint32_t* __restrict__ ranked,
                                                                  float4* __restrict__ rgba, uint64_t total, uint32_t max_iter) {
    const uint32_t top = 256u * max_iter;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t v = q[i];
        uint32_t r = top;
        if (v < top) {   // v >> 8 < max_iter: inside the pair table
            const uint2 pr = pairs[v >> 8];
            r = smooth_equalise::remap_pair(v, pr.x, pr.y);
        }
        if (ranked) ranked[i] = r;
        if (rgba) {   // r <= top (the launcher has checked the knots): smooth_colour reads lut[r >> 8] and its successor, at most lut[max_iter]
            float c[4];
            smooth::smooth_colour(r < top ? r : top, max_iter, reinterpret_cast<const float*>(lut), c);
            rgba[i] = make_float4(c[0], c[1], c[2], c[3]);
        }
    }
}

// The device state of the feature, a side record of the context (mandel_side_record.h).
struct SmoothEqualiseState {
    DeviceBuffer hist;                 // the whole-image calls' table
    DeviceBuffer pairs;                // (qmap[j], qmap[j + 1] - qmap[j]), max_iter uint2: a cached device table like the colour LUT
    std::vector<uint32_t> pairs_map;   // the knots `pairs` was composed from (max_iter + 1 of them); empty: none
    std::vector<uint32_t> hist_host, qmap_host;
};
SideRecords<SmoothEqualiseState> g_sq_states;

// A caller's knot table: non-decreasing, no entry above 256 * max_iter, the last one equal to it.
int check_knots(uint32_t max_iter, const uint32_t* qmap, const char* who) {
    const uint32_t top = 256u * max_iter;
    if (qmap[max_iter] != top) {
        set_error_detail(std::string(who) + ": qmap[max_iter] must be 256 * max_iter");
        return MC_ERR_INVALID_ARGUMENT;
    }
    for (uint32_t j = 0; j < max_iter; j++)
        if (qmap[j] > qmap[j + 1]) {   // (with the last entry at the top this bounds every entry)
            set_error_detail(std::string(who) + ": qmap[" + std::to_string(j) + "] = " + std::to_string(qmap[j]) +
                             (qmap[j] > top ? " is above 256 * max_iter" : " is above its successor: the knots must not decrease"));
            return MC_ERR_INVALID_ARGUMENT;
        }
    return MC_OK;
}

// The pair table of qmap as a cached device table of the context.
int pairs_device(mc_context* ctx, uint32_t max_iter, const uint32_t* qmap, hipStream_t s, const void** d_pairs) {
    SmoothEqualiseState* st = g_sq_states.get(ctx);
    const size_t knots = (size_t)max_iter + 1;
    const bool cached = st->pairs.ptr && st->pairs_map.size() == knots && std::memcmp(st->pairs_map.data(), qmap, knots * 4) == 0;
    if (!cached) {
        std::vector<uint32_t> composed((size_t)max_iter * 2);
        smooth_equalise::compose_pairs(max_iter, qmap, composed.data());
        // an earlier remap of this context may still read the old table (possibly on another stream): wait for the streams this context
        // has launched on before replacing it, as the colour table does
        int rc = ctx->drain_launch_streams();
        if (rc) return rc;
        st->pairs_map.clear();   // unusable until the copy below has completed
        if ((rc = st->pairs.reserve((size_t)max_iter * 8))) return rc;
        MC_HIP_TRY(hipMemcpyAsync(st->pairs.ptr, composed.data(), (size_t)max_iter * 8, hipMemcpyHostToDevice, s));
        MC_HIP_TRY(hipStreamSynchronize(s));   // the host vector goes out of scope
        st->pairs_map.assign(qmap, qmap + knots);
    }
    *d_pairs = st->pairs.ptr;
    return MC_OK;
}

}  // namespace

int smooth_equalise_check_knots(uint32_t max_iter, const uint32_t* qmap, const char* who) { return check_knots(max_iter, qmap, who); }
int smooth_equalise_pairs_device(mc_context* ctx, uint32_t max_iter, const uint32_t* qmap, hipStream_t s, const void** d_pairs) {
    return pairs_device(ctx, max_iter, qmap, s, d_pairs);
}

void smooth_equalise_release(mc_context* ctx) {
    g_sq_states.erase(ctx, [](SmoothEqualiseState& st) {
        st.hist.release();
        st.pairs.release();
    });
}

// The arguments of the histogram stage, checked before the context is touched.
static int smooth_histogram_check(const mc_context* ctx, const void* d_smooth, uint64_t n_pixels, uint32_t max_iter, const void* d_hist) {
    if (!ctx || !d_smooth || !d_hist || !max_iter) return MC_ERR_INVALID_ARGUMENT;
    if (max_iter > kSmoothMaxIter) {
        set_error_detail("mc_mandelbrot_smooth_histogram_device_async: max_iter <= 2^24 - 1 (the smooth plane is 24.8 fixed point)");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (n_pixels > 0xffffffffull) {
        set_error_detail("mc_mandelbrot_smooth_histogram_device_async: the table's bins are uint32_t, an image has fewer than 2^32 pixels");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (reinterpret_cast<uintptr_t>(d_smooth) % 4u || reinterpret_cast<uintptr_t>(d_hist) % 4u) return MC_ERR_INVALID_ARGUMENT;
    return MC_OK;
}

int mandelbrot_smooth_histogram_launch(mc_context* ctx, const void* d_smooth, uint64_t n_pixels, uint32_t max_iter, void* d_hist,
                                       hipStream_t s) {
    if (int rc = smooth_histogram_check(ctx, d_smooth, n_pixels, max_iter, d_hist)) return rc;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(d_smooth);
    if (!n_pixels) return MC_OK;
    const hist::Geometry g = hist::geometry(addr, 4u, n_pixels, max_iter, (uint32_t)ctx->props.multiProcessorCount);
    const dim3 grid(g.grid), block(256);
    const uint32_t* in = (const uint32_t*)d_smooth;
    uint32_t* h = (uint32_t*)d_hist;
    if (g.lds)
        hipLaunchKernelGGL((mandel_smooth_histogram_kernel<uint32_t, true>), grid, block, g.shared, s, in, g.head, g.nvec, g.tail, max_iter,
                           g.range_bins, g.ranges, h);
    else
        hipLaunchKernelGGL((mandel_smooth_histogram_kernel<uint32_t, false>), grid, block, g.shared, s, in, g.head, g.nvec, g.tail, max_iter,
                           g.range_bins, g.ranges, h);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

// The remap stage's params: the flag, alone among the colourings.
static int smooth_remap_check(const mc_mandelbrot_params* p, const char* who) {
    if (int rc = smooth_samples_refuse_flag(p, who)) return rc;
    if (!smooth_equalised_flag(p)) {
        set_error_detail(std::string(who) + ": the params must carry MC_MANDEL_COLOUR_SMOOTH_EQUALISED");
        return MC_ERR_INVALID_ARGUMENT;
    }
    return smooth_equalised_refuse_combination(p, who);
}

int mandelbrot_smooth_remap_launch(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_smooth, const uint32_t* qmap, void* d_ranked,
                                   void* d_rgba, const char* who, hipStream_t s) {
    if (!ctx || !p || !d_smooth || !qmap || (!d_ranked && !d_rgba) || !p->max_iter || !rows_ok(p)) return MC_ERR_INVALID_ARGUMENT;
    if (int rc = smooth_remap_check(p, who)) return rc;
    if (p->row_stride && (!p->row_block || p->row_block > p->row_stride)) return MC_ERR_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(d_smooth) % 4u || reinterpret_cast<uintptr_t>(d_ranked) % 4u || reinterpret_cast<uintptr_t>(d_rgba) % 16u)
        return MC_ERR_INVALID_ARGUMENT;
    const uint32_t M = p->max_iter;
    if (int rc = check_knots(M, qmap, who)) return rc;
    const void* pairs = nullptr;
    if (int rc = pairs_device(ctx, M, qmap, s, &pairs)) return rc;
    const void* lut = nullptr;
    if (d_rgba)
        if (int rc = mandelbrot_lut_device(ctx, p, s, &lut)) return rc;
    const uint64_t total = (uint64_t)tile_rows(p->row_begin, p->row_end, p->row_stride ? p->row_block : 0u, p->row_stride) * p->width;
    uint64_t blocks = (total + 255u) / 256u;
    const uint64_t cap = (uint64_t)ctx->props.multiProcessorCount * 8u;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(mandel_smooth_remap_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, (const uint32_t*)d_smooth, (const uint2*)pairs,
                       (const float4*)lut, (uint32_t*)d_ranked, (float4*)d_rgba, total, M);
    MC_HIP_TRY(hipGetLastError());
    return ctx->note_launch(s);   // (reads the cached pair and colour tables)
}

int mandelbrot_smooth_equalise_plane_map(mc_context* ctx, uint32_t max_iter, const void* d_smooth, uint64_t n, hipStream_t s,
                                         const uint32_t** qmap) {
    SmoothEqualiseState* st = g_sq_states.get(ctx);
    const size_t entries = (size_t)max_iter + 1;
    int rc = st->hist.reserve(entries * 4);
    if (rc) return rc;
    st->hist_host.resize(entries);
    st->qmap_host.resize(entries);
    MC_HIP_TRY(hipMemsetAsync(st->hist.ptr, 0, entries * 4, s));
    if ((rc = mandelbrot_smooth_histogram_launch(ctx, d_smooth, n, max_iter, st->hist.ptr, s))) return rc;
    MC_HIP_TRY(hipMemcpyAsync(st->hist_host.data(), st->hist.ptr, entries * 4, hipMemcpyDeviceToHost, s));
    MC_HIP_TRY(hipStreamSynchronize(s));
    if (!smooth_equalise::knot_map(max_iter, st->hist_host.data(), st->qmap_host.data())) return MC_ERR_INVALID_ARGUMENT;   // (n < 2^32: cannot happen)
    *qmap = st->qmap_host.data();
    return MC_OK;
}

int mandelbrot_smooth_equalise_whole(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_smooth, void* d_ranked, void* d_rgba,
                                     const char* who, hipStream_t s) {
    const uint64_t npix = (uint64_t)p->width * p->height;
    if (npix > 0xffffffffull) {
        set_error_detail(std::string(who) + ": MC_MANDEL_COLOUR_SMOOTH_EQUALISED: the histogram's bins are uint32_t, width * height must stay "
                         "below 2^32");
        return MC_ERR_INVALID_ARGUMENT;
    }
    const uint32_t* qmap = nullptr;
    if (int rc = mandelbrot_smooth_equalise_plane_map(ctx, p->max_iter, d_smooth, npix, s, &qmap)) return rc;
    return mandelbrot_smooth_remap_launch(ctx, p, d_smooth, qmap, d_ranked, d_rgba, who, s);
}

int mandelbrot_smooth_equalise_warmup(mc_context* ctx, const mc_mandelbrot_params* p, void* d_smooth, void* d_rgba, hipStream_t s) {
    // d_smooth holds at least 64 counts, d_rgba at least 64 vec4 (mc_context_warmup_mandelbrot)
    SmoothEqualiseState* st = g_sq_states.get(ctx);
    const size_t entries = (size_t)p->max_iter + 1;
    int rc = st->hist.reserve(entries * 4);
    if (rc) return rc;
    MC_HIP_TRY(hipMemsetAsync(st->hist.ptr, 0, entries * 4, s));
    MC_HIP_TRY(hipMemsetAsync(d_smooth, 0, 64 * 4, s));
    if ((rc = mandelbrot_smooth_histogram_launch(ctx, d_smooth, 64, p->max_iter, st->hist.ptr, s))) return rc;
    std::vector<uint32_t> identity(entries);   // the knots of a flat histogram: the table's device buffer at the request's size
    for (size_t j = 0; j < entries; j++) identity[j] = 256u * (uint32_t)j;
    mc_mandelbrot_params q = *p;
    q.width = 8; q.height = 8; q.row_begin = 0; q.row_end = 8; q.row_block = q.row_stride = 0;
    return mandelbrot_smooth_remap_launch(ctx, &q, d_smooth, identity.data(), nullptr, d_rgba, "mc_context_warmup_mandelbrot", s);
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_mandelbrot_smooth_histogram_device_async(mc_context* ctx, const void* d_smooth, uint64_t n_pixels, uint32_t max_iter, void* d_hist,
                                                void* stream) {
    if (int rc = smooth_histogram_check(ctx, d_smooth, n_pixels, max_iter, d_hist)) return rc;
    MC_HIP_TRY(hipSetDevice(ctx->device));
    return mandelbrot_smooth_histogram_launch(ctx, d_smooth, n_pixels, max_iter, d_hist, stream ? (hipStream_t)stream : ctx->stream);
}

int mc_mandelbrot_smooth_equalise_map(uint32_t max_iter, const uint32_t* hist, uint32_t* qmap) {
    if (!max_iter || max_iter > kSmoothMaxIter || !hist || !qmap) return MC_ERR_INVALID_ARGUMENT;
    if (!smooth_equalise::knot_map(max_iter, hist, qmap)) {
        set_error_detail("mc_mandelbrot_smooth_equalise_map: the histogram's total exceeds 2^32 - 1");
        return MC_ERR_INVALID_ARGUMENT;
    }
    return MC_OK;
}

int mc_mandelbrot_smooth_remap(uint32_t max_iter, const uint32_t* qmap, const uint32_t* q, uint64_t count, uint32_t* out_ranked) {
    if (!max_iter || max_iter > kSmoothMaxIter || !qmap || (count && (!q || !out_ranked))) return MC_ERR_INVALID_ARGUMENT;
    if (int rc = check_knots(max_iter, qmap, "mc_mandelbrot_smooth_remap")) return rc;
    for (uint64_t i = 0; i < count; i++)
        if (q[i] > 256u * max_iter) {
            set_error_detail("mc_mandelbrot_smooth_remap: q[" + std::to_string(i) + "] = " + std::to_string(q[i]) + " is above 256 * max_iter");
            return MC_ERR_INVALID_ARGUMENT;
        }
    std::vector<uint32_t> pairs((size_t)max_iter * 2);
    smooth_equalise::compose_pairs(max_iter, qmap, pairs.data());
    for (uint64_t i = 0; i < count; i++) out_ranked[i] = smooth_equalise::remap(q[i], max_iter, pairs.data());
    return MC_OK;
}

int mc_mandelbrot_smooth_remap_device_async(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_smooth, const uint32_t* qmap,
                                            void* d_ranked, void* d_rgba_f32, void* stream) {
    if (!ctx || !p || !d_smooth || !qmap || (!d_ranked && !d_rgba_f32) || !p->max_iter) return MC_ERR_INVALID_ARGUMENT;
    if (int rc = smooth_remap_check(p, "mc_mandelbrot_smooth_remap_device_async")) return rc;
    MC_HIP_TRY(hipSetDevice(ctx->device));
    return mandelbrot_smooth_remap_launch(ctx, p, d_smooth, qmap, d_ranked, d_rgba_f32, "mc_mandelbrot_smooth_remap_device_async",
                                          stream ? (hipStream_t)stream : ctx->stream);
}

}  // extern "C"
