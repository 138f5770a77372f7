// What the Mandelbrot render kernels address (the mapping templates of mandel_kernels.h and the two BLA kernels): the target block of their
// arguments, the 8x8 tile mapping, the store epilogue, and the launch geometry the two host launchers (launch_impl of mandelbrot.hip,
// perturb_launch of mandel_perturb.hip) compute from a request.
#pragma once
#include "mandel_adaptive.h"
#include "mc_internal.h"

namespace mc {

// The first member of every perturbation kernel's argument struct: the image, the tile's rows, the outputs and the two tables every
// one of them reads.  (MandelArgs of mandelbrot.hip keeps its own layout; the helpers below take either, and target_of of
// mandel_kernels.h names the one a kernel's arguments hold.)
struct MandelTarget {
    uint32_t W, H, max_iter, L;      // L: the orbit's length
    uint32_t row_begin, row_end, row_block, row_stride;
    float4* out_rgba;                // tile-local, may be null
    uint32_t* out_iters;             // tile-local, may be null
    uint16_t* out_iters16;           // the same plane as 16-bit counts (MC_MANDEL_ITERS_U16, max_iter <= 65535), may be null
    const float4* lut;               // max_iter+1 entries (null when out_rgba is null)
    const double* table;             // [x[W] | y[H]]: the pixel's offset from c_ref per column / per row (dc), a deep orbit's mantissas (u)
    const double2* orbit;            // Z_0 .. Z_L
};

#ifdef __HIPCC__
// workgroup = one wave = one 8x8 pixel tile, lane = (lx, ly) inside the tile.
struct TileLane {
    uint32_t gx, ty, gy;   // the column, the tile-local row, the storage row
    bool valid;            // inside the image and the tile's rows (mandelbrot.comp:27-28)
};

template <class Target>
__device__ __forceinline__ TileLane tile_lane(const Target& t) {
    const uint32_t lane = threadIdx.x;
    TileLane r;
    r.gx = blockIdx.x * 8u + (lane & 7u);
    r.ty = blockIdx.y * 8u + (lane >> 3);
    r.gy = tile_row_to_storage(r.ty, t.row_begin, t.row_block, t.row_stride);
    r.valid = r.gx < t.W && r.gy < t.row_end;
    return r;
}

// The lane's count n into whichever of the three outputs exist (row-major, tile-local: mandelbrot.comp:59).
template <class Target>
__device__ __forceinline__ void tile_store(const Target& t, const TileLane& ln, uint32_t n) {
    if (ln.valid) {
        const size_t idx = (size_t)ln.ty * t.W + ln.gx;
        if (t.out_iters) t.out_iters[idx] = n;
        if (t.out_iters16) t.out_iters16[idx] = (uint16_t)n;
        if (t.out_rgba) t.out_rgba[idx] = t.lut[n];
    }
}
#endif

// A request's launch geometry into t (W, H, max_iter, the normalised row fields, the three outputs with the uint16 split) and *grid.
// warm = the cold-start warm-up: one 8 x 8 tile run for at most 32 iterations, no colours (d_iters holds at least eight rows of counts).
// list = the list render of mandel_adaptive.h (p is the sample grid): a wave takes 64 / s^2 entries, one entry when warm, and the
// kernel's own outputs stay unused; *l is the list to launch with.  t->lut is the caller's: its table where t->out_rgba is set.
template <class Target>
int launch_geometry(const mc_mandelbrot_params* p, void* d_rgba, void* d_iters, bool warm, const SampleList* list, Target* t, dim3* grid,
                    SampleList* l) {
    const bool narrow = (p->flags & MC_MANDEL_ITERS_U16) != 0u;
    if (narrow && p->max_iter > 65535u) return MC_ERR_INVALID_ARGUMENT;
    t->W = p->width; t->H = p->height; t->max_iter = p->max_iter;
    t->row_begin = p->row_begin; t->row_end = p->row_end;
    t->row_block = p->row_stride ? p->row_block : 0u; t->row_stride = p->row_stride;
    t->out_rgba = warm ? nullptr : (float4*)d_rgba;
    t->out_iters = narrow ? nullptr : (uint32_t*)d_iters;
    t->out_iters16 = narrow ? (uint16_t*)d_iters : nullptr;
    const uint32_t rows = tile_rows(p->row_begin, p->row_end, t->row_block, t->row_stride);
    *grid = dim3((p->width + 7u) / 8u, (rows + 7u) / 8u);
    if (warm) {
        *grid = dim3(1, 1);
        t->max_iter = p->max_iter < 32u ? p->max_iter : 32u;
    }
    if (list) {
        t->out_rgba = nullptr; t->out_iters = nullptr; t->out_iters16 = nullptr;
        *l = *list;
        if (warm) l->count = 1u;
        const uint32_t per = 64u >> (2u * l->log2s);
        *grid = dim3((l->count + per - 1u) / per);
    }
    return MC_OK;
}

}  // namespace mc
