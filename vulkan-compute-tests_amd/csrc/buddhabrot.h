// Buddhabrot (mc_buddhabrot_*): the one text of a sample's arithmetic, shared by the kernels (buddhabrot.hip) and the host call
// (buddhabrot_host.cpp, a translation unit without HIP), and the entry points the rest of the library calls.
// The contract is in include/mc_compute.h, restated in tests/buddhabrot_ref.py; sizing, the two kernel forms and their measurements in
// DESIGN.md §3.26; the importance map's cells and the guided samples' words (restated in tests/buddhabrot_guided_ref.py) in §3.27.
// Everything here is IEEE double in the order written: both translation units are built with -ffp-contract=off.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/mc_compute.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MC_BUDDHA_FN __host__ __device__ inline
#else
#define MC_BUDDHA_FN inline
#endif

namespace mc {

void set_error_detail(const std::string& s);   // api.hip (the stand-alone check brings its own)

namespace buddha {

constexpr uint32_t kMaxIterLimit = 1u << 24;
constexpr uint64_t kMaxSamples = 1ull << 40;
constexpr uint32_t kMaxLevels = 1u << 20;
enum { kSamples = 0, kSkipped = 1, kContributing = 2, kPoints = 3, kAdded = 4, kStats = 5 };   // mc_buddhabrot_stats' order

// What a launch reads of mc_buddhabrot_params, with the plot's constants formed once on the host (kx, ky: one IEEE division each).
struct Args {
    double vcx, vcy, kx, ky, ox, oy, wf, hf;
    double scx, scy, ssx, ssy;
    uint64_t begin, end;
    uint32_t width, max_iter, min_iter, seed;
};
inline Args make_args(const mc_buddhabrot_params* p) {
    Args a;
    a.vcx = p->view_centre_x; a.vcy = p->view_centre_y;
    a.wf = (double)p->width; a.hf = (double)p->height;
    a.kx = a.wf / p->view_scale_x; a.ky = a.hf / p->view_scale_y;
    a.ox = 0.5 * a.wf; a.oy = 0.5 * a.hf;
    a.scx = p->sample_centre_x; a.scy = p->sample_centre_y; a.ssx = p->sample_scale_x; a.ssy = p->sample_scale_y;
    a.begin = p->sample_begin; a.end = p->sample_end;
    a.width = p->width; a.max_iter = p->max_iter; a.min_iter = p->min_iter; a.seed = p->seed;
    return a;
}

// Sample k's hash words: three rounds of the integer hash of pathTracer.comp:107-110 on (low word, high word, seed), the integers kept.
MC_BUDDHA_FN void hash_words(uint32_t seed, uint64_t k, uint32_t& ux, uint32_t& uy) {
    uint32_t x = (uint32_t)k, y = (uint32_t)(k >> 32), z = seed;
    for (int r = 0; r < 3; r++) {
        const uint32_t nx = ((x >> 8) ^ y) * 1103515245u;
        const uint32_t ny = ((y >> 8) ^ z) * 1103515245u;
        const uint32_t nz = ((z >> 8) ^ x) * 1103515245u;
        x = nx; y = ny; z = nz;
    }
    ux = x; uy = y;
}
// The c of a pair of hash words in the sample window.
MC_BUDDHA_FN void c_of_words(const Args& a, uint32_t ux, uint32_t uy, double& cx, double& cy) {
    const double tx = ((double)ux + 0.5) * 0x1p-32;
    const double ty = ((double)uy + 0.5) * 0x1p-32;
    cx = a.scx + ((tx - 0.5) * a.ssx);
    cy = a.scy + ((ty - 0.5) * a.ssy);
}
MC_BUDDHA_FN void sample_c(const Args& a, uint64_t k, double& cx, double& cy) {
    uint32_t ux, uy;
    hash_words(a.seed, k, ux, uy);
    c_of_words(a, ux, uy, cx, cy);
}

// The guided calls: the sample window cut into G x G cells by the top g bits of the hash words, g in 1 .. 12.
constexpr uint32_t kMaxGridLog2 = 12, kMaxDilate = 8;
// The cell of a pair of hash words: (uy >> (32 - g)) * G + (ux >> (32 - g)), row-major, the cell rows following cy.
MC_BUDDHA_FN uint32_t cell_of(uint32_t ux, uint32_t uy, uint32_t g) { return ((uy >> (32u - g)) << g) | (ux >> (32u - g)); }
// A guided sample's words: the cell's coordinates on top, the hash's HIGH bits shifted down below them.  cell < G * G.
MC_BUDDHA_FN void guided_words(uint32_t cell, uint32_t g, uint32_t& ux, uint32_t& uy) {
    ux = ((cell & ((1u << g) - 1u)) << (32u - g)) | (ux >> g);
    uy = ((cell >> g) << (32u - g)) | (uy >> g);
}
// What a guided or an importance launch reads beside Args; the uniform call leaves it zeroed.
struct Guide {
    uint32_t* map;           // importance: uint32_t[G * G], or null
    const uint32_t* cells;   // guided: the list, or null
    uint32_t n_cells, g, weight;
};

// The interior skip: the main cardioid or the period-2 disc.
MC_BUDDHA_FN bool interior(double cx, double cy) {
    const double xm = cx - 0.25, y2 = cy * cy;
    const double q = (xm * xm) + y2;
    const double xp = cx + 1.0;
    return (q * (q + xm)) <= (0.25 * y2) || ((xp * xp) + y2) <= 0.0625;
}

// MC_PRECISION_F64's step (mandelbrot.hip StateF64::advance), operation for operation; returns |z|^2 of the new z.
struct Orbit {
    double zx, zy, sx, sy;
    MC_BUDDHA_FN void reset() { zx = zy = sx = sy = 0.0; }
    MC_BUDDHA_FN double advance(double cx, double cy) {
        const double nzx = (sx - sy) + cx;
        const double nzy = ((2.0 * zx) * zy) + cy;
        zx = nzx; zy = nzy;
        sx = zx * zx; sy = zy * zy;
        return sx + sy;
    }
};

// The bin z lands in; false: outside the view (a NaN is outside).  width * height < 2^32, so the index fits.
MC_BUDDHA_FN bool bin_of(const Args& a, double zx, double zy, uint32_t& bin) {
    const double fx = ((zx - a.vcx) * a.kx) + a.ox;
    const double fy = ((zy - a.vcy) * a.ky) + a.oy;
    if (!(fx >= 0.0 && fx < a.wf && fy >= 0.0 && fy < a.hf)) return false;
    bin = (uint32_t)fy * a.width + (uint32_t)fx;
    return true;
}

}  // namespace buddha

// buddhabrot_host.cpp (no HIP): the checks every call shares, the host calls' bodies.
int buddhabrot_check(const mc_buddhabrot_params* p, const char* who);
int buddhabrot_check_grid(uint32_t grid_log2, const char* who);
int buddhabrot_check_cell_list(const uint32_t* cells, uint32_t n_cells, uint32_t grid_log2, uint32_t weight, bool read_list, const char* who);
int buddhabrot_check_guide(const mc_buddhabrot_guide_params* guide, const char* who);
int buddhabrot_check_levels(uint32_t levels, const char* who);
int buddhabrot_check_maps(uint32_t levels, const uint32_t* m0, const uint32_t* m1, const uint32_t* m2, const char* who);
// table[c * (levels + 1) + j] = (float)m_c[j] / (float)levels: the tone map's quotients (the device form uploads them).
void buddhabrot_tone_table(uint32_t levels, const uint32_t* m0, const uint32_t* m1, const uint32_t* m2, float* table);

}  // namespace mc

#if defined(__HIPCC__)
struct mc_context;
namespace mc {
// buddhabrot.hip.  ADDS p's samples to d_plane and (unless null) d_stats on s.
int buddhabrot_launch(mc_context* ctx, const mc_buddhabrot_params* p, void* d_plane, void* d_stats, hipStream_t s);
// mc_buddhabrot_importance_device_async: the same samples, and map[cell(k)] += added_k; d_plane may be null (then no plane add is issued).
int buddhabrot_importance_launch(mc_context* ctx, const mc_buddhabrot_params* p, uint32_t grid_log2, void* d_map, void* d_plane,
                                 void* d_stats, hipStream_t s);
// mc_buddhabrot_density_guided_device_async: sample k in cell d_cells[k mod n_cells], every point adds weight.
int buddhabrot_guided_launch(mc_context* ctx, const mc_buddhabrot_params* p, const void* d_cells, uint32_t n_cells, uint32_t grid_log2,
                             uint32_t weight, void* d_plane, void* d_stats, hipStream_t s);
// mc_buddhabrot_render_guided's device map (G * G words), cell lists (G * G words: the list, then its complement) and the three statistics
// records of its passes (pilot, render, complement: 3 x 5 x uint64_t), buffers of the context's side record.
int buddhabrot_guide_buffers(mc_context* ctx, uint32_t grid_log2, void** d_map, void** d_cells, void** d_stats3);
// mc_buddhabrot_render's device plane (width * height words) and statistics (5 x uint64_t), buffers of the context's side record.
int buddhabrot_render_buffers(mc_context* ctx, const mc_buddhabrot_params* p, void** d_plane, void** d_stats);
int buddhabrot_tonemap_launch(mc_context* ctx, uint32_t width, uint32_t height, const void* d0, const void* d1, const void* d2,
                              uint32_t levels, const uint32_t* m0, const uint32_t* m1, const uint32_t* m2, void* d_rgba, hipStream_t s);
// mc_context_destroy: the context's plane, statistics and tone table, if any, are freed.
void buddhabrot_release(mc_context* ctx);
}  // namespace mc
#endif
