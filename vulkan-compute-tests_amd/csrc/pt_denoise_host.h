// Path-tracer denoiser, host side: the launchers and the argument checks the entry points share (pt_denoise.hip; the fused call
// mc_pathtrace_render_denoised is api.hip's, beside the blocking calls whose skeleton it uses).  The arithmetic is in pt_denoise.h.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "mc_internal.h"
#include "pt_denoise.h"

namespace mc {

// d: not NULL, sizes above 0, passes in 1 .. 8, sigma_colour finite and above 0 (and its fp32 square neither 0 nor infinite), k_normal and
// k_position finite and not negative, flags 0.  who: the entry point's name for the refusal.
int pt_denoise_check_params(const mc_pathtrace_denoise_params* d, const char* who);
// The scene tables of a guides call: a table that is NULL although it has entries, more than 2^20 objects (MC_ERR_UNSUPPORTED).
int pt_guides_check_scene(const float* planes, uint32_t n_planes, const float* spheres, uint32_t n_spheres, const char* who);

// Bytes of device scratch a guides launch needs for the scene records (a multiple of 256).
size_t pt_guides_records_bytes(uint32_t n_planes, uint32_t n_spheres);
// The guide planes of a W x H image into d_normal_t and d_position_id (vec4 each, storage order) on s.  d_records: device scratch of
// pt_guides_records_bytes(); the host tables are copied there on s and s is synchronised (they are pageable memory of the caller's).
int pt_guides_launch(mc_context* ctx, uint32_t W, uint32_t H, const float* planes, uint32_t n_planes, const float* spheres, uint32_t n_spheres,
                     void* d_records, void* d_normal_t, void* d_position_id, const char* who, hipStream_t s);
// The d->passes passes from d_rgba into d_out (which may be d_rgba) on s, through the two W x H vec4 scratch planes d_tmp0 and d_tmp1.
int pt_denoise_launch(mc_context* ctx, const mc_pathtrace_denoise_params* d, const void* d_rgba, const void* d_normal_t, const void* d_position_id,
                      void* d_out, void* d_tmp0, void* d_tmp1, const char* who, hipStream_t s);

// ---- the noise plane and the filter it steers (pt_noise.hip; arithmetic in pt_noise.h) --------------------
// radius at most 4; k_noise finite and above 0 with a finite fp32 square.
int pt_noise_check(uint32_t radius, const char* who);
int pt_noise_check_k(float k_noise, const char* who);
// Bytes of one float per pixel, rounded up to a multiple of 256 (the planes of a scratch layout start aligned).
inline size_t pt_noise_plane_bytes(size_t npix) { return (npix * 4 + 255) & ~(size_t)255; }
// V of a W x H image into d_variance (one float per pixel) on s, from the vec4 planes d_half and d_full; d_v: scratch of one float per pixel.
int pt_noise_launch(mc_context* ctx, uint32_t W, uint32_t H, const void* d_half, float scale, const void* d_full, uint32_t radius, void* d_variance,
                    void* d_v, const char* who, hipStream_t s);
// pt_denoise_launch with the colour weight taken per pixel from d_variance and k_noise (d->sigma_colour is checked and not used).
int pt_denoise_adaptive_launch(mc_context* ctx, const mc_pathtrace_denoise_params* d, float k_noise, const void* d_rgba, const void* d_normal_t,
                               const void* d_position_id, const void* d_variance, void* d_out, void* d_tmp0, void* d_tmp1, const char* who,
                               hipStream_t s);

// ---- what the translation units of the denoiser share (pt_denoise.hip, pt_noise.hip) ----------------------------------------------
namespace ptdh {

using ptd::vec4;

// The launch shape of every plane kernel: blocks of 64 x 4 lanes, a wave on 64 adjacent pixels of a storage row, blockIdx.y striding the rows.
inline dim3 plane_grid(uint32_t W, uint32_t H) { return dim3((W + 63u) / 64u, std::min<uint32_t>((H + 3u) / 4u, 65535u)); }

inline bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}
inline bool misaligned(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16u != 0u; }

inline int refuse(const char* who, const std::string& what) {
    set_error_detail(std::string(who) + ": " + what);
    return MC_ERR_INVALID_ARGUMENT;
}

// A host plane as vec4: the caller's memory where it is 16-byte aligned, a copy in `store` otherwise.
inline const vec4* aligned_in(const float* a, size_t npix, std::vector<vec4>& store) {
    if (!misaligned(a)) return reinterpret_cast<const vec4*>(a);
    store.resize(npix);
    std::memcpy(store.data(), a, npix * 16);
    return store.data();
}
// A host output plane: written in place where aligned, else through `store` (finish() copies it out).
struct AlignedOut {
    float* user;
    size_t npix;
    std::vector<vec4> store;
    AlignedOut(float* u, size_t n) : user(u), npix(n) { if (misaligned(u)) store.resize(n); }
    vec4* ptr() { return store.empty() ? reinterpret_cast<vec4*>(user) : store.data(); }
    void finish() { if (!store.empty()) std::memcpy(user, store.data(), npix * 16); }
};

}  // namespace ptdh

}  // namespace mc
