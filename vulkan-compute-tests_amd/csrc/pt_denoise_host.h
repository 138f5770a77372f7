// Path-tracer denoiser, host side: the launchers and the argument checks the entry points share (pt_denoise.hip; the fused call
// mc_pathtrace_render_denoised is api.hip's, beside the blocking calls whose skeleton it uses).  The arithmetic is in pt_denoise.h.
#pragma once
#include <string>

#include "mc_internal.h"

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

}  // namespace mc
