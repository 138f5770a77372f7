// Path tracer BVH, device side of the host code: the launches and the selection pt_bvh.hip / pt_bvh_guides.hip define and api.hip's blocking
// calls use.
#pragma once
#include "mc_internal.h"
#include "pt_bvh_host.h"

namespace mc {

// The request's checks (the plain render's, plus: flags must be 0, no extended sphere-test precision) and the kernel that will run.
int pathtrace_accel_select(const mc_pathtrace_accel* a, const mc_pathtrace_params* p, mc_pathtrace_kernel_info* out, const char* who);
// The render of p through a's tree into d_rgba on s.  The device copy of `a` for ctx is made on first use and kept.
int pathtrace_accel_launch(mc_context* ctx, const mc_pathtrace_accel* a, const mc_pathtrace_params* p, void* d_rgba, hipStream_t s,
                           const char* who);
// mc_pathtrace_render_accel_list_device_async after the context: every check of the list render (pt_budget_list_render's, with the
// object's in place of the tables'), then the list kernels of pt_bvh_kernel.h.  DESIGN.md section 3.24.
int pathtrace_accel_list_render(mc_context* ctx, const mc_pathtrace_accel* a, const mc_pathtrace_params* p, const void* d_list, uint32_t n_list,
                                float prescale, void* d_acc, const char* who, hipStream_t s);
// The device pointers of a's copy for ctx (made on first use, on s).
int pt_accel_device_view(mc_context* ctx, const mc_pathtrace_accel* a, hipStream_t s, bvh::View& view);
// The object of a guides call: not NULL, live.
int pt_accel_guides_check(const mc_pathtrace_accel* a, const char* who);
// The guide planes of a W x H image through a's tree into d_normal_t and d_position_id (vec4 each, storage order) on s (pt_bvh_guides.hip).
int pt_accel_guides_launch(mc_context* ctx, const mc_pathtrace_accel* a, uint32_t W, uint32_t H, void* d_normal_t, void* d_position_id,
                           const char* who, hipStream_t s);
// Frees every device copy made for ctx (mc_context_destroy).
void pt_accel_release_context(mc_context* ctx);

}  // namespace mc
