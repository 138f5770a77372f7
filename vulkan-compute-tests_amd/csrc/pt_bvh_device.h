// Path tracer BVH, device side of the host code: the launch and the selection pt_bvh.hip defines and api.hip's blocking calls use.
#pragma once
#include "mc_internal.h"
#include "pt_bvh_host.h"

namespace mc {

// The request's checks (the plain render's, plus: flags must be 0, no extended sphere-test precision) and the kernel that will run.
int pathtrace_accel_select(const mc_pathtrace_accel* a, const mc_pathtrace_params* p, mc_pathtrace_kernel_info* out, const char* who);
// The render of p through a's tree into d_rgba on s.  The device copy of `a` for ctx is made on first use and kept.
int pathtrace_accel_launch(mc_context* ctx, const mc_pathtrace_accel* a, const mc_pathtrace_params* p, void* d_rgba, hipStream_t s,
                           const char* who);
// Frees every device copy made for ctx (mc_context_destroy).
void pt_accel_release_context(mc_context* ctx);

}  // namespace mc
