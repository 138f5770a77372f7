// Path tracer BVH, host side: what pt_bvh_host.cpp (plain C++17, no HIP header: it also builds and runs on its own,
// tools/pt_bvh_host_check.cpp), pt_bvh.hip (the launches) and api.hip (the blocking calls) share.  The arithmetic is in pt_bvh.h.
#pragma once
#include <string>

#include "../../include/mc_compute.h"
#include "pt_bvh.h"

namespace mc {

void set_error_detail(const std::string& s);   // api.hip (the stand-alone check brings its own)

// True while `a` is an object mc_pathtrace_accel_create returned and mc_pathtrace_accel_destroy has not yet taken.
bool pt_accel_live(const mc_pathtrace_accel* a);
// Frees the device copies made for `a` (pt_bvh.hip; the stand-alone check brings an empty one).  Called by mc_pathtrace_accel_destroy.
void pt_accel_release_device(const mc_pathtrace_accel* a);
// Device copies held for `a` at the moment (pt_bvh.hip): mc_pathtrace_accel_info reports it.
uint32_t pt_accel_device_copies(const mc_pathtrace_accel* a);

}  // namespace mc
