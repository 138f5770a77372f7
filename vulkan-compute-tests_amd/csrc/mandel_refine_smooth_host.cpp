// mc_mandelbrot_refine_smooth: the refine rule of MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE on the host (include/mc_compute.h states the
// contract).  A translation unit without HIP: the rule is mandel_refine_smooth.h, the text the kernel compiles, and
// tools/mandel_refine_smooth_host_check.cpp links this file alone under a sanitizer.
#include <string>

#include "../../include/mc_compute.h"
#include "mandel_refine_smooth.h"

namespace mc {
void set_error_detail(const std::string& s);   // api.hip (the stand-alone check brings its own)
}

extern "C" int mc_mandelbrot_refine_smooth(uint32_t width, uint32_t height, uint32_t max_iter, const uint32_t* q, uint32_t threshold,
                                           uint8_t* mask, uint64_t* refined) {
    const char* what = !width || !height                    ? "width and height must be at least 1"
                       : !max_iter || max_iter > 0x00ffffffu ? "max_iter must be in 1 .. 2^24 - 1 (the smooth plane is 24.8 fixed point)"
                       : !q                                 ? "q is NULL"
                       : !mask && !refined                  ? "mask and refined are both NULL: nothing to write"
                                                            : nullptr;
    if (what) {
        mc::set_error_detail(std::string("mc_mandelbrot_refine_smooth: ") + what);
        return MC_ERR_INVALID_ARGUMENT;
    }
    const uint64_t count = mc::refine_smooth::refine_plane(width, height, max_iter, q, threshold, mask);
    if (refined) *refined = count;
    return MC_OK;
}
