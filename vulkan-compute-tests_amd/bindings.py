"""ctypes binding of lib/libmc_compute.so — the C ABI declared in include/mc_compute.h.

This is plumbing for tests/ and bench.py (Python drives torch.distributed and owns device tensors);
the product's host layer is the C++ code in host/.  There is NO CPU fallback: if the HIP library is
missing or no GPU is visible, the calls fail loudly.
"""
import ctypes as C
import fractions
import math
import os
import re
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MC_LIB_PATH") or os.path.join(_HERE, "lib", "libmc_compute.so")   # MC_LIB_PATH: diagnostic builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mc_compute.h")

MC_OK = 0
ABI_VERSION = 3   # MC_ABI_VERSION of include/mc_compute.h this binding is written against
PRECISION_F32, PRECISION_DS, PRECISION_F64, PRECISION_PERTURB, PRECISION_PERTURB_BLA, PRECISION_PERTURB_BLA_DEEP = 0, 1, 2, 3, 4, 5
PT_MATH_STRICT, PT_MATH_FAST, PT_MATH_FAST_CAREFUL = 0, 1, 2
MANDEL_FMA = 1
MANDEL_PERTURB_FORCE_DEEP = 4   # test switch (include/mc_compute_test.h): any bound orbit renders by the deep kernel
MANDEL_BLA_COUNT_TRIPS = 8      # test switch (include/mc_compute_test.h): PERTURB_BLA writes each pixel's loop-trip count in place of n
MANDEL_SUPERSAMPLE_ADAPTIVE = 32   # MC_MANDEL_SUPERSAMPLE_ADAPTIVE: with MANDEL_SUPERSAMPLE(s), only pixels whose count differs from a neighbour's are sampled s x s
MANDEL_COLOUR_SMOOTH = 64       # MC_MANDEL_COLOUR_SMOOTH: smooth colouring by a fractional escape count, 24.8 fixed point (include/mc_compute.h)
MANDEL_COLOUR_DISTANCE = 128    # MC_MANDEL_COLOUR_DISTANCE: the smooth colour shaded by a boundary distance estimate, whole images; set without MANDEL_COLOUR_SMOOTH
ZOOM_FILTER_BILINEAR = 0   # MC_MANDEL_ZOOM_FILTER_BILINEAR: the filtered zoom calls return what their unfiltered namesakes return
ZOOM_FILTER_AREA = 1       # MC_MANDEL_ZOOM_FILTER_AREA: a box over the pixel's footprint in the minified deep keyframe
MANDEL_COLOUR_SMOOTH_EQUALISED = 4096   # MC_MANDEL_COLOUR_SMOOTH_EQUALISED: the smooth count ranked among a whole image's escaped pixels; set without MANDEL_COLOUR_SMOOTH
MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE = 16384   # MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE: with MANDEL_SUPERSAMPLE(s) and one smooth colouring, only pixels whose smooth count is further than a threshold from a neighbour's get their s x s smooth samples
MANDEL_ADAPTIVE_SMOOTH_THRESHOLD = 256   # MC_MANDEL_ADAPTIVE_SMOOTH_THRESHOLD: the default threshold, one iteration in units of 1/256
MANDEL_SUPERSAMPLE_SMOOTH = 8192   # MC_MANDEL_SUPERSAMPLE_SMOOTH: with MANDEL_SUPERSAMPLE(s) and one smooth colouring, the s x s samples are smooth counts
MANDEL_COLOUR_EQUALISED = 16    # MC_MANDEL_COLOUR_EQUALISED: histogram-equalised colouring of a whole image (include/mc_compute.h)


BUDDHA_KERNEL_PLAIN = 1    # MC_BUDDHA_KERNEL_PLAIN: measurement bit, the device call's plain form (one sample per lane, classify then replay)
BUDDHA_CELLS_COMPLEMENT = 1   # MC_BUDDHA_CELLS_COMPLEMENT: mc_buddhabrot_importance_cells lists the cells NOT in the set
BUDDHA_KERNEL_POOLED = 2   # MC_BUDDHA_KERNEL_POOLED: measurement bit, the pooled form (a wave owns a run of samples, one loop body for both phases)


def MANDEL_SUPERSAMPLE(s):
    """MC_MANDEL_SUPERSAMPLE(s): s x s samples per pixel, resolved on the device (bits 8-11 of flags; 2, 4 or 8; 0 and 1: off)."""
    return (int(s) & 15) << 8
MANDEL_ITERS_U16 = 2   # device form: d_iters is a uint16 plane (max_iter <= 65535): the multi-GPU exchange format
PT_GENERIC_KERNEL = 1
PT_NO_BOX_KERNEL = 4    # fast math: the general slab kernel instead of the closed-box ones
PT_NO_POOL_KERNEL = 8   # fast math: the round-synchronous closed-box kernel instead of the sample-pool kernel
PT_SCENE_IN_LDS = 16    # generic scenes: records staged into LDS by every block (automatic for small scenes) ...
PT_SCENE_IN_MEMORY = 32  # ... or read where they lie (automatic for large ones); same results
PT_NO_FAST_GUARD = 64    # measurements only: fast math even on a scene classified PT_SCENE_LIGHT_ENCLOSED
PT_PREC_F32, PT_PREC_FP64, PT_PREC_DS, PT_PREC_DF64 = 0, 1, 2, 3
DS_OPS = {"add": 0, "sub": 1, "mul": 2, "compare": 3, "sqrt": 4, "df64_add": 5, "df64_mult": 6, "df64_sqrt": 7, "twoprod": 8,
          "div": 9, "twodiff": 10, "df64_eqneq": 11, "mul_fma": 12}


def pt_precision(x):
    return int(x) << 16


def pt_force_s(s):
    return int(s) << 8


class McError(RuntimeError):
    def __init__(self, status, what, detail):
        super().__init__(f"{what}: {detail[0]} (status {status}){': ' + detail[1] if detail[1] else ''}")
        self.status = status


class MandelbrotParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("max_iter", C.c_uint32), ("precision", C.c_uint32),
                ("centre_x_hi", C.c_float), ("centre_x_lo", C.c_float), ("centre_y_hi", C.c_float),
                ("centre_y_lo", C.c_float), ("scale_x_hi", C.c_float), ("scale_x_lo", C.c_float),
                ("scale_y_hi", C.c_float), ("scale_y_lo", C.c_float), ("k_color", C.c_float * 4),
                ("row_begin", C.c_uint32), ("row_end", C.c_uint32), ("row_block", C.c_uint32),
                ("row_stride", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class PathtraceParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("spp", C.c_uint32), ("sample_begin", C.c_uint32),
                ("sample_end", C.c_uint32), ("max_depth", C.c_uint32), ("row_begin", C.c_uint32),
                ("row_end", C.c_uint32), ("row_block", C.c_uint32), ("row_stride", C.c_uint32),
                ("math_mode", C.c_uint32), ("flags", C.c_uint32)]


class PathtraceKernelInfo(C.Structure):
    _fields_ = [("kernel", C.c_uint32), ("lanes_per_pixel", C.c_uint32), ("math_mode", C.c_uint32), ("launches", C.c_uint32)]


class PathtraceAccelStats(C.Structure):
    """mc_pathtrace_accel_stats (include/mc_compute.h): the shape of an mc_pathtrace_accel's tree and its two linear lists."""
    _fields_ = [("n_planes", C.c_uint32), ("n_spheres", C.c_uint32), ("nodes", C.c_uint32), ("depth", C.c_uint32), ("leaves", C.c_uint32),
                ("boxed", C.c_uint32), ("unboxed", C.c_uint32), ("device_copies", C.c_uint32), ("bytes", C.c_uint64)]


class PathtraceDenoiseParams(C.Structure):
    """mc_pathtrace_denoise_params (include/mc_compute.h): the a-trous filter's size, pass count and weights."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("passes", C.c_uint32), ("sigma_colour", C.c_float),
                ("k_normal", C.c_float), ("k_position", C.c_float), ("flags", C.c_uint32)]


class PathtraceBudgetParams(C.Structure):
    """mc_pathtrace_budget_params (include/mc_compute.h): the deepest level, the noise a pixel may keep, the noise window's radius."""
    _fields_ = [("max_level", C.c_uint32), ("target", C.c_float), ("radius", C.c_uint32), ("flags", C.c_uint32)]


class BuddhabrotParams(C.Structure):
    """mc_buddhabrot_params (include/mc_compute.h): the view, the sample window, the sample range, the plane's size, M, min_iter, seed."""
    _fields_ = [("view_centre_x", C.c_double), ("view_centre_y", C.c_double), ("view_scale_x", C.c_double), ("view_scale_y", C.c_double),
                ("sample_centre_x", C.c_double), ("sample_centre_y", C.c_double), ("sample_scale_x", C.c_double),
                ("sample_scale_y", C.c_double), ("sample_begin", C.c_uint64), ("sample_end", C.c_uint64), ("width", C.c_uint32),
                ("height", C.c_uint32), ("max_iter", C.c_uint32), ("min_iter", C.c_uint32), ("seed", C.c_uint32), ("flags", C.c_uint32)]


class BuddhabrotStats(C.Structure):
    """mc_buddhabrot_stats (include/mc_compute.h); the device form is uint64[5] in this order."""
    _fields_ = [("samples", C.c_uint64), ("skipped", C.c_uint64), ("contributing", C.c_uint64), ("points", C.c_uint64),
                ("added", C.c_uint64)]

    def as_tuple(self):
        return (self.samples, self.skipped, self.contributing, self.points, self.added)


class BuddhabrotGuideParams(C.Structure):
    """mc_buddhabrot_guide_params (include/mc_compute.h): the grid, the pilot, the list's threshold and dilation, the complement's weight."""
    _fields_ = [("grid_log2", C.c_uint32), ("dilate", C.c_uint32), ("pilot_samples", C.c_uint64), ("threshold", C.c_uint32),
                ("complement_weight", C.c_uint32)]


class BuddhabrotGuideInfo(C.Structure):
    """mc_buddhabrot_guide_info (include/mc_compute.h): what mc_buddhabrot_render_guided reports beside the render's statistics."""
    _fields_ = [("n_cells", C.c_uint32), ("n_complement", C.c_uint32), ("pilot", BuddhabrotStats), ("complement", BuddhabrotStats)]


def declared_symbols():
    """Every function name include/mc_compute.h declares (used by the export test)."""
    text = open(HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mc_[a-z0-9_]+)\s*\(", text)))


_lib = None


def lib():
    """Loads libmc_compute.so (raises if it has not been built: run __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} not built — run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        vp, u32, i32, f32 = C.c_void_p, C.c_uint32, C.c_int, C.c_float
        # The binding below is written against ABI_VERSION of include/mc_compute.h.  A diagnostic build loaded through MC_LIB_PATH may
        # be older (it then lacks the entry points added since, bound conditionally below); the shipped library must match.
        have = int(L.mc_abi_version())
        if have != ABI_VERSION and not os.environ.get("MC_LIB_PATH"):
            raise RuntimeError(f"{LIB_PATH} reports ABI version {have}, this binding is written against {ABI_VERSION}: rebuild "
                               f"(python -c 'import __graft_entry__ as g; g.build()')")
        L.mc_error_string.restype = C.c_char_p
        L.mc_error_string.argtypes = [i32]
        L.mc_last_error_detail.restype = C.c_char_p
        L.mc_device_count.argtypes = [C.POINTER(i32)]
        L.mc_context_create.argtypes = [i32, C.POINTER(vp)]
        L.mc_context_destroy.argtypes = [vp]
        L.mc_context_device_info.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(i32), C.POINTER(i32)]
        L.mc_context_synchronize.argtypes = [vp]
        L.mc_context_measure_clock.argtypes = [vp, C.POINTER(C.c_double)]
        L.mc_row_block.argtypes = []
        L.mc_row_block.restype = u32
        L.mc_tile_rows.argtypes = [u32, u32, u32, u32]
        L.mc_tile_rows.restype = u32
        L.mc_deinterleave_rows_device_async.argtypes = [vp, vp, u32, u32, u32, u32, u32, u32, vp, vp]
        L.mc_mandelbrot_assemble_device_async.argtypes = [vp, vp, vp, u32, u32, u32, u32, vp, vp, vp]
        L.mc_mandelbrot_default_params.argtypes = [u32, u32, C.POINTER(MandelbrotParams)]
        L.mc_mandelbrot_render.argtypes = [vp, C.POINTER(MandelbrotParams), vp, vp]
        if hasattr(L, "mc_mandelbrot_render_rgba8"):
            L.mc_mandelbrot_render_rgba8.argtypes = [vp, C.POINTER(MandelbrotParams), vp]
        L.mc_mandelbrot_render_device_async.argtypes = [vp, C.POINTER(MandelbrotParams), vp, vp, vp]
        L.mc_mandelbrot_colour_lut.argtypes = [u32, C.POINTER(f32), vp]
        L.mc_pathtrace_default_params.argtypes = [u32, u32, u32, C.POINTER(PathtraceParams)]
        L.mc_pathtrace_default_scene.argtypes = [C.POINTER(C.POINTER(f32)), C.POINTER(u32), C.POINTER(C.POINTER(f32)),
                                                 C.POINTER(u32)]
        L.mc_pathtrace_render.argtypes = [vp, C.POINTER(PathtraceParams), vp, u32, vp, u32, vp]
        L.mc_pathtrace_render_device_async.argtypes = [vp, C.POINTER(PathtraceParams), vp, u32, vp, u32, vp, vp]
        L.mc_convert_rgba8_device_async.argtypes = [vp, vp, u32, u32, f32, i32, vp, vp]
        L.mc_convert_rgba8.argtypes = [vp, vp, u32, u32, f32, i32, vp]
        if have >= 2 or hasattr(L, "mc_build_id"):   # (ABI 1 libraries older than round 5 lack these four)
            L.mc_build_id.restype = C.c_char_p
            L.mc_build_id.argtypes = []
            L.mc_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
            L.mc_host_free.argtypes = [vp]
            L.mc_context_last_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        if have >= 2:   # round 6
            L.mc_assemble_rgba8_device_async.argtypes = [vp, vp, u32, u32, u32, u32, u32, i32, vp, vp]
            L.mc_multi_pathtrace_render_rgba8.argtypes = [vp, C.POINTER(PathtraceParams), vp, u32, vp, u32, vp]
            L.mc_multi_mandelbrot_render_rgba8.argtypes = [vp, C.POINTER(MandelbrotParams), vp]
        if hasattr(L, "mc_mandelbrot_orbit_create"):   # MC_PRECISION_PERTURB (additions within ABI 3)
            L.mc_mandelbrot_orbit_create.argtypes = [C.c_char_p, C.c_char_p, C.c_double, C.c_double, u32, C.POINTER(vp)]
            L.mc_mandelbrot_orbit_destroy.argtypes = [vp]
            L.mc_mandelbrot_orbit_info.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
            L.mc_mandelbrot_orbit_copy.argtypes = [vp, vp]
            L.mc_context_bind_mandelbrot_orbit.argtypes = [vp, vp]
        if hasattr(L, "mc_mandelbrot_orbit_create_deep"):
            L.mc_mandelbrot_orbit_create_deep.argtypes = [C.c_char_p, C.c_char_p, C.c_double, C.c_double, C.c_int32, u32,
                                                          C.POINTER(vp)]
        if hasattr(L, "mc_mandelbrot_orbit_create_device"):   # the orbit's loop on the device
            L.mc_mandelbrot_orbit_create_device.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_double, C.c_double, C.c_int32, u32,
                                                            C.POINTER(vp)]
            L.mc_context_last_orbit_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(u32), C.POINTER(u32)]
        if hasattr(L, "mc_mandelbrot_orbit_bla"):   # MC_PRECISION_PERTURB_BLA
            L.mc_mandelbrot_orbit_bla.argtypes = [vp, C.POINTER(u32), C.POINTER(C.c_uint64)]
            L.mc_mandelbrot_orbit_bla_copy.argtypes = [vp, vp]
        if hasattr(L, "mc_mandelbrot_orbit_bla_deep"):   # MC_PRECISION_PERTURB_BLA_DEEP
            L.mc_mandelbrot_orbit_bla_deep.argtypes = [vp, C.POINTER(u32), C.POINTER(C.c_uint64)]
            L.mc_mandelbrot_orbit_bla_deep_copy.argtypes = [vp, vp, vp]
        if hasattr(L, "mc_mandelbrot_orbit_rescale"):   # dives: one shared orbit, BLA tables built on the device
            L.mc_mandelbrot_orbit_rescale.argtypes = [vp, C.c_double, C.c_double, C.c_int32, C.POINTER(vp)]
            L.mc_context_bind_mandelbrot_orbit_tables.argtypes = [vp, vp, u32]
            L.mc_context_last_table_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(u32)]
            L.mc_context_bound_bla_copy.argtypes = [vp, vp, C.POINTER(u32), C.POINTER(C.c_uint64)]
            L.mc_context_bound_bla_deep_copy.argtypes = [vp, vp, vp, C.POINTER(u32), C.POINTER(C.c_uint64)]
        if hasattr(L, "mc_mandelbrot_exact_counts"):   # exact counts of sampled pixels
            L.mc_mandelbrot_exact_pixel_offsets.argtypes = [vp, u32, u32, C.c_uint64, vp, vp, vp, vp, C.POINTER(C.c_int32)]
            L.mc_mandelbrot_exact_counts.argtypes = [vp, u32, u32, C.c_uint64, vp, vp, C.c_int32, vp]
            L.mc_mandelbrot_exact_counts_device.argtypes = [vp, vp, u32, u32, C.c_uint64, vp, vp, C.c_int32, vp]
            L.mc_context_last_exact_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32),
                                                       C.POINTER(u32)]
        if hasattr(L, "mc_mandelbrot_equalise_map"):   # MC_MANDEL_COLOUR_EQUALISED
            L.mc_mandelbrot_histogram_device_async.argtypes = [vp, vp, u32, C.c_uint64, u32, vp, vp]
            L.mc_mandelbrot_equalise_map.argtypes = [u32, vp, vp]
            L.mc_mandelbrot_recolour_device_async.argtypes = [vp, C.POINTER(MandelbrotParams), vp, u32, vp, vp, vp]
        if hasattr(L, "mc_mandelbrot_supersample_params"):   # MC_MANDEL_SUPERSAMPLE
            L.mc_mandelbrot_supersample_params.argtypes = [C.POINTER(MandelbrotParams), C.POINTER(MandelbrotParams)]
            L.mc_mandelbrot_resolve_device_async.argtypes = [vp, C.POINTER(MandelbrotParams), vp, u32, vp, vp, vp]
        if hasattr(L, "mc_context_last_refined"):   # MC_MANDEL_SUPERSAMPLE_ADAPTIVE
            L.mc_context_last_refined.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        if hasattr(L, "mc_mandelbrot_smooth_count"):   # MC_MANDEL_COLOUR_SMOOTH
            L.mc_mandelbrot_render_smooth.argtypes = [vp, C.POINTER(MandelbrotParams), vp, vp, vp]
            L.mc_mandelbrot_render_smooth_device_async.argtypes = [vp, C.POINTER(MandelbrotParams), vp, vp, vp, vp]
            L.mc_mandelbrot_smooth_count.argtypes = [u32, u32, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(u32)]
            L.mc_mandelbrot_smooth_colour.argtypes = [u32, C.POINTER(f32), vp, C.c_uint64, vp]
        if hasattr(L, "mc_mandelbrot_distance_plane"):   # MC_MANDEL_COLOUR_DISTANCE
            L.mc_mandelbrot_render_distance.argtypes = [vp, C.POINTER(MandelbrotParams), vp, vp, vp, vp]
            L.mc_mandelbrot_distance_device_async.argtypes = [vp, C.POINTER(MandelbrotParams), vp, f32, vp, vp, vp]
            L.mc_mandelbrot_distance_plane.argtypes = [u32, u32, u32, vp, vp]
            L.mc_mandelbrot_distance_colour.argtypes = [u32, C.POINTER(f32), vp, vp, C.c_uint64, f32, vp]
        if hasattr(L, "mc_mandelbrot_smooth_equalise_map"):   # MC_MANDEL_COLOUR_SMOOTH_EQUALISED
            L.mc_mandelbrot_render_smooth_equalised.argtypes = [vp, C.POINTER(MandelbrotParams), vp, vp, vp, vp]
            L.mc_mandelbrot_smooth_histogram_device_async.argtypes = [vp, vp, C.c_uint64, u32, vp, vp]
            L.mc_mandelbrot_smooth_equalise_map.argtypes = [u32, vp, vp]
            L.mc_mandelbrot_smooth_remap.argtypes = [u32, vp, vp, C.c_uint64, vp]
            L.mc_mandelbrot_smooth_remap_device_async.argtypes = [vp, C.POINTER(MandelbrotParams), vp, vp, vp, vp, vp]
        if hasattr(L, "mc_mandelbrot_resolve_smooth"):   # MC_MANDEL_SUPERSAMPLE_SMOOTH
            L.mc_mandelbrot_resolve_smooth_device_async.argtypes = [vp, C.POINTER(MandelbrotParams), vp, vp, vp, vp]
            L.mc_mandelbrot_resolve_smooth.argtypes = [u32, C.POINTER(f32), u32, u32, u32, vp, vp, vp]
        if hasattr(L, "mc_mandelbrot_refine_smooth"):   # MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE
            L.mc_mandelbrot_render_adaptive_smooth.argtypes = [vp, C.POINTER(MandelbrotParams), u32, vp, vp]
            L.mc_mandelbrot_refine_smooth.argtypes = [u32, u32, u32, vp, u32, vp, C.POINTER(C.c_uint64)]
        if hasattr(L, "mc_mandelbrot_zoom_compose"):   # zoom sequences
            dbl = C.c_double
            L.mc_mandelbrot_zoom_ratio.argtypes = [u32, u32, C.POINTER(dbl)]
            L.mc_mandelbrot_zoom_compose.argtypes = [u32, u32, vp, vp, dbl, vp, vp]
            L.mc_mandelbrot_zoom_compose_device_async.argtypes = [vp, u32, u32, vp, vp, dbl, vp, vp, vp]
            L.mc_mandelbrot_zoom_create.argtypes = [vp, u32, u32, C.POINTER(vp)]
            L.mc_mandelbrot_zoom_push.argtypes = [vp, C.POINTER(MandelbrotParams)]
            L.mc_mandelbrot_zoom_frame.argtypes = [vp, dbl, vp, vp]
            L.mc_mandelbrot_zoom_destroy.argtypes = [vp]
        if hasattr(L, "mc_mandelbrot_zoom_compose_counts"):   # zoom sequences from count keyframes
            dbl, mp = C.c_double, C.POINTER(MandelbrotParams)
            L.mc_mandelbrot_zoom_blend_map.argtypes = [u32, vp, vp, u32, u32, vp]
            L.mc_mandelbrot_zoom_compose_counts.argtypes = [mp, vp, vp, vp, dbl, vp, vp]
            L.mc_mandelbrot_zoom_compose_counts_device_async.argtypes = [vp, mp, vp, vp, vp, dbl, vp, vp, vp]
            L.mc_mandelbrot_zoom_counts_create.argtypes = [vp, u32, u32, C.POINTER(vp)]
            L.mc_mandelbrot_zoom_counts_push.argtypes = [vp, mp]
            L.mc_mandelbrot_zoom_counts_frame.argtypes = [vp, u32, u32, vp, vp]
            L.mc_mandelbrot_zoom_counts_maps.argtypes = [vp, vp, vp]
            L.mc_mandelbrot_zoom_counts_destroy.argtypes = [vp]
        if hasattr(L, "mc_mandelbrot_zoom_compose_filtered"):   # the area filter of the minified deep keyframe
            L.mc_mandelbrot_zoom_compose_filtered.argtypes = [u32, u32, vp, vp, dbl, u32, vp, vp]
            L.mc_mandelbrot_zoom_compose_filtered_device_async.argtypes = [vp, u32, u32, vp, vp, dbl, u32, vp, vp, vp]
            L.mc_mandelbrot_zoom_compose_counts_filtered.argtypes = [mp, vp, vp, vp, dbl, u32, vp, vp]
            L.mc_mandelbrot_zoom_compose_counts_filtered_device_async.argtypes = [vp, mp, vp, vp, vp, dbl, u32, vp, vp, vp]
            L.mc_mandelbrot_zoom_frame_filtered.argtypes = [vp, dbl, u32, vp, vp]
            L.mc_mandelbrot_zoom_counts_frame_filtered.argtypes = [vp, u32, u32, u32, vp, vp]
        if hasattr(L, "mc_pathtrace_denoise"):   # the path-tracer denoiser
            dp = C.POINTER(PathtraceDenoiseParams)
            L.mc_pathtrace_denoise_default_params.argtypes = [u32, u32, dp]
            L.mc_pathtrace_guides.argtypes = [u32, u32, vp, u32, vp, u32, vp, vp]
            L.mc_pathtrace_guides_device_async.argtypes = [vp, u32, u32, vp, u32, vp, u32, vp, vp, vp]
            L.mc_pathtrace_denoise.argtypes = [dp, vp, vp, vp, vp]
            L.mc_pathtrace_denoise_device_async.argtypes = [vp, dp, vp, vp, vp, vp, vp]
            L.mc_pathtrace_render_denoised.argtypes = [vp, C.POINTER(PathtraceParams), dp, vp, u32, vp, u32, vp, vp]
        if hasattr(L, "mc_pathtrace_noise"):   # the noise plane and the filter it steers
            dp = C.POINTER(PathtraceDenoiseParams)
            L.mc_pathtrace_noise_default_params.argtypes = [C.POINTER(f32), C.POINTER(u32)]
            L.mc_pathtrace_noise.argtypes = [u32, u32, vp, f32, vp, u32, vp]
            L.mc_pathtrace_noise_device_async.argtypes = [vp, u32, u32, vp, f32, vp, u32, vp, vp]
            L.mc_pathtrace_denoise_adaptive.argtypes = [dp, f32, vp, vp, vp, vp, vp]
            L.mc_pathtrace_denoise_adaptive_device_async.argtypes = [vp, dp, f32, vp, vp, vp, vp, vp, vp]
            L.mc_pathtrace_render_denoised_adaptive.argtypes = [vp, C.POINTER(PathtraceParams), dp, f32, u32, vp, u32, vp, u32, vp, vp]
        if hasattr(L, "mc_pathtrace_render_budgeted"):   # per-pixel sample budgets
            bp = C.POINTER(PathtraceBudgetParams)
            L.mc_pathtrace_budget_default_params.argtypes = [bp]
            L.mc_pathtrace_budget_levels.argtypes = [u32, u32, vp, f32, u32, vp]
            L.mc_pathtrace_budget_resolve.argtypes = [u32, u32, vp, vp, vp]
            L.mc_pathtrace_budget_levels_device_async.argtypes = [vp, u32, u32, vp, f32, u32, vp, vp]
            L.mc_pathtrace_budget_lists_device_async.argtypes = [vp, u32, u32, vp, u32, vp, vp, vp]
            L.mc_pathtrace_budget_resolve_device_async.argtypes = [vp, u32, u32, vp, vp, vp, vp]
            L.mc_pathtrace_render_list_device_async.argtypes = [vp, C.POINTER(PathtraceParams), vp, u32, vp, u32, vp, u32, f32, vp, vp]
            L.mc_pathtrace_render_budgeted.argtypes = [vp, C.POINTER(PathtraceParams), bp, vp, u32, vp, u32, vp, vp, vp]
            L.mc_context_last_budget.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        if hasattr(L, "mc_pathtrace_accel_create"):   # the path tracer through a sphere BVH
            pp, u64 = C.POINTER(PathtraceParams), C.c_uint64
            L.mc_pathtrace_accel_create.argtypes = [vp, u32, vp, u32, C.POINTER(vp)]
            L.mc_pathtrace_accel_destroy.argtypes = [vp]
            L.mc_pathtrace_accel_info.argtypes = [vp, C.POINTER(PathtraceAccelStats)]
            L.mc_pathtrace_accel_copy.argtypes = [vp, vp, u64]
            L.mc_pathtrace_accel_intersect.argtypes = [vp, u64, vp, vp, vp, vp]
            L.mc_pathtrace_accel_select_kernel.argtypes = [vp, pp, C.POINTER(PathtraceKernelInfo)]
            L.mc_pathtrace_render_accel.argtypes = [vp, vp, pp, vp]
            L.mc_pathtrace_render_accel_device_async.argtypes = [vp, vp, pp, vp, vp]
            L.mc_pathtrace_render_accel_rgba8.argtypes = [vp, vp, pp, vp]
        if hasattr(L, "mc_pathtrace_accel_guides"):   # guides, the denoised chains, the list render and the budgeted chain through the BVH
            pp, dp, bp = C.POINTER(PathtraceParams), C.POINTER(PathtraceDenoiseParams), C.POINTER(PathtraceBudgetParams)
            L.mc_pathtrace_accel_guides.argtypes = [vp, u32, u32, vp, vp]
            L.mc_pathtrace_accel_guides_device_async.argtypes = [vp, vp, u32, u32, vp, vp, vp]
            L.mc_pathtrace_render_accel_denoised.argtypes = [vp, vp, pp, dp, vp, vp]
            L.mc_pathtrace_render_accel_denoised_adaptive.argtypes = [vp, vp, pp, dp, f32, u32, vp, vp]
            L.mc_pathtrace_render_accel_list_device_async.argtypes = [vp, vp, pp, vp, u32, f32, vp, vp]
            L.mc_pathtrace_render_accel_budgeted.argtypes = [vp, vp, pp, bp, vp, vp, vp]
        if hasattr(L, "mc_buddhabrot_density"):   # the Buddhabrot
            bp, u64 = C.POINTER(BuddhabrotParams), C.c_uint64
            L.mc_buddhabrot_default_params.argtypes = [u32, u32, u64, bp]
            L.mc_buddhabrot_density.argtypes = [bp, vp, C.POINTER(BuddhabrotStats)]
            L.mc_buddhabrot_density_device_async.argtypes = [vp, bp, vp, vp, vp]
            L.mc_buddhabrot_render.argtypes = [vp, bp, vp, C.POINTER(BuddhabrotStats)]
            L.mc_buddhabrot_sqrt_map.argtypes = [u32, vp]
            L.mc_buddhabrot_tonemap.argtypes = [u32, u32, vp, vp, vp, u32, vp, vp, vp, vp]
            L.mc_buddhabrot_tonemap_device_async.argtypes = [vp, u32, u32, vp, vp, vp, u32, vp, vp, vp, vp, vp]
        if hasattr(L, "mc_buddhabrot_importance"):   # its importance map and guided sampling
            bp, sp, gp = C.POINTER(BuddhabrotParams), C.POINTER(BuddhabrotStats), C.POINTER(BuddhabrotGuideParams)
            L.mc_buddhabrot_importance.argtypes = [bp, u32, vp, vp, sp]
            L.mc_buddhabrot_importance_device_async.argtypes = [vp, bp, u32, vp, vp, vp, vp]
            L.mc_buddhabrot_importance_cells.argtypes = [u32, vp, u32, u32, u32, vp, C.POINTER(u32)]
            L.mc_buddhabrot_density_guided.argtypes = [bp, vp, u32, u32, u32, vp, sp]
            L.mc_buddhabrot_density_guided_device_async.argtypes = [vp, bp, vp, u32, u32, u32, vp, vp, vp]
            L.mc_buddhabrot_guide_default_params.argtypes = [gp]
            L.mc_buddhabrot_render_guided.argtypes = [vp, bp, gp, vp, sp, C.POINTER(BuddhabrotGuideInfo)]
        if hasattr(L, "mc_mandelbrot_render_atom"):   # atom domains: the period plane, its domains, Newton's method, the centre as text
            mp, u64, f64 = C.POINTER(MandelbrotParams), C.c_uint64, C.c_double
            L.mc_mandelbrot_render_atom.argtypes = [vp, mp, vp, vp, vp]
            L.mc_mandelbrot_render_atom_device_async.argtypes = [vp, mp, vp, vp, vp, vp]
            L.mc_mandelbrot_atom_scan.argtypes = [vp, u32, C.POINTER(u32), C.POINTER(f64)]
            L.mc_mandelbrot_atom_domains.argtypes = [vp, vp, u64, u32, vp, vp, vp]
            L.mc_mandelbrot_atom_domains_device_async.argtypes = [vp, vp, vp, u64, u32, vp, vp, vp, vp]
            L.mc_mandelbrot_nucleus_refine.argtypes = [vp, u32, u32, vp, C.POINTER(u32), vp]
            L.mc_mandelbrot_orbit_offset_text.argtypes = [vp, f64, f64, u32, C.c_char_p, C.c_char_p, C.c_size_t]
        L.mc_multi_create.argtypes = [i32, C.POINTER(vp)]
        L.mc_multi_destroy.argtypes = [vp]
        L.mc_multi_mandelbrot_render.argtypes = [vp, C.POINTER(MandelbrotParams), vp, vp]
        L.mc_multi_pathtrace_render.argtypes = [vp, C.POINTER(PathtraceParams), vp, u32, vp, u32, vp]
        _lib = L
    return _lib


_test_lib = None
TEST_LIB_PATH = os.path.join(_HERE, "lib", "libmc_compute_test.so")
TEST_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mc_compute_test.h")


def test_lib():
    """Loads libmc_compute_test.so — the device self-test hooks of the parity suite (include/mc_compute_test.h).  Test
    infrastructure: not part of the drop-in boundary, never linked by the apps."""
    global _test_lib
    if _test_lib is None:
        lib()   # the product library first (the hooks link against it; with MC_LIB_PATH the diagnostic build must be the one bound)
        if not os.path.exists(TEST_LIB_PATH):
            raise FileNotFoundError(f"{TEST_LIB_PATH} not built — run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(TEST_LIB_PATH)
        vp, i32 = C.c_void_p, C.c_int
        L.mc_test_math.argtypes = [vp, i32, i32, vp, vp, C.c_size_t]
        L.mc_test_div3.argtypes = [vp, i32, vp, vp, vp, C.c_size_t]
        L.mc_test_math_sweep.argtypes = [vp, i32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint32)]
        L.mc_test_rand01.argtypes = [vp, vp, vp, C.c_size_t]
        L.mc_test_ds_op.argtypes = [vp, i32, vp, vp, vp, C.c_size_t]
        if hasattr(L, "mc_hook_mandel_refine"):   # MC_MANDEL_SUPERSAMPLE_ADAPTIVE
            L.mc_hook_mandel_refine.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp]
        if hasattr(L, "mc_hook_orbit_mul_host"):   # mc_mandelbrot_orbit_create_device's arithmetic
            L.mc_hook_orbit_mul_host.argtypes = [i32, vp, vp, vp]
            L.mc_hook_orbit_mul_device.argtypes = [vp, i32, vp, vp, vp]
            L.mc_hook_orbit_to_double_host.argtypes = [i32, vp, i32, C.POINTER(C.c_double)]
            L.mc_hook_orbit_create_lanes_host.argtypes = [C.c_char_p, C.c_char_p, C.c_double, C.c_double, C.c_int32, C.c_uint32,
                                                          C.POINTER(vp)]
        if hasattr(L, "mc_hook_mandel_block_audit"):   # the per-lane audit of the escape loop's fast block
            L.mc_hook_mandel_block_audit.argtypes = [vp, C.POINTER(MandelbrotParams), i32, vp]
            L.mc_hook_mandel_perturb_block_audit.argtypes = [vp, vp, C.c_uint32, i32, C.c_int32, vp, vp, C.c_size_t, C.c_uint32, i32, vp]
        _test_lib = L
    return _test_lib


def declared_test_symbols():
    """Every function name include/mc_compute_test.h declares."""
    text = re.sub(r"/\*.*?\*/", "", open(TEST_HEADER_PATH).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mc_test_[a-z0-9_]+)\s*\(", text)))


def declared_hook_symbols():
    """Every mc_hook_* function name include/mc_compute_test.h declares (kernels of the product library run on a caller's data)."""
    text = re.sub(r"/\*.*?\*/", "", open(TEST_HEADER_PATH).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mc_hook_[a-z0-9_]+)\s*\(", text)))


def _check(status, what):
    if status != MC_OK:
        L = lib()
        raise McError(status, what, (L.mc_error_string(status).decode(), L.mc_last_error_detail().decode()))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def device_count():
    n = C.c_int(0)
    _check(lib().mc_device_count(C.byref(n)), "mc_device_count")
    return n.value


def default_scene():
    pp, sp = C.POINTER(C.c_float)(), C.POINTER(C.c_float)()
    np_, ns_ = C.c_uint32(0), C.c_uint32(0)
    _check(lib().mc_pathtrace_default_scene(C.byref(pp), C.byref(np_), C.byref(sp), C.byref(ns_)), "default_scene")
    planes = np.ctypeslib.as_array(pp, shape=(np_.value * 12,)).copy()
    spheres = np.ctypeslib.as_array(sp, shape=(ns_.value * 12,)).copy()
    return planes, spheres


def split_double(d):
    hi = np.float32(d)
    lo = np.float32(np.float64(d) - np.float64(hi))
    return float(hi), float(lo)


def mandelbrot_params(width, height, max_iter=128, precision=PRECISION_F32, centre=(-0.445, 0.0), scale=(2.34, 2.34),
                      k_color=(0.1, 0.7, 0.6, 0.0), row_begin=0, row_end=None, row_block=0, row_stride=0, flags=0, supersample=0,
                      adaptive=False, smooth_samples=False, adaptive_smooth=False):
    """adaptive: MANDEL_SUPERSAMPLE_ADAPTIVE beside supersample= (only pixels whose count differs from a neighbour's are sampled s x s).
    smooth_samples: MANDEL_SUPERSAMPLE_SMOOTH beside supersample= and one of MANDEL_COLOUR_SMOOTH / MANDEL_COLOUR_SMOOTH_EQUALISED in
    flags= (the samples are smooth counts, resolved over fractional counts).
    adaptive_smooth: MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE beside supersample= and one of the two smooth colourings in flags=, without the
    other two (only pixels whose smooth count is further than a threshold from a neighbour's get their s x s smooth samples)."""
    p = MandelbrotParams()
    _check(lib().mc_mandelbrot_default_params(width, height, C.byref(p)), "mc_mandelbrot_default_params")
    p.max_iter, p.precision, p.flags = max_iter, precision, flags | MANDEL_SUPERSAMPLE(supersample) | (MANDEL_SUPERSAMPLE_ADAPTIVE if adaptive else 0)
    p.flags |= MANDEL_SUPERSAMPLE_SMOOTH if smooth_samples else 0
    p.flags |= MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE if adaptive_smooth else 0
    p.centre_x_hi, p.centre_x_lo = split_double(centre[0])
    p.centre_y_hi, p.centre_y_lo = split_double(centre[1])
    p.scale_x_hi, p.scale_x_lo = split_double(scale[0])
    p.scale_y_hi, p.scale_y_lo = split_double(scale[1])
    for i in range(4):
        p.k_color[i] = k_color[i]
    p.row_begin, p.row_end = row_begin, height if row_end is None else row_end
    p.row_block, p.row_stride = row_block, row_stride
    return p


def supersample_params(p):
    """mc_mandelbrot_supersample_params (host only): the plain-render params of p's sample grid (s times the width, height and rows; the
    supersample bits, MANDEL_COLOUR_EQUALISED and MANDEL_SUPERSAMPLE_ADAPTIVE cleared; with MANDEL_SUPERSAMPLE_SMOOTH that bit cleared too and
    the colouring MANDEL_COLOUR_SMOOTH: the params of the grid's smooth render; MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE likewise)."""
    q = MandelbrotParams()
    _check(lib().mc_mandelbrot_supersample_params(C.byref(p), C.byref(q)), "mc_mandelbrot_supersample_params")
    return q


def colour_lut(max_iter, k_color=(0.1, 0.7, 0.6, 0.0)):
    """mc_mandelbrot_colour_lut (host only): float32 (max_iter + 1, 4), entry n = the vec4 written for iteration count n."""
    k = (C.c_float * 4)(*k_color)
    out = np.empty((max_iter + 1, 4), np.float32)
    _check(lib().mc_mandelbrot_colour_lut(max_iter, k, _ptr(out)), "mc_mandelbrot_colour_lut")
    return out


def equalise_map(max_iter, hist):
    """mc_mandelbrot_equalise_map (host only): the rank map uint32[max_iter + 1] of a histogram uint32[max_iter + 1]."""
    h = np.ascontiguousarray(hist, np.uint32).reshape(-1)
    if max_iter and h.size != max_iter + 1:
        raise ValueError(f"equalise_map: the histogram has {h.size} bins, max_iter + 1 = {max_iter + 1} expected")
    out = np.empty(max(h.size, 1), np.uint32)
    _check(lib().mc_mandelbrot_equalise_map(max_iter, _ptr(h), _ptr(out)), "mc_mandelbrot_equalise_map")
    return out


def buddhabrot_params(width, height, samples, max_iter=1000, min_iter=0, seed=1, view=None, sample_window=None, sample_begin=0, flags=0):
    """mc_buddhabrot_default_params, then the overrides: view and sample_window are (centre_x, centre_y, scale_x, scale_y); the range is
    [sample_begin, sample_begin + samples)."""
    p = BuddhabrotParams()
    _check(lib().mc_buddhabrot_default_params(width, height, samples, C.byref(p)), "mc_buddhabrot_default_params")
    p.max_iter, p.min_iter, p.seed, p.flags = max_iter, min_iter, seed, flags
    p.sample_begin, p.sample_end = sample_begin, sample_begin + samples
    if view is not None:
        p.view_centre_x, p.view_centre_y, p.view_scale_x, p.view_scale_y = view
    if sample_window is not None:
        p.sample_centre_x, p.sample_centre_y, p.sample_scale_x, p.sample_scale_y = sample_window
    return p


def buddhabrot_density(p, plane=None, stats=None):
    """mc_buddhabrot_density (host only): ADDS p's samples to plane (uint32 (height, width); a zeroed one when None) and to stats (a
    BuddhabrotStats; a zeroed one when None).  Returns (plane, stats)."""
    if plane is None:
        plane = np.zeros((p.height, p.width), np.uint32)
    if plane.dtype != np.uint32 or not plane.flags["C_CONTIGUOUS"] or plane.size != p.width * p.height:
        raise ValueError("buddhabrot_density: plane must be a C-contiguous uint32 array of height x width")
    if stats is None:
        stats = BuddhabrotStats()
    _check(lib().mc_buddhabrot_density(C.byref(p), _ptr(plane), C.byref(stats)), "mc_buddhabrot_density")
    return plane, stats


def buddhabrot_importance(p, grid_log2, map=None, plane=None, stats=None, want_plane=True):
    """mc_buddhabrot_importance (host only): ADDS p's samples to map (uint32[G * G], G = 2^grid_log2; a zeroed one when None), to plane
    (a zeroed one when None; no plane at all when want_plane is false) and to stats.  Returns (map, plane or None, stats)."""
    if map is None:
        map = np.zeros(1 << (2 * grid_log2), np.uint32)
    if map.dtype != np.uint32 or not map.flags["C_CONTIGUOUS"] or map.size != 1 << (2 * grid_log2):
        raise ValueError("buddhabrot_importance: map must be a C-contiguous uint32 array of G * G words")
    if want_plane and plane is None:
        plane = np.zeros((p.height, p.width), np.uint32)
    if want_plane and (plane.dtype != np.uint32 or not plane.flags["C_CONTIGUOUS"] or plane.size != p.width * p.height):
        raise ValueError("buddhabrot_importance: plane must be a C-contiguous uint32 array of height x width")
    if stats is None:
        stats = BuddhabrotStats()
    _check(lib().mc_buddhabrot_importance(C.byref(p), grid_log2, _ptr(map), _ptr(plane) if want_plane else None, C.byref(stats)),
           "mc_buddhabrot_importance")
    return map, (plane if want_plane else None), stats


def buddhabrot_importance_cells(grid_log2, map, threshold=1, dilate=0, flags=0):
    """mc_buddhabrot_importance_cells (host only): the ascending uint32 list of the cells with map >= threshold, grown by `dilate` rings;
    BUDDHA_CELLS_COMPLEMENT in flags: the cells not in that set."""
    m = np.ascontiguousarray(map, np.uint32).reshape(-1)
    if 1 <= grid_log2 <= 12 and m.size != 1 << (2 * grid_log2):
        raise ValueError(f"buddhabrot_importance_cells: the map has {m.size} words, G * G = {1 << (2 * grid_log2)} expected")
    n = C.c_uint32(0)
    _check(lib().mc_buddhabrot_importance_cells(grid_log2, _ptr(m), threshold, dilate, flags, None, C.byref(n)),
           "mc_buddhabrot_importance_cells")
    out = np.empty(n.value, np.uint32)
    _check(lib().mc_buddhabrot_importance_cells(grid_log2, _ptr(m), threshold, dilate, flags, _ptr(out), C.byref(n)),
           "mc_buddhabrot_importance_cells")
    return out


def buddhabrot_density_guided(p, cells, grid_log2, weight=1, plane=None, stats=None):
    """mc_buddhabrot_density_guided (host only): sample k in cell cells[k mod len(cells)], `weight` per plotted point.  ADDS to plane (a
    zeroed one when None) and to stats.  Returns (plane, stats)."""
    cells = np.ascontiguousarray(cells, np.uint32).reshape(-1)
    if plane is None:
        plane = np.zeros((p.height, p.width), np.uint32)
    if plane.dtype != np.uint32 or not plane.flags["C_CONTIGUOUS"] or plane.size != p.width * p.height:
        raise ValueError("buddhabrot_density_guided: plane must be a C-contiguous uint32 array of height x width")
    if stats is None:
        stats = BuddhabrotStats()
    _check(lib().mc_buddhabrot_density_guided(C.byref(p), _ptr(cells), cells.size, grid_log2, weight, _ptr(plane), C.byref(stats)),
           "mc_buddhabrot_density_guided")
    return plane, stats


def buddhabrot_guide_params(**overrides):
    """mc_buddhabrot_guide_default_params (g = 8, pilot 2^24 samples, threshold 1, dilate 1, no complement pass), then the overrides by
    field name."""
    g = BuddhabrotGuideParams()
    _check(lib().mc_buddhabrot_guide_default_params(C.byref(g)), "mc_buddhabrot_guide_default_params")
    for k, v in overrides.items():
        if k not in dict(BuddhabrotGuideParams._fields_):
            raise ValueError(f"buddhabrot_guide_params: no field {k}")
        setattr(g, k, v)
    return g


def buddhabrot_sqrt_map(levels):
    """mc_buddhabrot_sqrt_map (host only): uint32[levels + 1], map[j] = floor(levels * sqrt(j / levels)) clamped to levels."""
    out = np.empty(max(int(levels), 0) + 1, np.uint32)
    _check(lib().mc_buddhabrot_sqrt_map(levels, _ptr(out)), "mc_buddhabrot_sqrt_map")
    return out


def _tone_maps(levels, maps, what):
    out = []
    for m in maps:
        a = np.ascontiguousarray(m, np.uint32).reshape(-1)
        if a.size != levels + 1:
            raise ValueError(f"{what}: a map has {a.size} entries, levels + 1 = {levels + 1} expected")
        out.append(a)
    return out


def buddhabrot_tonemap(d0, d1, d2, levels, m0, m1, m2):
    """mc_buddhabrot_tonemap (host): float32 (height, width, 4) from three uint32 planes (which may be one array) and three maps."""
    planes = [np.ascontiguousarray(d, np.uint32) for d in (d0, d1, d2)]
    H, W = planes[0].shape
    if any(d.shape != (H, W) for d in planes):
        raise ValueError("buddhabrot_tonemap: the three planes differ in shape")
    maps = _tone_maps(levels, (m0, m1, m2), "buddhabrot_tonemap")
    out = np.empty((H, W, 4), np.float32)
    _check(lib().mc_buddhabrot_tonemap(W, H, _ptr(planes[0]), _ptr(planes[1]), _ptr(planes[2]), levels, _ptr(maps[0]), _ptr(maps[1]),
                                       _ptr(maps[2]), _ptr(out)), "mc_buddhabrot_tonemap")
    return out


def smooth_equalise_map(max_iter, hist):
    """mc_mandelbrot_smooth_equalise_map (host only): the knot map uint32[max_iter + 1] of a histogram uint32[max_iter + 1] of q >> 8."""
    h = np.ascontiguousarray(hist, np.uint32).reshape(-1)
    if max_iter and h.size != max_iter + 1:
        raise ValueError(f"smooth_equalise_map: the histogram has {h.size} bins, max_iter + 1 = {max_iter + 1} expected")
    out = np.empty(max(h.size, 1), np.uint32)
    _check(lib().mc_mandelbrot_smooth_equalise_map(max_iter, _ptr(h), _ptr(out)), "mc_mandelbrot_smooth_equalise_map")
    return out


def smooth_remap(max_iter, qmap, q):
    """mc_mandelbrot_smooth_remap (host only): q' of each smooth count q (q <= 256 * max_iter) under the knot map qmap, uint32 of q's shape."""
    m = np.ascontiguousarray(qmap, np.uint32).reshape(-1)
    if max_iter and m.size != max_iter + 1:
        raise ValueError(f"smooth_remap: the map has {m.size} knots, max_iter + 1 = {max_iter + 1} expected")
    qa = np.ascontiguousarray(q, np.uint32)
    out = np.empty(qa.shape, np.uint32)
    _check(lib().mc_mandelbrot_smooth_remap(max_iter, _ptr(m), _ptr(qa), qa.size, _ptr(out)), "mc_mandelbrot_smooth_remap")
    return out


def resolve_smooth(max_iter, s, q, qmap=None, k_color=(0.1, 0.7, 0.6, 0.0)):
    """mc_mandelbrot_resolve_smooth (host only): float32 (rows, width, 4), the s x s resolve over fractional counts of the dense smooth
    sample plane q, uint32 (rows * s, width * s), each q <= 256 * max_iter; qmap: max_iter + 1 knots for the ranked form, or None."""
    qa = np.ascontiguousarray(q, np.uint32)
    if qa.ndim != 2 or not s or qa.shape[0] % s or qa.shape[1] % s:
        raise ValueError("resolve_smooth: q is a (rows * s, width * s) plane")
    m = None
    if qmap is not None:
        m = np.ascontiguousarray(qmap, np.uint32).reshape(-1)
        if max_iter and m.size != max_iter + 1:
            raise ValueError(f"resolve_smooth: the map has {m.size} knots, max_iter + 1 = {max_iter + 1} expected")
    rows, width = qa.shape[0] // s, qa.shape[1] // s
    k = (C.c_float * 4)(*k_color)
    out = np.empty((rows, width, 4), np.float32)
    _check(lib().mc_mandelbrot_resolve_smooth(max_iter, k, s, width, rows, _ptr(qa), _ptr(m), _ptr(out)), "mc_mandelbrot_resolve_smooth")
    return out


def refine_smooth(q, max_iter, threshold=MANDEL_ADAPTIVE_SMOOTH_THRESHOLD):
    """mc_mandelbrot_refine_smooth (host only): the refine rule of MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE on the smooth plane q, uint32
    (height, width).  Returns (mask bool (height, width), refined): a pixel is refined iff its count, clamped to 256 * max_iter, is further
    than threshold (units of 1/256 iteration) from one of its up to eight neighbours'."""
    qa = np.ascontiguousarray(q, np.uint32)
    if qa.ndim != 2:
        raise ValueError("refine_smooth: q is a (height, width) plane")
    mask = np.empty(qa.shape, np.uint8)
    n = C.c_uint64(0)
    _check(lib().mc_mandelbrot_refine_smooth(qa.shape[1], qa.shape[0], max_iter, _ptr(qa), threshold, _ptr(mask), C.byref(n)),
           "mc_mandelbrot_refine_smooth")
    return mask.astype(bool), n.value


def smooth_count(n, max_iter, zx, zy, cx, cy):
    """mc_mandelbrot_smooth_count (host only): q, the 24.8 fixed-point smooth count, of each escape state.  n: the counts; (zx, zy): the z
    of the iteration that escaped; (cx, cy): the pixel's c (arrays of one shape, or scalars); returns uint32 of that shape."""
    n, zx, zy, cx, cy = np.broadcast_arrays(np.asarray(n, np.uint32), *(np.asarray(v, np.float64) for v in (zx, zy, cx, cy)))
    out = np.empty(n.shape, np.uint32)
    fn = lib().mc_mandelbrot_smooth_count
    q = C.c_uint32()
    flat = out.reshape(-1)
    for i, (a, b, c, d, e) in enumerate(zip(n.ravel().tolist(), zx.ravel().tolist(), zy.ravel().tolist(), cx.ravel().tolist(),
                                            cy.ravel().tolist())):
        _check(fn(a, max_iter, b, c, d, e, C.byref(q)), "mc_mandelbrot_smooth_count")
        flat[i] = q.value
    return out


def smooth_colour(max_iter, q, k_color=(0.1, 0.7, 0.6, 0.0)):
    """mc_mandelbrot_smooth_colour (host only): float32 (..., 4), the colour of each smooth count q (q <= 256 * max_iter)."""
    qa = np.ascontiguousarray(q, np.uint32)
    k = (C.c_float * 4)(*k_color)
    out = np.empty(qa.shape + (4,), np.float32)
    _check(lib().mc_mandelbrot_smooth_colour(max_iter, k, _ptr(qa), qa.size, _ptr(out)), "mc_mandelbrot_smooth_colour")
    return out


def distance_plane(max_iter, q):
    """mc_mandelbrot_distance_plane (host only): float32 (H, W), the distance estimate in pixel pitches of the WHOLE image's smooth plane
    q (uint32 (H, W); 256 * max_iter means interior)."""
    qa = np.ascontiguousarray(q, np.uint32)
    if qa.ndim != 2:
        raise ValueError("distance_plane: q is a (H, W) plane")
    out = np.empty(qa.shape, np.float32)
    _check(lib().mc_mandelbrot_distance_plane(qa.shape[1], qa.shape[0], max_iter, _ptr(qa), _ptr(out)), "mc_mandelbrot_distance_plane")
    return out


def distance_colour(max_iter, q, distance, threshold_px=1.0, k_color=(0.1, 0.7, 0.6, 0.0)):
    """mc_mandelbrot_distance_colour (host only): float32 (..., 4), the smooth colour of each q dimmed by min(D / threshold_px, 1)."""
    qa = np.ascontiguousarray(q, np.uint32)
    da = np.ascontiguousarray(distance, np.float32)
    if da.shape != qa.shape:
        raise ValueError("distance_colour: q and distance have one shape")
    k = (C.c_float * 4)(*k_color)
    out = np.empty(qa.shape + (4,), np.float32)
    _check(lib().mc_mandelbrot_distance_colour(max_iter, k, _ptr(qa), _ptr(da), qa.size, threshold_px, _ptr(out)),
           "mc_mandelbrot_distance_colour")
    return out


def zoom_ratio(step, steps_per_octave):
    """mc_mandelbrot_zoom_ratio (host only): r = 2^(-step / steps_per_octave), exactly 1.0 and 0.5 at the ends.  The one place a frame's r
    comes from: one bit of r changes a tap's weight."""
    r = C.c_double(0.0)
    _check(lib().mc_mandelbrot_zoom_ratio(int(step), int(steps_per_octave), C.byref(r)), "mc_mandelbrot_zoom_ratio")
    return r.value


def _keyframe(a, what):
    a = np.ascontiguousarray(a, np.float32)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"{what}: a keyframe is a float32 (H, W, 4) array")
    return a


def zoom_compose(wide, deep, r, want_rgba=True, want_rgba8=False):
    """mc_mandelbrot_zoom_compose (host only): the frame whose scale is r times the keyframe wide's, composed from wide and deep (float32
    (H, W, 4) each; deep shows half the scale, or None).  Returns (rgba float32 (H, W, 4), rgba8 uint8 (H, W, 4)), None where not wanted."""
    w = _keyframe(wide, "zoom_compose")
    d = None
    if deep is not None:
        d = _keyframe(deep, "zoom_compose")
        if d.shape != w.shape:
            raise ValueError("zoom_compose: the two keyframes have one shape")
    H, W = w.shape[:2]
    rgba = np.empty((H, W, 4), np.float32) if want_rgba else None
    rgba8 = np.empty((H, W, 4), np.uint8) if want_rgba8 else None
    _check(lib().mc_mandelbrot_zoom_compose(W, H, _ptr(w), _ptr(d), float(r), _ptr(rgba), _ptr(rgba8)), "mc_mandelbrot_zoom_compose")
    return rgba, rgba8


def zoom_compose_filtered(wide, deep, r, filter, want_rgba=True, want_rgba8=False):
    """mc_mandelbrot_zoom_compose_filtered (host only): zoom_compose with a filter, ZOOM_FILTER_BILINEAR (zoom_compose's own bits) or
    ZOOM_FILTER_AREA (a box over the footprint of the pixels that read deep)."""
    w = _keyframe(wide, "zoom_compose_filtered")
    d = None
    if deep is not None:
        d = _keyframe(deep, "zoom_compose_filtered")
        if d.shape != w.shape:
            raise ValueError("zoom_compose_filtered: the two keyframes have one shape")
    H, W = w.shape[:2]
    rgba = np.empty((H, W, 4), np.float32) if want_rgba else None
    rgba8 = np.empty((H, W, 4), np.uint8) if want_rgba8 else None
    _check(lib().mc_mandelbrot_zoom_compose_filtered(W, H, _ptr(w), _ptr(d), float(r), int(filter), _ptr(rgba), _ptr(rgba8)),
           "mc_mandelbrot_zoom_compose_filtered")
    return rgba, rgba8


def zoom_blend_map(map_wide, map_deep, step, steps_per_octave):
    """mc_mandelbrot_zoom_blend_map (host only): the moving map of a frame, (map_wide (S - s) + map_deep s) / S per entry in 64-bit integers,
    rounded down; uint32 of the maps' length."""
    a = np.ascontiguousarray(map_wide, np.uint32).reshape(-1)
    b = np.ascontiguousarray(map_deep, np.uint32).reshape(-1)
    if a.size != b.size:
        raise ValueError("zoom_blend_map: the two maps have one length")
    out = np.empty(a.size, np.uint32)
    _check(lib().mc_mandelbrot_zoom_blend_map(a.size, _ptr(a), _ptr(b), int(step), int(steps_per_octave), _ptr(out)),
           "mc_mandelbrot_zoom_blend_map")
    return out


def _count_plane(a, p, what):
    a = np.ascontiguousarray(a, np.uint32)
    if a.shape != (p.height, p.width):
        raise ValueError(f"{what}: a count keyframe is a uint32 (height, width) plane of the params' size")
    return a


def zoom_compose_counts(p, wide, deep, map, r, want_rgba=True, want_rgba8=False):
    """mc_mandelbrot_zoom_compose_counts (host only): the frame at r from the count keyframes wide and deep (uint32 (H, W): n, or q for the
    smooth colourings; deep may be None), coloured by p's colouring through map (uint32 (max_iter + 1), the equalised colourings; else
    None).  Returns (rgba float32 (H, W, 4), rgba8 uint8 (H, W, 4)), None where not wanted."""
    w = _count_plane(wide, p, "zoom_compose_counts")
    d = None if deep is None else _count_plane(deep, p, "zoom_compose_counts")
    m = None
    if map is not None:
        m = np.ascontiguousarray(map, np.uint32).reshape(-1)
        if m.size != p.max_iter + 1:
            raise ValueError(f"zoom_compose_counts: the map has {m.size} entries, max_iter + 1 = {p.max_iter + 1} expected")
    rgba = np.empty((p.height, p.width, 4), np.float32) if want_rgba else None
    rgba8 = np.empty((p.height, p.width, 4), np.uint8) if want_rgba8 else None
    _check(lib().mc_mandelbrot_zoom_compose_counts(C.byref(p), _ptr(w), _ptr(d), _ptr(m), float(r), _ptr(rgba), _ptr(rgba8)),
           "mc_mandelbrot_zoom_compose_counts")
    return rgba, rgba8


def zoom_compose_counts_filtered(p, wide, deep, map, r, filter, want_rgba=True, want_rgba8=False):
    """mc_mandelbrot_zoom_compose_counts_filtered (host only): zoom_compose_counts with a filter (ZOOM_FILTER_BILINEAR, ZOOM_FILTER_AREA)."""
    w = _count_plane(wide, p, "zoom_compose_counts_filtered")
    d = None if deep is None else _count_plane(deep, p, "zoom_compose_counts_filtered")
    m = None
    if map is not None:
        m = np.ascontiguousarray(map, np.uint32).reshape(-1)
        if m.size != p.max_iter + 1:
            raise ValueError(f"zoom_compose_counts_filtered: the map has {m.size} entries, max_iter + 1 = {p.max_iter + 1} expected")
    rgba = np.empty((p.height, p.width, 4), np.float32) if want_rgba else None
    rgba8 = np.empty((p.height, p.width, 4), np.uint8) if want_rgba8 else None
    _check(lib().mc_mandelbrot_zoom_compose_counts_filtered(C.byref(p), _ptr(w), _ptr(d), _ptr(m), float(r), int(filter), _ptr(rgba),
                                                            _ptr(rgba8)), "mc_mandelbrot_zoom_compose_counts_filtered")
    return rgba, rgba8


def pathtrace_params(width, height, spp, math_mode=PT_MATH_STRICT, sample_begin=0, sample_end=None, max_depth=12,
                     row_begin=0, row_end=None, row_block=0, row_stride=0, flags=0):
    p = PathtraceParams()
    _check(lib().mc_pathtrace_default_params(width, height, spp, C.byref(p)), "mc_pathtrace_default_params")
    p.math_mode, p.sample_begin, p.max_depth = math_mode, sample_begin, max_depth
    p.sample_end = spp if sample_end is None else sample_end
    p.row_begin, p.row_end = row_begin, height if row_end is None else row_end
    p.row_block, p.row_stride = row_block, row_stride
    p.flags = flags
    return p


def pathtrace_denoise_params(width, height, passes=None, sigma_colour=None, k_normal=None, k_position=None, flags=0):
    """mc_pathtrace_denoise_default_params (passes 5, sigma_colour 128, k_normal 8, k_position 4), then the values given."""
    d = PathtraceDenoiseParams()
    _check(lib().mc_pathtrace_denoise_default_params(width, height, C.byref(d)), "mc_pathtrace_denoise_default_params")
    if passes is not None:
        d.passes = passes
    if sigma_colour is not None:
        d.sigma_colour = sigma_colour
    if k_normal is not None:
        d.k_normal = k_normal
    if k_position is not None:
        d.k_position = k_position
    d.flags = flags
    return d


def _scene_tables(planes, spheres):
    if planes is None or spheres is None:
        planes, spheres = default_scene()
    return np.ascontiguousarray(planes, np.float32).reshape(-1), np.ascontiguousarray(spheres, np.float32).reshape(-1)


def pathtrace_guides(width, height, planes=None, spheres=None):
    """mc_pathtrace_guides (host only): what the centre ray of each pixel hits, as two float32 (height, width, 4) planes in storage order:
    normal_t = (nl, t) and position_id = (x, id); a miss is (0, 0, 0, 1e20) and (0, 0, 0, -1)."""
    planes, spheres = _scene_tables(planes, spheres)
    nt = np.empty((height, width, 4), np.float32)
    pid = np.empty((height, width, 4), np.float32)
    _check(lib().mc_pathtrace_guides(width, height, _ptr(planes), planes.size // 12, _ptr(spheres), spheres.size // 12, _ptr(nt), _ptr(pid)),
           "mc_pathtrace_guides")
    return nt, pid


def pathtrace_denoise(d, rgba, normal_t, position_id):
    """mc_pathtrace_denoise (host only): the a-trous filter of d over the float32 (height, width, 4) plane rgba, steered by the guide planes."""
    shape = (d.height, d.width, 4)
    arrs = [np.ascontiguousarray(a, np.float32) for a in (rgba, normal_t, position_id)]
    for a in arrs:
        if a.shape != shape:
            raise ValueError(f"pathtrace_denoise: every plane is float32 of shape {shape}, got {a.shape}")
    out = np.empty(shape, np.float32)
    _check(lib().mc_pathtrace_denoise(C.byref(d), _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]), _ptr(out)), "mc_pathtrace_denoise")
    return out


def pathtrace_noise_defaults():
    """mc_pathtrace_noise_default_params: (k_noise, radius), 4.0 and 3."""
    k, r = C.c_float(0.0), C.c_uint32(0)
    _check(lib().mc_pathtrace_noise_default_params(C.byref(k), C.byref(r)), "mc_pathtrace_noise_default_params")
    return k.value, r.value


def pathtrace_noise(half, scale, full, radius=None):
    """mc_pathtrace_noise (host only): the float32 (height, width) noise plane of a render from half, the linear accumulator after its
    first h samples, and full, its finished buffer (float32 (height, width, 4) each); scale = spp / h."""
    h, f = np.ascontiguousarray(half, np.float32), np.ascontiguousarray(full, np.float32)
    if h.ndim != 3 or h.shape[2] != 4 or f.shape != h.shape:
        raise ValueError("pathtrace_noise: half and full are float32 (height, width, 4) arrays of one shape")
    if radius is None:
        radius = pathtrace_noise_defaults()[1]
    out = np.empty(h.shape[:2], np.float32)
    _check(lib().mc_pathtrace_noise(h.shape[1], h.shape[0], _ptr(h), scale, _ptr(f), radius, _ptr(out)), "mc_pathtrace_noise")
    return out


def pathtrace_denoise_adaptive(d, rgba, normal_t, position_id, variance, k_noise=None):
    """mc_pathtrace_denoise_adaptive (host only): pathtrace_denoise with the colour tolerance taken per pixel from the float32
    (height, width) plane variance and k_noise (default: mc_pathtrace_noise_default_params'); d.sigma_colour is not used."""
    shape = (d.height, d.width, 4)
    arrs = [np.ascontiguousarray(a, np.float32) for a in (rgba, normal_t, position_id)]
    var = np.ascontiguousarray(variance, np.float32)
    if any(a.shape != shape for a in arrs) or var.shape != shape[:2]:
        raise ValueError(f"pathtrace_denoise_adaptive: the planes are float32 of shape {shape}, the variance of shape {shape[:2]}")
    if k_noise is None:
        k_noise = pathtrace_noise_defaults()[0]
    out = np.empty(shape, np.float32)
    _check(lib().mc_pathtrace_denoise_adaptive(C.byref(d), k_noise, _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]), _ptr(var), _ptr(out)),
           "mc_pathtrace_denoise_adaptive")
    return out


def pathtrace_budget_params(max_level=None, target=None, radius=None, flags=0):
    """mc_pathtrace_budget_default_params (max_level 4, target 32, radius 3), then the values given."""
    b = PathtraceBudgetParams()
    _check(lib().mc_pathtrace_budget_default_params(C.byref(b)), "mc_pathtrace_budget_default_params")
    if max_level is not None:
        b.max_level = max_level
    if target is not None:
        b.target = target
    if radius is not None:
        b.radius = radius
    b.flags = flags
    return b


def pathtrace_budget_levels(variance, target, max_level):
    """mc_pathtrace_budget_levels (host only): the uint8 (height, width) level plane of the float32 (height, width) noise plane; a pixel of
    level l is worth n0 << l samples."""
    v = np.ascontiguousarray(variance, np.float32)
    if v.ndim != 2:
        raise ValueError("pathtrace_budget_levels: variance is a float32 (height, width) array")
    out = np.empty(v.shape, np.uint8)
    _check(lib().mc_pathtrace_budget_levels(v.shape[1], v.shape[0], _ptr(v), target, max_level, _ptr(out)), "mc_pathtrace_budget_levels")
    return out


def pathtrace_budget_resolve(acc, levels, in_place=False):
    """mc_pathtrace_budget_resolve (host only): the encoded float32 (height, width, 4) buffer of the linear accumulator plane acc and the
    uint8 (height, width) level plane.  in_place: acc (a contiguous float32 array) is overwritten and returned."""
    a = acc if in_place else np.ascontiguousarray(acc, np.float32)
    lv = np.ascontiguousarray(levels, np.uint8)
    if a.dtype != np.float32 or not a.flags.c_contiguous or a.ndim != 3 or a.shape[2] != 4 or lv.shape != a.shape[:2]:
        raise ValueError("pathtrace_budget_resolve: acc is a contiguous float32 (height, width, 4) array, levels uint8 (height, width)")
    out = a if in_place else np.empty(a.shape, np.float32)
    _check(lib().mc_pathtrace_budget_resolve(a.shape[1], a.shape[0], _ptr(a), _ptr(lv), _ptr(out)), "mc_pathtrace_budget_resolve")
    return out


def tile_rows(p):
    return int(lib().mc_tile_rows(p.row_begin, p.row_end, p.row_block, p.row_stride))


PT_SCENE_SLAB, PT_SCENE_LIGHTS_INSIDE, PT_SCENE_SPHERES_DISJOINT, PT_SCENE_LIGHT_ENCLOSED, PT_SCENE_MANY_SPHERES = 1, 2, 4, 8, 16
PT_SCENE_SPECULAR = 32
PT_KERNEL_GENERIC, PT_KERNEL_SLAB, PT_KERNEL_BOX, PT_KERNEL_POOL, PT_KERNEL_GENERIC_MEMORY = 0, 1, 3, 4, 5
PT_KERNEL_BVH = 6
PT_KERNEL_NAMES = {0: "generic", 1: "slab", 3: "box", 4: "pool", 5: "generic_memory", 6: "bvh"}


def pathtrace_select_kernel(p, planes=None, spheres=None):
    """mc_pathtrace_select_kernel: the kernel a render call with these parameters and this scene runs (no device needed)."""
    if planes is None or spheres is None:
        planes, spheres = default_scene()
    planes = np.ascontiguousarray(planes, np.float32).reshape(-1, 12)
    spheres = np.ascontiguousarray(spheres, np.float32).reshape(-1, 12)
    out = PathtraceKernelInfo()
    fn = lib().mc_pathtrace_select_kernel
    fn.argtypes = [C.POINTER(PathtraceParams), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(PathtraceKernelInfo)]
    _check(fn(C.byref(p), _ptr(planes), planes.shape[0], _ptr(spheres), spheres.shape[0], C.byref(out)), "mc_pathtrace_select_kernel")
    return out


class PathtraceAccel:
    """mc_pathtrace_accel: a scene's tables and the BVH over its spheres (host only: no device is needed to make or query one).
    Context.pathtrace_accel / pathtrace_accel_device / pathtrace_accel_rgba8 render through it."""

    def __init__(self, planes=None, spheres=None):
        self._h = C.c_void_p()
        if planes is None or spheres is None:
            planes, spheres = default_scene()
        planes = np.ascontiguousarray(planes, np.float32).reshape(-1)
        spheres = np.ascontiguousarray(spheres, np.float32).reshape(-1)
        self.n_planes, self.n_spheres = planes.size // 12, spheres.size // 12
        _check(lib().mc_pathtrace_accel_create(_ptr(planes), self.n_planes, _ptr(spheres), self.n_spheres, C.byref(self._h)),
               "mc_pathtrace_accel_create")

    def info(self):
        st = PathtraceAccelStats()
        _check(lib().mc_pathtrace_accel_info(self._h, C.byref(st)), "mc_pathtrace_accel_info")
        return {name: int(getattr(st, name)) for name, _ in PathtraceAccelStats._fields_}

    def bytes(self):
        """The structure's bytes (nodes, leaf spheres, leaf indices, unboxed list): equal for equal tables."""
        out = np.zeros(self.info()["bytes"], np.uint8)
        _check(lib().mc_pathtrace_accel_copy(self._h, _ptr(out), out.size), "mc_pathtrace_accel_copy")
        return out

    def intersect(self, origins, dirs):
        """mc_pathtrace_accel_intersect: (id, t) per ray, id int32 (-1: miss), t float32; origins and dirs are (n, 3) float32."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError("PathtraceAccel.intersect: origins and dirs must have the same shape")
        ids = np.empty(o.shape[0], np.int32)
        t = np.empty(o.shape[0], np.float32)
        _check(lib().mc_pathtrace_accel_intersect(self._h, o.shape[0], _ptr(o), _ptr(d), _ptr(ids), _ptr(t)), "mc_pathtrace_accel_intersect")
        return ids, t

    def select_kernel(self, p):
        out = PathtraceKernelInfo()
        _check(lib().mc_pathtrace_accel_select_kernel(self._h, C.byref(p), C.byref(out)), "mc_pathtrace_accel_select_kernel")
        return out

    def guides(self, width, height):
        """mc_pathtrace_accel_guides: the planes of pathtrace_guides for the object's tables, through the tree (host only)."""
        nt = np.empty((height, width, 4), np.float32)
        pid = np.empty((height, width, 4), np.float32)
        _check(lib().mc_pathtrace_accel_guides(self._h, width, height, _ptr(nt), _ptr(pid)), "mc_pathtrace_accel_guides")
        return nt, pid

    def close(self):
        if self._h:
            _check(lib().mc_pathtrace_accel_destroy(self._h), "mc_pathtrace_accel_destroy")
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def build_id():
    """mc_build_id as a dict: {"pt": ..., "mandel": ..., "lib": ...} (source hashes of the loaded library's kernel families)."""
    return dict(kv.split("=") for kv in lib().mc_build_id().decode().split())


class HostBuffer:
    """Page-locked host memory from mc_host_alloc, exposed as a numpy array (the storage buffer an application owns)."""

    def __init__(self, shape, dtype=np.float32):
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self._p = C.c_void_p()
        _check(lib().mc_host_alloc(self.nbytes, C.byref(self._p)), "mc_host_alloc")
        self.array = np.frombuffer((C.c_char * self.nbytes).from_address(self._p.value), dtype=dtype).reshape(shape)

    def free(self):
        if self._p:
            self.array = None
            _check(lib().mc_host_free(self._p), "mc_host_free")
            self._p = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()

    def __del__(self):   # (views handed out earlier dangle once the buffer is freed: keep the HostBuffer alive while `array` is in use)
        try:
            self.free()
        except Exception:
            pass


def _check_out(out, shape, what):
    """The caller's own output array goes to the library as a bare pointer: it must be exactly the buffer the call fills."""
    if not isinstance(out, np.ndarray) or out.dtype != np.float32 or tuple(out.shape) != tuple(shape):
        raise ValueError(f"{what}: out must be a float32 array of shape {tuple(shape)}, got "
                         f"{getattr(out, 'dtype', type(out))} {getattr(out, 'shape', '')}")
    if not out.flags.c_contiguous or not out.flags.writeable:
        raise ValueError(f"{what}: out must be C-contiguous and writeable")


def pathtrace_scene_class(planes, spheres):
    """mc_pathtrace_scene_class: which kernel specialisations the host would select for this scene (no device needed)."""
    planes = np.ascontiguousarray(planes, np.float32).reshape(-1, 12)
    spheres = np.ascontiguousarray(spheres, np.float32).reshape(-1, 12)
    out = C.c_uint32(0)
    fn = lib().mc_pathtrace_scene_class
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    _check(fn(_ptr(planes), planes.shape[0], _ptr(spheres), spheres.shape[0], C.byref(out)), "mc_pathtrace_scene_class")
    return int(out.value)


def scale_from_text(text):
    """A decimal scale as (mantissa, exp2) with text = mantissa * 2^exp2 to the nearest double mantissa (ties to even), the mantissa in
    [0.5, 1] in magnitude: any depth, far below the doubles (the scale arguments of Orbit(..., scale_exp2=...))."""
    v = fractions.Fraction(text.strip())
    if v == 0:
        raise ValueError(f"scale_from_text: {text!r} is zero")
    a = abs(v)
    e = a.numerator.bit_length() - a.denominator.bit_length()   # 2^(e-1) <= a < 2^(e+1)
    if a >= fractions.Fraction(2) ** e:
        e += 1                                                    # now 2^(e-1) <= a < 2^e
    m = float(a / fractions.Fraction(2) ** e)                     # correctly rounded (int / int true division)
    return (-m if v < 0 else m), e


ORBIT_TABLE_BLA = 1 << 0        # mc_context_bind_mandelbrot_orbit_tables: the tables to build on the device
ORBIT_TABLE_BLA_DEEP = 1 << 1


def atom_scan(z):
    """mc_mandelbrot_atom_scan: (period, amin) of the sequence z_1 .. z_n, an (n, 2) float64 array (re, im), by the update the atom
    kernels compile.  Host only."""
    z = np.ascontiguousarray(z, np.float64).reshape(-1, 2)
    per, best = C.c_uint32(0), C.c_double(0.0)
    _check(lib().mc_mandelbrot_atom_scan(_ptr(z) if len(z) else None, len(z), C.byref(per), C.byref(best)), "mc_mandelbrot_atom_scan")
    return per.value, best.value


def atom_domains(period, amin, max_iter):
    """mc_mandelbrot_atom_domains: (count uint32, amin float64, pixel uint32), max_iter + 1 entries each, of a period plane and its amin
    plane (any shape, the linear index is the flattened one).  Host only."""
    period, amin = np.ascontiguousarray(period, np.uint32).ravel(), np.ascontiguousarray(amin, np.float64).ravel()
    if period.size != amin.size:
        raise ValueError("atom_domains: the two planes differ in size")
    n = int(max_iter) + 1
    count, tab, pixel = np.empty(n, np.uint32), np.empty(n, np.float64), np.empty(n, np.uint32)
    _check(lib().mc_mandelbrot_atom_domains(_ptr(period) if period.size else _ptr(count), _ptr(amin) if amin.size else _ptr(tab), period.size,
                                            int(max_iter), _ptr(count), _ptr(tab), _ptr(pixel)), "mc_mandelbrot_atom_domains")
    return count, tab, pixel


def bla_table_group_entries():
    """MC_BLA_TABLE_GROUP_ENTRIES of include/mc_compute_test.h: the device table build's single-workgroup threshold."""
    return int(re.search(r"#define\s+MC_BLA_TABLE_GROUP_ENTRIES\s+(\d+)u", open(TEST_HEADER_PATH).read()).group(1))


class Orbit:
    """mc_mandelbrot_orbit: the reference orbit of MC_PRECISION_PERTURB, computed on the host (no device needed) from the centre as
    decimal text (str, taken verbatim) and the scale as doubles.  A context manager; Context.bind_mandelbrot_orbit copies it to a device.
    scale_exp2=None: mc_mandelbrot_orbit_create.  An integer: mc_mandelbrot_orbit_create_deep, the scale (scale_x, scale_y) * 2^scale_exp2
    (scale_from_text makes the pair from text).  `deep`: the orbit renders by the rescaled loop (min |scale| < 2^-960); then `scale`
    holds the mantissas and `scale_exp2` the exponent, otherwise `scale` holds the doubles and `scale_exp2` is 0 (or None).
    device=ctx (with an integer scale_exp2): mc_mandelbrot_orbit_create_device, the same object with its iteration loop run on that
    context's device; Context.last_orbit_timing() then reports it."""

    def __init__(self, centre_x, centre_y, scale_x, scale_y, max_iter, scale_exp2=None, device=None):
        enc = lambda v: v.encode() if isinstance(v, str) else v
        self._h = C.c_void_p()
        self.deep = False
        if device is not None and scale_exp2 is None:
            raise ValueError("Orbit: device= takes the scale as (scale_x, scale_y) * 2^scale_exp2; pass scale_exp2 (0 for plain doubles)")
        if scale_exp2 is None:
            _check(lib().mc_mandelbrot_orbit_create(enc(centre_x), enc(centre_y), float(scale_x), float(scale_y), int(max_iter),
                                                    C.byref(self._h)), "mc_mandelbrot_orbit_create")
            self.scale = (float(scale_x), float(scale_y))
        else:
            E = int(scale_exp2)
            if device is not None:
                _check(lib().mc_mandelbrot_orbit_create_device(device._h, enc(centre_x), enc(centre_y), float(scale_x), float(scale_y), E,
                                                               int(max_iter), C.byref(self._h)), "mc_mandelbrot_orbit_create_device")
            else:
                _check(lib().mc_mandelbrot_orbit_create_deep(enc(centre_x), enc(centre_y), float(scale_x), float(scale_y), E,
                                                             int(max_iter), C.byref(self._h)), "mc_mandelbrot_orbit_create_deep")
            self._set_scale(scale_x, scale_y, E)
            E = self.scale_exp2
        self.scale_exp2 = None if scale_exp2 is None else E
        self._read_info()

    def _set_scale(self, scale_x, scale_y, E):
        """The attributes of an object made for (scale_x, scale_y) * 2^E, as the deep constructor stores the scale."""
        emin = min(math.frexp(abs(float(scale_x))), math.frexp(abs(float(scale_y))), key=lambda fe: (fe[1], fe[0]))[1] + E
        self.deep = emin < -959
        if self.deep:
            self.scale, self.scale_exp2 = (float(scale_x), float(scale_y)), E
        else:
            self.scale, self.scale_exp2 = (math.ldexp(float(scale_x), E), math.ldexp(float(scale_y), E)), 0

    def _read_info(self):
        n, m, b = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        _check(lib().mc_mandelbrot_orbit_info(self._h, C.byref(n), C.byref(m), C.byref(b)), "mc_mandelbrot_orbit_info")
        self.length, self.max_iter, self.bits = n.value, m.value, b.value

    def rescale(self, scale_x, scale_y, scale_exp2=0):
        """mc_mandelbrot_orbit_rescale: a new Orbit with this one's table under the scale (scale_x, scale_y) * 2^scale_exp2 of the same
        centre (no BLA table; this object is untouched).  Refused when the new scale asks for more bits than this orbit carries."""
        h = C.c_void_p()
        _check(lib().mc_mandelbrot_orbit_rescale(self._h, float(scale_x), float(scale_y), int(scale_exp2), C.byref(h)),
               "mc_mandelbrot_orbit_rescale")
        o = Orbit.__new__(Orbit)
        o._h = h
        o._set_scale(scale_x, scale_y, int(scale_exp2))
        o._read_info()
        return o

    def table(self):
        """Z_0 .. Z_L as an (L + 1, 2) float64 array (re, im)."""
        out = np.empty((self.length + 1, 2), np.float64)
        _check(lib().mc_mandelbrot_orbit_copy(self._h, _ptr(out)), "mc_mandelbrot_orbit_copy")
        return out

    def bla(self):
        """mc_mandelbrot_orbit_bla: build the BLA table of MC_PRECISION_PERTURB_BLA once (kept in the orbit; bind afterwards).
        Returns (levels, entries)."""
        lv, n = C.c_uint32(0), C.c_uint64(0)
        _check(lib().mc_mandelbrot_orbit_bla(self._h, C.byref(lv), C.byref(n)), "mc_mandelbrot_orbit_bla")
        self.bla_levels, self.bla_entries = lv.value, n.value
        return lv.value, n.value

    def bla_table(self):
        """The BLA table as an (entries, 5) float64 array, level-major, (A.x, A.y, B.x, B.y, R) per entry (after bla())."""
        if not hasattr(self, "bla_entries"):
            raise ValueError("Orbit.bla_table: call bla() first")
        out = np.empty((self.bla_entries, 5), np.float64)
        _check(lib().mc_mandelbrot_orbit_bla_copy(self._h, _ptr(out)), "mc_mandelbrot_orbit_bla_copy")
        return out

    def bla_deep(self):
        """mc_mandelbrot_orbit_bla_deep: build the floatexp BLA table of MC_PRECISION_PERTURB_BLA_DEEP once (kept in the orbit beside any
        bla() table; bind afterwards).  Returns (levels, entries)."""
        lv, n = C.c_uint32(0), C.c_uint64(0)
        _check(lib().mc_mandelbrot_orbit_bla_deep(self._h, C.byref(lv), C.byref(n)), "mc_mandelbrot_orbit_bla_deep")
        self.bla_deep_levels, self.bla_deep_entries = lv.value, n.value
        return lv.value, n.value

    def bla_deep_table(self):
        """The floatexp table as (mantissas (entries, 5) float64: A.x, A.y, B.x, B.y, R; exponents (entries, 3) int32: e_A, e_B, e_R),
        level-major as bla_table() (after bla_deep())."""
        if not hasattr(self, "bla_deep_entries"):
            raise ValueError("Orbit.bla_deep_table: call bla_deep() first")
        mant = np.empty((self.bla_deep_entries, 5), np.float64)
        exps = np.empty((self.bla_deep_entries, 3), np.int32)
        _check(lib().mc_mandelbrot_orbit_bla_deep_copy(self._h, _ptr(mant), _ptr(exps)), "mc_mandelbrot_orbit_bla_deep_copy")
        return mant, exps

    def exact_pixel_offsets(self, width, height, pixels):
        """mc_mandelbrot_exact_pixel_offsets: (dcx, dcy, dc_exp2) of the pixels ((gx, gy) pairs, an (N, 2) array) of the width x height
        view of this orbit: the offsets the perturbation kernels use, two float64 arrays and the exponent they share."""
        px = np.ascontiguousarray(pixels, np.uint32).reshape(-1, 2)
        gx, gy = np.ascontiguousarray(px[:, 0]), np.ascontiguousarray(px[:, 1])
        dcx, dcy, e = np.empty(len(px), np.float64), np.empty(len(px), np.float64), C.c_int32(0)
        _check(lib().mc_mandelbrot_exact_pixel_offsets(self._h, int(width), int(height), len(px), _ptr(gx), _ptr(gy), _ptr(dcx), _ptr(dcy),
                                                       C.byref(e)), "mc_mandelbrot_exact_pixel_offsets")
        return dcx, dcy, e.value

    def exact_counts(self, max_iter, dcx, dcy, dc_exp2=0, extra_limbs=0, device=None):
        """mc_mandelbrot_exact_counts: the exact count of c = c_ref + (dcx[i], dcy[i]) * 2^dc_exp2 for every i, a uint32 array; on the
        host, serially, or (device=ctx) mc_mandelbrot_exact_counts_device, the same integers from that context's device."""
        dcx, dcy = np.ascontiguousarray(dcx, np.float64).ravel(), np.ascontiguousarray(dcy, np.float64).ravel()
        if dcx.size != dcy.size:
            raise ValueError("Orbit.exact_counts: dcx and dcy differ in length")
        out = np.empty(dcx.size, np.uint32)
        if device is None:
            _check(lib().mc_mandelbrot_exact_counts(self._h, int(max_iter), int(extra_limbs), dcx.size, _ptr(dcx), _ptr(dcy), int(dc_exp2),
                                                    _ptr(out)), "mc_mandelbrot_exact_counts")
        else:
            _check(lib().mc_mandelbrot_exact_counts_device(device._h, self._h, int(max_iter), int(extra_limbs), dcx.size, _ptr(dcx),
                                                           _ptr(dcy), int(dc_exp2), _ptr(out)), "mc_mandelbrot_exact_counts_device")
        return out

    def nucleus_refine(self, period, offset, max_steps=64):
        """mc_mandelbrot_nucleus_refine: Newton's method on z_period(c_ref + offset) = 0 from offset = (ox, oy), in PERTURB's dc units.
        Returns ((ox, oy) refined, steps taken, (qx, qy) the last step)."""
        off, last, steps = np.array(offset, np.float64).reshape(2), np.zeros(2, np.float64), C.c_uint32(0)
        _check(lib().mc_mandelbrot_nucleus_refine(self._h, int(period), int(max_steps), _ptr(off), C.byref(steps), _ptr(last)),
               "mc_mandelbrot_nucleus_refine")
        return (float(off[0]), float(off[1])), steps.value, (float(last[0]), float(last[1]))

    def offset_text(self, ox, oy, frac_digits, capacity=None):
        """mc_mandelbrot_orbit_offset_text: c_ref + (ox, oy) (a deep orbit: (ox, oy) * 2^scale_exp2), summed exactly, as two decimal strings
        with frac_digits fractional digits, truncated toward zero.  capacity=None: large enough."""
        cap = int(frac_digits) + 32 if capacity is None else int(capacity)
        bx, by = C.create_string_buffer(max(cap, 1)), C.create_string_buffer(max(cap, 1))
        _check(lib().mc_mandelbrot_orbit_offset_text(self._h, float(ox), float(oy), int(frac_digits), bx, by, cap),
               "mc_mandelbrot_orbit_offset_text")
        return bx.value.decode(), by.value.decode()

    def close(self):
        if self._h:
            lib().mc_mandelbrot_orbit_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """mc_context wrapper (replaces VulkanComputeApp::init / cleanup)."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        _check(lib().mc_context_create(device, C.byref(self._h)), "mc_context_create")
        self.device = device
        self._zooms = []   # weak references to the Zoom objects made on this context: closed with it, before it

    def close(self):
        if self._h:
            for ref in getattr(self, "_zooms", []):   # their device slots are freed while the context still exists
                z = ref()
                if z is not None:
                    z.close()
            self._zooms = []
            lib().mc_context_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_info(self):
        name = C.create_string_buffer(256)
        cu, clk = C.c_int(0), C.c_int(0)
        _check(lib().mc_context_device_info(self._h, name, 256, C.byref(cu), C.byref(clk)), "mc_context_device_info")
        return name.value.decode(), cu.value, clk.value

    def measure_clock(self):
        """Shader clock (MHz) under full fp32 VALU load, measured in-kernel."""
        mhz = C.c_double(0.0)
        _check(lib().mc_context_measure_clock(self._h, C.byref(mhz)), "mc_context_measure_clock")
        return mhz.value

    def synchronize(self):
        _check(lib().mc_context_synchronize(self._h), "mc_context_synchronize")

    def last_timing(self):
        """(kernel_ms, copy_ms) of the last blocking host-buffer call on this context (mc_context_last_timing)."""
        k, c = C.c_double(0.0), C.c_double(0.0)
        _check(lib().mc_context_last_timing(self._h, C.byref(k), C.byref(c)), "mc_context_last_timing")
        return k.value, c.value

    def last_orbit_timing(self):
        """(device_ms, launches, limbs) of the last successful Orbit(..., device=this context) (mc_context_last_orbit_timing)."""
        ms, n, k1 = C.c_double(0), C.c_uint32(0), C.c_uint32(0)
        _check(lib().mc_context_last_orbit_timing(self._h, C.byref(ms), C.byref(n), C.byref(k1)), "mc_context_last_orbit_timing")
        return ms.value, n.value, k1.value

    def exact_counts(self, orbit, width, height, pixels, max_iter, extra_limbs=0, device=True):
        """The exact counts of the pixels ((gx, gy) pairs) of the width x height view of `orbit` (uint32, one per pixel): the offsets of
        mc_mandelbrot_exact_pixel_offsets iterated by mc_mandelbrot_exact_counts_device on this context, or (device=False) by the
        serial host call."""
        dcx, dcy, e = orbit.exact_pixel_offsets(width, height, pixels)
        return orbit.exact_counts(max_iter, dcx, dcy, e, extra_limbs, device=self if device else None)

    EXACT_KERNEL_WAVE, EXACT_KERNEL_WORKGROUP = 1, 2

    def last_exact_timing(self):
        """(device_ms, launches, limbs, iters_per_launch, kernel) of the last successful device exact-count call of this context
        (mc_context_last_exact_timing); kernel is EXACT_KERNEL_WAVE or EXACT_KERNEL_WORKGROUP."""
        ms, n, k1, it, kind = C.c_double(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        _check(lib().mc_context_last_exact_timing(self._h, C.byref(ms), C.byref(n), C.byref(k1), C.byref(it), C.byref(kind)),
               "mc_context_last_exact_timing")
        return ms.value, n.value, k1.value, it.value, kind.value

    def last_refined(self):
        """(refined, pixels) of the last successful adaptive render on this context (mc_context_last_refined)."""
        r, n = C.c_uint64(0), C.c_uint64(0)
        _check(lib().mc_context_last_refined(self._h, C.byref(r), C.byref(n)), "mc_context_last_refined")
        return r.value, n.value

    def bind_mandelbrot_orbit(self, orbit, device_tables=None):
        """mc_context_bind_mandelbrot_orbit: the view of MC_PRECISION_PERTURB renders on this context (None unbinds).
        device_tables (an OR of ORBIT_TABLE_BLA / ORBIT_TABLE_BLA_DEEP, or 0): mc_context_bind_mandelbrot_orbit_tables, which builds the
        named BLA tables on this context's device instead of taking them from the orbit; last_table_timing() then reports the build."""
        if orbit is not None and not orbit._h:   # a closed orbit's handle is NULL, which the C call reads as "unbind"
            raise ValueError("Context.bind_mandelbrot_orbit: the orbit is closed")
        h = orbit._h if orbit is not None else None
        if device_tables is None:
            _check(lib().mc_context_bind_mandelbrot_orbit(self._h, h), "mc_context_bind_mandelbrot_orbit")
        else:
            _check(lib().mc_context_bind_mandelbrot_orbit_tables(self._h, h, int(device_tables)),
                   "mc_context_bind_mandelbrot_orbit_tables")

    def last_table_timing(self):
        """(device_ms, launches) of the last bind_mandelbrot_orbit(..., device_tables=nonzero) (mc_context_last_table_timing)."""
        ms, n = C.c_double(0), C.c_uint32(0)
        _check(lib().mc_context_last_table_timing(self._h, C.byref(ms), C.byref(n)), "mc_context_last_table_timing")
        return ms.value, n.value

    def bound_bla_table(self):
        """mc_context_bound_bla_copy: (table (entries, 5) float64 in Orbit.bla_table()'s layout, levels) of the bound BLA table."""
        lv, n = C.c_uint32(0), C.c_uint64(0)
        _check(lib().mc_context_bound_bla_copy(self._h, None, C.byref(lv), C.byref(n)), "mc_context_bound_bla_copy")
        out = np.empty((n.value, 5), np.float64)
        _check(lib().mc_context_bound_bla_copy(self._h, _ptr(out), None, None), "mc_context_bound_bla_copy")
        return out, lv.value

    def bound_bla_deep_table(self):
        """mc_context_bound_bla_deep_copy: (mantissas (entries, 5) float64, exponents (entries, 3) int32, levels) of the bound floatexp
        table, in Orbit.bla_deep_table()'s layout."""
        lv, n = C.c_uint32(0), C.c_uint64(0)
        _check(lib().mc_context_bound_bla_deep_copy(self._h, None, None, C.byref(lv), C.byref(n)), "mc_context_bound_bla_deep_copy")
        mant, exps = np.empty((n.value, 5), np.float64), np.empty((n.value, 3), np.int32)
        _check(lib().mc_context_bound_bla_deep_copy(self._h, _ptr(mant), _ptr(exps), None, None), "mc_context_bound_bla_deep_copy")
        return mant, exps, lv.value

    # ---- host-buffer forms -------------------------------------------------------------------------
    def mandelbrot(self, p, want_rgba=True, want_iters=True, out=None):
        rows = tile_rows(p)
        if out is not None:
            if not want_rgba:
                raise ValueError("Context.mandelbrot: out= is the colour buffer; it needs want_rgba=True")
            _check_out(out, (rows, p.width, 4), "Context.mandelbrot")
        rgba = (out if out is not None else np.empty((rows, p.width, 4), np.float32)) if want_rgba else None
        iters = np.empty((rows, p.width), np.uint32) if want_iters else None
        _check(lib().mc_mandelbrot_render(self._h, C.byref(p), _ptr(rgba), _ptr(iters)), "mc_mandelbrot_render")
        return rgba, iters

    def mandelbrot_atom(self, p, want_iters=True, want_period=True, want_amin=True):
        """mc_mandelbrot_render_atom: (n uint32, period uint32, amin float64) planes of p's whole image, None where not wanted."""
        shape = (p.height, p.width)
        iters = np.empty(shape, np.uint32) if want_iters else None
        period = np.empty(shape, np.uint32) if want_period else None
        amin = np.empty(shape, np.float64) if want_amin else None
        _check(lib().mc_mandelbrot_render_atom(self._h, C.byref(p), _ptr(iters), _ptr(period), _ptr(amin)), "mc_mandelbrot_render_atom")
        return iters, period, amin

    def mandelbrot_atom_device(self, p, d_iters=0, d_period=0, d_amin=0, stream=0):
        """mc_mandelbrot_render_atom_device_async into device planes (0: not wanted)."""
        _check(lib().mc_mandelbrot_render_atom_device_async(self._h, C.byref(p), d_iters or None, d_period or None, d_amin or None,
                                                            stream or None), "mc_mandelbrot_render_atom_device_async")

    def mandelbrot_atom_domains_device(self, d_period, d_amin, n_pixels, max_iter, d_count, d_amin_table, d_pixel, stream=0):
        """mc_mandelbrot_atom_domains_device_async: device planes into device tables of max_iter + 1 entries (count uint32, amin float64,
        pixel uint32), which the call initialises itself."""
        _check(lib().mc_mandelbrot_atom_domains_device_async(self._h, d_period or None, d_amin or None, int(n_pixels), int(max_iter),
                                                             d_count or None, d_amin_table or None, d_pixel or None, stream or None),
               "mc_mandelbrot_atom_domains_device_async")

    def mandelbrot_smooth(self, p, want_rgba=True, want_iters=True, want_smooth=True):
        """mc_mandelbrot_render_smooth (p carries MANDEL_COLOUR_SMOOTH): (rgba float32, n uint32, q uint32) of p's tile, None where not
        wanted.  q is the smooth count in 24.8 fixed point."""
        rows = tile_rows(p)
        rgba = np.empty((rows, p.width, 4), np.float32) if want_rgba else None
        iters = np.empty((rows, p.width), np.uint32) if want_iters else None
        smooth = np.empty((rows, p.width), np.uint32) if want_smooth else None
        _check(lib().mc_mandelbrot_render_smooth(self._h, C.byref(p), _ptr(rgba), _ptr(iters), _ptr(smooth)), "mc_mandelbrot_render_smooth")
        return rgba, iters, smooth

    def mandelbrot_distance(self, p, want_rgba=True, want_iters=True, want_smooth=True, want_distance=True):
        """mc_mandelbrot_render_distance (p carries MANDEL_COLOUR_DISTANCE, a whole image): (rgba float32, n uint32, q uint32, D float32),
        None where not wanted.  D is the distance estimate in pixel pitches; the colours are shaded with a threshold of one pixel."""
        shape = (p.height, p.width)
        rgba = np.empty(shape + (4,), np.float32) if want_rgba else None
        iters = np.empty(shape, np.uint32) if want_iters else None
        smooth = np.empty(shape, np.uint32) if want_smooth else None
        dist = np.empty(shape, np.float32) if want_distance else None
        _check(lib().mc_mandelbrot_render_distance(self._h, C.byref(p), _ptr(rgba), _ptr(iters), _ptr(smooth), _ptr(dist)),
               "mc_mandelbrot_render_distance")
        return rgba, iters, smooth, dist

    def mandelbrot_smooth_equalised(self, p, want_rgba=True, want_iters=True, want_smooth=True, want_ranked=True):
        """mc_mandelbrot_render_smooth_equalised (p carries MANDEL_COLOUR_SMOOTH_EQUALISED, a whole image): (rgba float32, n uint32,
        q uint32, q' uint32), None where not wanted.  q' is the smooth count ranked among the image's escaped pixels."""
        shape = (p.height, p.width)
        rgba = np.empty(shape + (4,), np.float32) if want_rgba else None
        iters = np.empty(shape, np.uint32) if want_iters else None
        smooth = np.empty(shape, np.uint32) if want_smooth else None
        ranked = np.empty(shape, np.uint32) if want_ranked else None
        _check(lib().mc_mandelbrot_render_smooth_equalised(self._h, C.byref(p), _ptr(rgba), _ptr(iters), _ptr(smooth), _ptr(ranked)),
               "mc_mandelbrot_render_smooth_equalised")
        return rgba, iters, smooth, ranked

    def mandelbrot_banded(self, p, band_rows, rgba8=False):
        """mc_mandelbrot_render_banded: the image (rows [row_begin, row_end)) rendered in pipelined row bands; returns the image — the fp32
        storage buffer, or RGBA8 converted on the device — and the rows_done values the callback heard, in the order it heard them."""
        rows = p.row_end - p.row_begin
        out = np.empty((rows, p.width, 4), np.uint8 if rgba8 else np.float32)
        heard = []
        cb_t = C.CFUNCTYPE(None, C.c_uint32, C.c_void_p)
        cb = cb_t(lambda done, user: heard.append(int(done)))
        fn = lib().mc_mandelbrot_render_banded
        fn.argtypes = [C.c_void_p, C.POINTER(MandelbrotParams), C.c_void_p, C.c_void_p, C.c_uint32, cb_t, C.c_void_p]
        _check(fn(self._h, C.byref(p), None if rgba8 else _ptr(out), _ptr(out) if rgba8 else None, band_rows, cb, None),
               "mc_mandelbrot_render_banded")
        return out, heard

    def pathtrace(self, p, planes=None, spheres=None, acc=None, out=None):
        if planes is None or spheres is None:
            planes, spheres = default_scene()
        planes = np.ascontiguousarray(planes, np.float32).reshape(-1)
        spheres = np.ascontiguousarray(spheres, np.float32).reshape(-1)
        rows = tile_rows(p)
        if out is not None:   # (out: the caller's own buffer, e.g. HostBuffer.array — written in place)
            _check_out(out, (rows, p.width, 4), "Context.pathtrace")
            if acc is not None:   # a progressive continuation starts from the accumulator: it goes into the caller's buffer first
                out[...] = np.asarray(acc, np.float32).reshape(out.shape)
        else:
            out = np.zeros((rows, p.width, 4), np.float32) if acc is None else np.ascontiguousarray(acc, np.float32).copy()
        _check(lib().mc_pathtrace_render(self._h, C.byref(p), _ptr(planes), planes.size // 12, _ptr(spheres),
                                         spheres.size // 12, _ptr(out)), "mc_pathtrace_render")
        return out

    def convert_rgba8(self, rgba_f32, scale, rotate180=False):
        a = np.ascontiguousarray(rgba_f32, np.float32)
        H, W = a.shape[0], a.shape[1]
        out = np.empty((H, W, 4), np.uint8)
        _check(lib().mc_convert_rgba8(self._h, _ptr(a), W, H, scale, int(rotate180), _ptr(out)), "mc_convert_rgba8")
        return out

    def buddhabrot(self, p):
        """mc_buddhabrot_render: (plane uint32 (height, width), BuddhabrotStats) of p's sample range."""
        plane = np.empty((p.height, p.width), np.uint32)
        stats = BuddhabrotStats()
        _check(lib().mc_buddhabrot_render(self._h, C.byref(p), _ptr(plane), C.byref(stats)), "mc_buddhabrot_render")
        return plane, stats

    def buddhabrot_guided(self, p, guide):
        """mc_buddhabrot_render_guided: (plane uint32 (height, width), BuddhabrotStats of the guided render, BuddhabrotGuideInfo) of the
        chain pilot -> map -> cell list -> guided render [-> complement pass]."""
        plane = np.empty((p.height, p.width), np.uint32)
        stats, info = BuddhabrotStats(), BuddhabrotGuideInfo()
        _check(lib().mc_buddhabrot_render_guided(self._h, C.byref(p), C.byref(guide), _ptr(plane), C.byref(stats), C.byref(info)),
               "mc_buddhabrot_render_guided")
        return plane, stats, info

    # ---- device-buffer forms (pointers are ints, e.g. torch.Tensor.data_ptr()) ------------------------
    def buddhabrot_importance_device(self, p, grid_log2, d_map, d_plane=0, d_stats=0, stream=0):
        """mc_buddhabrot_importance_device_async: ADDS to the device map uint32[G * G], to d_plane (0: no plane add is issued) and to
        d_stats (uint64[5]; 0: none)."""
        _check(lib().mc_buddhabrot_importance_device_async(self._h, C.byref(p), grid_log2, d_map or None, d_plane or None, d_stats or None,
                                                           stream or None), "mc_buddhabrot_importance_device_async")

    def buddhabrot_guided_device(self, p, d_cells, n_cells, grid_log2, weight, d_plane, d_stats=0, stream=0):
        """mc_buddhabrot_density_guided_device_async: d_cells is a DEVICE list of n_cells uint32 cell indices below G * G."""
        _check(lib().mc_buddhabrot_density_guided_device_async(self._h, C.byref(p), d_cells or None, n_cells, grid_log2, weight,
                                                               d_plane or None, d_stats or None, stream or None),
               "mc_buddhabrot_density_guided_device_async")

    def buddhabrot_device(self, p, d_plane, d_stats=0, stream=0):
        """mc_buddhabrot_density_device_async: ADDS p's samples to the device plane uint32[height][width] and to d_stats (uint64[5]; 0: none)."""
        _check(lib().mc_buddhabrot_density_device_async(self._h, C.byref(p), d_plane or None, d_stats or None, stream or None),
               "mc_buddhabrot_density_device_async")

    def buddhabrot_tonemap_device(self, width, height, d0, d1, d2, levels, m0, m1, m2, d_rgba, stream=0):
        """mc_buddhabrot_tonemap_device_async: three device planes (which may be one pointer), three host maps of levels + 1 entries."""
        maps = _tone_maps(levels, (m0, m1, m2), "Context.buddhabrot_tonemap_device")
        _check(lib().mc_buddhabrot_tonemap_device_async(self._h, width, height, d0 or None, d1 or None, d2 or None, levels, _ptr(maps[0]),
                                                        _ptr(maps[1]), _ptr(maps[2]), d_rgba or None, stream or None),
               "mc_buddhabrot_tonemap_device_async")

    def mandelbrot_device(self, p, d_rgba=0, d_iters=0, stream=0):
        _check(lib().mc_mandelbrot_render_device_async(self._h, C.byref(p), d_rgba or None, d_iters or None, stream or None),
               "mc_mandelbrot_render_device_async")

    def mandelbrot_smooth_device(self, p, d_rgba=0, d_iters=0, d_smooth=0, stream=0):
        """mc_mandelbrot_render_smooth_device_async: the device form of mandelbrot_smooth (d_smooth: a uint32 plane)."""
        _check(lib().mc_mandelbrot_render_smooth_device_async(self._h, C.byref(p), d_rgba or None, d_iters or None, d_smooth or None,
                                                              stream or None), "mc_mandelbrot_render_smooth_device_async")

    def mandelbrot_adaptive_smooth(self, p, threshold=MANDEL_ADAPTIVE_SMOOTH_THRESHOLD, rgba8=False):
        """mc_mandelbrot_render_adaptive_smooth (p carries MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE, a whole image): the adaptive smooth image
        with the caller's threshold, float32 (height, width, 4) or, with rgba8=True, uint8 (height, width, 4).  Context.last_refined()
        reports the refined share."""
        out = np.empty((p.height, p.width, 4), np.uint8 if rgba8 else np.float32)
        _check(lib().mc_mandelbrot_render_adaptive_smooth(self._h, C.byref(p), threshold, None if rgba8 else _ptr(out),
                                                          _ptr(out) if rgba8 else None), "mc_mandelbrot_render_adaptive_smooth")
        return out

    def mandelbrot_rgba8(self, p):
        """mc_mandelbrot_render_rgba8: the rows [row_begin, row_end) rendered and converted on the device; only RGBA8 leaves the GPU."""
        out = np.empty((p.row_end - p.row_begin, p.width, 4), np.uint8)
        _check(lib().mc_mandelbrot_render_rgba8(self._h, C.byref(p), _ptr(out)), "mc_mandelbrot_render_rgba8")
        return out

    def mandelbrot_distance_device(self, p, d_smooth, threshold_px=1.0, d_distance=0, d_rgba=0, stream=0):
        """mc_mandelbrot_distance_device_async: D (float32) and / or the shaded colours of p's rows [row_begin, row_end), stored compactly,
        from d_smooth, the WHOLE image's uint32 smooth plane."""
        _check(lib().mc_mandelbrot_distance_device_async(self._h, C.byref(p), d_smooth or None, threshold_px, d_distance or None,
                                                         d_rgba or None, stream or None), "mc_mandelbrot_distance_device_async")

    def mandelbrot_smooth_histogram_device(self, d_smooth, n_pixels, max_iter, d_hist, stream=0):
        """mc_mandelbrot_smooth_histogram_device_async: ADDS the counts of min(q >> 8, max_iter) over n_pixels uint32 smooth counts to the
        device table uint32[max_iter + 1]."""
        _check(lib().mc_mandelbrot_smooth_histogram_device_async(self._h, d_smooth or None, n_pixels, max_iter, d_hist or None,
                                                                 stream or None), "mc_mandelbrot_smooth_histogram_device_async")

    def mandelbrot_smooth_remap_device(self, p, d_smooth, qmap, d_ranked=0, d_rgba=0, stream=0):
        """mc_mandelbrot_smooth_remap_device_async: q' (uint32) and / or its colour for the tile p describes; qmap is a host array of
        max_iter + 1 knots."""
        m = np.ascontiguousarray(qmap, np.uint32).reshape(-1)
        if m.size != p.max_iter + 1:
            raise ValueError(f"Context.mandelbrot_smooth_remap_device: the map has {m.size} knots, max_iter + 1 = {p.max_iter + 1} expected")
        _check(lib().mc_mandelbrot_smooth_remap_device_async(self._h, C.byref(p), d_smooth or None, _ptr(m), d_ranked or None,
                                                             d_rgba or None, stream or None), "mc_mandelbrot_smooth_remap_device_async")

    def mandelbrot_histogram_device(self, d_iters, iters_bytes, n_pixels, max_iter, d_hist, stream=0):
        """mc_mandelbrot_histogram_device_async: ADDS the counts of n_pixels values (2 or 4 B each) to the device table
        uint32[max_iter + 1]."""
        _check(lib().mc_mandelbrot_histogram_device_async(self._h, d_iters or None, iters_bytes, n_pixels, max_iter, d_hist or None,
                                                          stream or None), "mc_mandelbrot_histogram_device_async")

    def mandelbrot_recolour_device(self, p, d_iters, iters_bytes, map_, d_rgba, stream=0):
        """mc_mandelbrot_recolour_device_async: lut[map[n]] for the tile p describes; map_ is a host array of max_iter + 1 entries."""
        m = np.ascontiguousarray(map_, np.uint32).reshape(-1)
        if m.size != p.max_iter + 1:
            raise ValueError(f"Context.mandelbrot_recolour_device: the map has {m.size} entries, max_iter + 1 = {p.max_iter + 1} expected")
        _check(lib().mc_mandelbrot_recolour_device_async(self._h, C.byref(p), d_iters or None, iters_bytes, _ptr(m), d_rgba or None,
                                                         stream or None), "mc_mandelbrot_recolour_device_async")

    def mandelbrot_resolve_device(self, p, d_samples, iters_bytes, map_, d_rgba, stream=0):
        """mc_mandelbrot_resolve_device_async: the colours of p's tile (p carries MANDEL_SUPERSAMPLE(s)) from the sample plane that
        mandelbrot_device(supersample_params(p)) wrote; map_ is a host array of max_iter + 1 entries, or None for the plain colouring."""
        m = None
        if map_ is not None:
            m = np.ascontiguousarray(map_, np.uint32).reshape(-1)
            if m.size != p.max_iter + 1:
                raise ValueError(f"Context.mandelbrot_resolve_device: the map has {m.size} entries, max_iter + 1 = {p.max_iter + 1} expected")
        _check(lib().mc_mandelbrot_resolve_device_async(self._h, C.byref(p), d_samples or None, iters_bytes, _ptr(m), d_rgba or None,
                                                        stream or None), "mc_mandelbrot_resolve_device_async")

    def mandelbrot_resolve_smooth_device(self, p, d_smooth, qmap, d_rgba, stream=0):
        """mc_mandelbrot_resolve_smooth_device_async: the colours of p's tile (p carries MANDEL_SUPERSAMPLE_SMOOTH, MANDEL_SUPERSAMPLE(s) and
        one smooth colouring) from the smooth sample plane that mandelbrot_smooth_device(supersample_params(p)) wrote; qmap is a host array
        of max_iter + 1 knots for MANDEL_COLOUR_SMOOTH_EQUALISED, None otherwise."""
        m = None
        if qmap is not None:
            m = np.ascontiguousarray(qmap, np.uint32).reshape(-1)
            if m.size != p.max_iter + 1:
                raise ValueError(f"Context.mandelbrot_resolve_smooth_device: the map has {m.size} knots, max_iter + 1 = {p.max_iter + 1} expected")
        _check(lib().mc_mandelbrot_resolve_smooth_device_async(self._h, C.byref(p), d_smooth or None, _ptr(m), d_rgba or None, stream or None),
               "mc_mandelbrot_resolve_smooth_device_async")

    def zoom_compose_device(self, width, height, d_wide, d_deep, r, d_rgba=0, d_rgba8=0, stream=0):
        """mc_mandelbrot_zoom_compose_device_async: the frame at r from the device keyframes d_wide and d_deep (0: absent) into the vec4
        buffer d_rgba and / or the RGBA8 buffer d_rgba8."""
        _check(lib().mc_mandelbrot_zoom_compose_device_async(self._h, width, height, d_wide or None, d_deep or None, float(r), d_rgba or None,
                                                             d_rgba8 or None, stream or None), "mc_mandelbrot_zoom_compose_device_async")

    def zoom_compose_filtered_device(self, width, height, d_wide, d_deep, r, filter, d_rgba=0, d_rgba8=0, stream=0):
        """mc_mandelbrot_zoom_compose_filtered_device_async: zoom_compose_device with a filter (ZOOM_FILTER_BILINEAR, ZOOM_FILTER_AREA)."""
        _check(lib().mc_mandelbrot_zoom_compose_filtered_device_async(self._h, width, height, d_wide or None, d_deep or None, float(r),
                                                                      int(filter), d_rgba or None, d_rgba8 or None, stream or None),
               "mc_mandelbrot_zoom_compose_filtered_device_async")

    def zoom(self, width, height):
        """mc_mandelbrot_zoom_create: a zoom sequence of width x height frames on this context (a context manager)."""
        return Zoom(self, width, height)

    def zoom_compose_counts_device(self, p, d_wide, d_deep, map, r, d_rgba=0, d_rgba8=0, stream=0):
        """mc_mandelbrot_zoom_compose_counts_device_async: the frame at r from the device count keyframes d_wide and d_deep (0: absent),
        coloured by p's colouring through the HOST table map (None: plain, smooth), into the vec4 plane d_rgba and / or the RGBA8 plane
        d_rgba8."""
        m = None
        if map is not None:
            m = np.ascontiguousarray(map, np.uint32).reshape(-1)
            if m.size != p.max_iter + 1:
                raise ValueError(f"zoom_compose_counts_device: the map has {m.size} entries, max_iter + 1 = {p.max_iter + 1} expected")
        _check(lib().mc_mandelbrot_zoom_compose_counts_device_async(self._h, C.byref(p), d_wide or None, d_deep or None, _ptr(m), float(r),
                                                                    d_rgba or None, d_rgba8 or None, stream or None),
               "mc_mandelbrot_zoom_compose_counts_device_async")

    def zoom_compose_counts_filtered_device(self, p, d_wide, d_deep, map, r, filter, d_rgba=0, d_rgba8=0, stream=0):
        """mc_mandelbrot_zoom_compose_counts_filtered_device_async: zoom_compose_counts_device with a filter (ZOOM_FILTER_BILINEAR,
        ZOOM_FILTER_AREA)."""
        m = None
        if map is not None:
            m = np.ascontiguousarray(map, np.uint32).reshape(-1)
            if m.size != p.max_iter + 1:
                raise ValueError(f"zoom_compose_counts_filtered_device: the map has {m.size} entries, max_iter + 1 = {p.max_iter + 1} expected")
        _check(lib().mc_mandelbrot_zoom_compose_counts_filtered_device_async(self._h, C.byref(p), d_wide or None, d_deep or None, _ptr(m),
                                                                             float(r), int(filter), d_rgba or None, d_rgba8 or None,
                                                                             stream or None),
               "mc_mandelbrot_zoom_compose_counts_filtered_device_async")

    def zoom_counts(self, width, height):
        """mc_mandelbrot_zoom_counts_create: a zoom sequence from count keyframes on this context (a context manager)."""
        return ZoomCounts(self, width, height)

    def pathtrace_guides_device(self, width, height, d_normal_t, d_position_id, planes=None, spheres=None, stream=0):
        """mc_pathtrace_guides_device_async: the guide planes of a width x height image into two device vec4 planes."""
        planes, spheres = _scene_tables(planes, spheres)
        _check(lib().mc_pathtrace_guides_device_async(self._h, width, height, _ptr(planes), planes.size // 12, _ptr(spheres), spheres.size // 12,
                                                      d_normal_t or None, d_position_id or None, stream or None),
               "mc_pathtrace_guides_device_async")

    def pathtrace_denoise_device(self, d, d_rgba, d_normal_t, d_position_id, d_out, stream=0):
        """mc_pathtrace_denoise_device_async: the filter of d from the device plane d_rgba into d_out (which may be d_rgba)."""
        _check(lib().mc_pathtrace_denoise_device_async(self._h, C.byref(d), d_rgba or None, d_normal_t or None, d_position_id or None,
                                                       d_out or None, stream or None), "mc_pathtrace_denoise_device_async")

    def pathtrace_denoised(self, p, d=None, planes=None, spheres=None, rgba8=False):
        """mc_pathtrace_render_denoised: render, guides and filter in one blocking call.  Returns the float32 (height, width, 4) storage
        buffer, or with rgba8 the uint8 image converted and rotated as mc_pathtrace_render_rgba8 does.  d: default parameters when None."""
        planes, spheres = _scene_tables(planes, spheres)
        if d is None:
            d = pathtrace_denoise_params(p.width, p.height)
        out = np.empty((p.height, p.width, 4), np.uint8 if rgba8 else np.float32)
        _check(lib().mc_pathtrace_render_denoised(self._h, C.byref(p), C.byref(d), _ptr(planes), planes.size // 12, _ptr(spheres),
                                                  spheres.size // 12, None if rgba8 else _ptr(out), _ptr(out) if rgba8 else None),
               "mc_pathtrace_render_denoised")
        return out

    def pathtrace_noise_device(self, width, height, d_half, scale, d_full, radius, d_variance, stream=0):
        """mc_pathtrace_noise_device_async: the noise plane (one float per pixel) of the device vec4 planes d_half and d_full."""
        _check(lib().mc_pathtrace_noise_device_async(self._h, width, height, d_half or None, scale, d_full or None, radius, d_variance or None,
                                                     stream or None), "mc_pathtrace_noise_device_async")

    def pathtrace_denoise_adaptive_device(self, d, k_noise, d_rgba, d_normal_t, d_position_id, d_variance, d_out, stream=0):
        """mc_pathtrace_denoise_adaptive_device_async: the noise-guided filter from d_rgba into d_out (which may be d_rgba)."""
        _check(lib().mc_pathtrace_denoise_adaptive_device_async(self._h, C.byref(d), k_noise, d_rgba or None, d_normal_t or None,
                                                                d_position_id or None, d_variance or None, d_out or None, stream or None),
               "mc_pathtrace_denoise_adaptive_device_async")

    def pathtrace_denoised_adaptive(self, p, d=None, k_noise=None, radius=None, planes=None, spheres=None, rgba8=False):
        """mc_pathtrace_render_denoised_adaptive: the render in two sample ranges, the guides, the noise plane and the noise-guided filter in
        one blocking call; the outputs of pathtrace_denoised.  d, k_noise, radius: the defaults when None."""
        planes, spheres = _scene_tables(planes, spheres)
        if d is None:
            d = pathtrace_denoise_params(p.width, p.height)
        k0, r0 = pathtrace_noise_defaults()
        out = np.empty((p.height, p.width, 4), np.uint8 if rgba8 else np.float32)
        _check(lib().mc_pathtrace_render_denoised_adaptive(self._h, C.byref(p), C.byref(d), k0 if k_noise is None else k_noise,
                                                           r0 if radius is None else radius, _ptr(planes), planes.size // 12, _ptr(spheres),
                                                           spheres.size // 12, None if rgba8 else _ptr(out), _ptr(out) if rgba8 else None),
               "mc_pathtrace_render_denoised_adaptive")
        return out

    def pathtrace_budget_levels_device(self, width, height, d_variance, target, max_level, d_levels, stream=0):
        """mc_pathtrace_budget_levels_device_async: the level plane (one byte per pixel) of the device noise plane d_variance."""
        _check(lib().mc_pathtrace_budget_levels_device_async(self._h, width, height, d_variance or None, target, max_level, d_levels or None,
                                                             stream or None), "mc_pathtrace_budget_levels_device_async")

    def pathtrace_budget_lists_device(self, width, height, d_levels, max_level, d_list, d_counts, stream=0):
        """mc_pathtrace_budget_lists_device_async: the storage indices bucketed by level, highest first, into d_list (width * height uint32)
        and the pixels of every level into d_counts (nine uint32)."""
        _check(lib().mc_pathtrace_budget_lists_device_async(self._h, width, height, d_levels or None, max_level, d_list or None, d_counts or None,
                                                            stream or None), "mc_pathtrace_budget_lists_device_async")

    def pathtrace_budget_resolve_device(self, width, height, d_acc, d_levels, d_out, stream=0):
        """mc_pathtrace_budget_resolve_device_async: the encoded buffer of the accumulator plane d_acc into d_out (which may be d_acc)."""
        _check(lib().mc_pathtrace_budget_resolve_device_async(self._h, width, height, d_acc or None, d_levels or None, d_out or None,
                                                              stream or None), "mc_pathtrace_budget_resolve_device_async")

    def pathtrace_list_device(self, p, d_list, n_list, prescale, d_acc, planes=None, spheres=None, stream=0):
        """mc_pathtrace_render_list_device_async: samples [sample_begin, sample_end) of p added to the listed pixels of the linear accumulator
        plane d_acc, each first scaled by prescale; no final encode."""
        planes, spheres = _scene_tables(planes, spheres)
        _check(lib().mc_pathtrace_render_list_device_async(self._h, C.byref(p), _ptr(planes), planes.size // 12, _ptr(spheres), spheres.size // 12,
                                                           d_list or None, n_list, prescale, d_acc or None, stream or None),
               "mc_pathtrace_render_list_device_async")

    def pathtrace_budgeted(self, p, b=None, planes=None, spheres=None, rgba8=False, want_levels=False):
        """mc_pathtrace_render_budgeted: the pilot of p.spp samples, the noise plane, levels, lists, the doubling rounds and the resolve in one
        blocking call; the outputs of pathtrace_denoised, with want_levels the pair (image, uint8 (height, width) levels).  b: the defaults
        when None."""
        planes, spheres = _scene_tables(planes, spheres)
        if b is None:
            b = pathtrace_budget_params()
        out = np.empty((p.height, p.width, 4), np.uint8 if rgba8 else np.float32)
        levels = np.empty((p.height, p.width), np.uint8) if want_levels else None
        _check(lib().mc_pathtrace_render_budgeted(self._h, C.byref(p), C.byref(b), _ptr(planes), planes.size // 12, _ptr(spheres),
                                                  spheres.size // 12, None if rgba8 else _ptr(out), _ptr(out) if rgba8 else None, _ptr(levels)),
               "mc_pathtrace_render_budgeted")
        return (out, levels) if want_levels else out

    def last_budget(self):
        """mc_context_last_budget: (pixels per level 0 .. 8, mean samples per pixel) of the last pathtrace_budgeted."""
        per = (C.c_uint64 * 9)()
        mean = C.c_double(0.0)
        _check(lib().mc_context_last_budget(self._h, per, C.byref(mean)), "mc_context_last_budget")
        return [int(x) for x in per], mean.value

    def pathtrace_accel(self, accel, p, acc=None):
        """mc_pathtrace_render_accel: Context.pathtrace through a PathtraceAccel (acc: the accumulator a sample range continues)."""
        rows = tile_rows(p)
        out = np.zeros((rows, p.width, 4), np.float32) if acc is None else np.ascontiguousarray(acc, np.float32).copy()
        _check(lib().mc_pathtrace_render_accel(self._h, accel._h, C.byref(p), _ptr(out)), "mc_pathtrace_render_accel")
        return out

    def pathtrace_accel_rgba8(self, accel, p):
        out = np.empty((p.height, p.width, 4), np.uint8)
        _check(lib().mc_pathtrace_render_accel_rgba8(self._h, accel._h, C.byref(p), _ptr(out)), "mc_pathtrace_render_accel_rgba8")
        return out

    def pathtrace_accel_device(self, accel, p, d_rgba, stream=0):
        _check(lib().mc_pathtrace_render_accel_device_async(self._h, accel._h, C.byref(p), d_rgba or None, stream or None),
               "mc_pathtrace_render_accel_device_async")

    def pathtrace_accel_guides_device(self, accel, width, height, d_normal_t, d_position_id, stream=0):
        """mc_pathtrace_accel_guides_device_async: pathtrace_guides_device through a PathtraceAccel's cached device copy."""
        _check(lib().mc_pathtrace_accel_guides_device_async(self._h, accel._h, width, height, d_normal_t or None, d_position_id or None,
                                                            stream or None), "mc_pathtrace_accel_guides_device_async")

    def pathtrace_accel_denoised(self, accel, p, d=None, rgba8=False):
        """mc_pathtrace_render_accel_denoised: pathtrace_denoised through a PathtraceAccel."""
        if d is None:
            d = pathtrace_denoise_params(p.width, p.height)
        out = np.empty((p.height, p.width, 4), np.uint8 if rgba8 else np.float32)
        _check(lib().mc_pathtrace_render_accel_denoised(self._h, accel._h, C.byref(p), C.byref(d), None if rgba8 else _ptr(out),
                                                        _ptr(out) if rgba8 else None), "mc_pathtrace_render_accel_denoised")
        return out

    def pathtrace_accel_denoised_adaptive(self, accel, p, d=None, k_noise=None, radius=None, rgba8=False):
        """mc_pathtrace_render_accel_denoised_adaptive: pathtrace_denoised_adaptive through a PathtraceAccel."""
        if d is None:
            d = pathtrace_denoise_params(p.width, p.height)
        k0, r0 = pathtrace_noise_defaults()
        out = np.empty((p.height, p.width, 4), np.uint8 if rgba8 else np.float32)
        _check(lib().mc_pathtrace_render_accel_denoised_adaptive(self._h, accel._h, C.byref(p), C.byref(d), k0 if k_noise is None else k_noise,
                                                                 r0 if radius is None else radius, None if rgba8 else _ptr(out),
                                                                 _ptr(out) if rgba8 else None),
               "mc_pathtrace_render_accel_denoised_adaptive")
        return out

    def pathtrace_accel_list_device(self, accel, p, d_list, n_list, prescale, d_acc, stream=0):
        """mc_pathtrace_render_accel_list_device_async: pathtrace_list_device through a PathtraceAccel."""
        _check(lib().mc_pathtrace_render_accel_list_device_async(self._h, accel._h, C.byref(p), d_list or None, n_list, prescale, d_acc or None,
                                                                 stream or None), "mc_pathtrace_render_accel_list_device_async")

    def pathtrace_accel_budgeted(self, accel, p, b=None, rgba8=False, want_levels=False):
        """mc_pathtrace_render_accel_budgeted: pathtrace_budgeted through a PathtraceAccel; last_budget reports it."""
        if b is None:
            b = pathtrace_budget_params()
        out = np.empty((p.height, p.width, 4), np.uint8 if rgba8 else np.float32)
        levels = np.empty((p.height, p.width), np.uint8) if want_levels else None
        _check(lib().mc_pathtrace_render_accel_budgeted(self._h, accel._h, C.byref(p), C.byref(b), None if rgba8 else _ptr(out),
                                                        _ptr(out) if rgba8 else None, _ptr(levels)), "mc_pathtrace_render_accel_budgeted")
        return (out, levels) if want_levels else out

    def pathtrace_device(self, p, d_rgba, planes=None, spheres=None, stream=0):
        if planes is None or spheres is None:
            planes, spheres = default_scene()
        planes = np.ascontiguousarray(planes, np.float32).reshape(-1)
        spheres = np.ascontiguousarray(spheres, np.float32).reshape(-1)
        _check(lib().mc_pathtrace_render_device_async(self._h, C.byref(p), _ptr(planes), planes.size // 12, _ptr(spheres),
                                                      spheres.size // 12, d_rgba, stream or None),
               "mc_pathtrace_render_device_async")

    def convert_rgba8_device(self, d_rgba_f32, W, H, scale, rotate180, d_rgba8, stream=0):
        _check(lib().mc_convert_rgba8_device_async(self._h, d_rgba_f32, W, H, scale, int(rotate180), d_rgba8, stream or None),
               "mc_convert_rgba8_device_async")

    def mandelbrot_assemble_device(self, p, d_tiles, iters_bytes, n_tiles, row_block, tile_rows_padded, d_rgba=0, d_iters=0, stream=0):
        """Root side of the Mandelbrot exchange: gathered interleaved tiles of iteration counts (2 or 4 B/pixel) -> the whole
        image's vec4 storage buffer (lut[n]) and / or its uint32 count plane."""
        _check(lib().mc_mandelbrot_assemble_device_async(self._h, C.byref(p), d_tiles, iters_bytes, n_tiles, row_block,
                                                         tile_rows_padded, d_rgba or None, d_iters or None, stream or None),
               "mc_mandelbrot_assemble_device_async")

    def assemble_rgba8_device(self, d_tiles_u8, W, H, n_tiles, row_block, tile_rows_padded, rotate180, d_rgba8, stream=0):
        """Root side of the path tracer's RGBA8 exchange: gathered interleaved byte tiles -> the whole RGBA8 image, point-reflected
        as saveRenderedImage leaves it when rotate180 is set."""
        _check(lib().mc_assemble_rgba8_device_async(self._h, d_tiles_u8, W, H, n_tiles, row_block, tile_rows_padded, int(rotate180),
                                                    d_rgba8, stream or None), "mc_assemble_rgba8_device_async")

    def deinterleave_rows_device(self, d_tiles, W, H, n_tiles, row_block, tile_rows_padded, bpp, d_out, stream=0):
        _check(lib().mc_deinterleave_rows_device_async(self._h, d_tiles, W, H, n_tiles, row_block, tile_rows_padded, bpp,
                                                       d_out, stream or None), "mc_deinterleave_rows_device_async")

    # ---- device self-tests ---------------------------------------------------------------------------
    def test_math(self, fn, x, fast=False):
        """mc_test_math: fast = False / 0 the strict functions, True / 1 the fast tier's, 2 the careful tier's short forms without
        their window tests (rsqrt, sqrt and rcp only)."""
        code = {"sin": 0, "cos": 1, "log2": 2, "exp2": 3, "pow045": 4, "rsqrt": 5, "sqrt": 6, "rcp": 7, "sincos_s": 8,
                "sincos_c": 9}[fn]
        if int(fast) == 2 and code not in (5, 6, 7):
            raise ValueError(f"Context.test_math: the careful tier (fast=2) has rsqrt, sqrt and rcp only, not {fn}")
        x = np.ascontiguousarray(x, np.float32).reshape(-1)
        out = np.empty_like(x)
        _check(test_lib().mc_test_math(self._h, code, int(fast), _ptr(x), _ptr(out), x.size), "mc_test_math")
        return out

    def test_div3(self, a, s, with_y=False):
        a = np.ascontiguousarray(a, np.float32).reshape(-1, 3)
        s = np.ascontiguousarray(s, np.float32).reshape(-1)
        out = np.empty_like(a)
        _check(test_lib().mc_test_div3(self._h, int(with_y), _ptr(a), _ptr(s), _ptr(out), s.size), "mc_test_div3")
        return out

    def test_math_sweep(self, fn, first_bits, count):
        """(mismatches vs the IEEE expansion, checksum, first mismatching pattern) over `count` consecutive bit patterns."""
        code = {"rsqrt": 5, "sqrt": 6, "rcp": 7}[fn]
        bad, chk, first = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        _check(test_lib().mc_test_math_sweep(self._h, code, first_bits, count, C.byref(bad), C.byref(chk), C.byref(first)),
               "mc_test_math_sweep")
        return bad.value, chk.value, first.value

    def test_rand01(self, xyz):
        k = np.ascontiguousarray(xyz, np.uint32).reshape(-1, 3)
        out = np.empty(k.shape, np.float32)
        _check(test_lib().mc_test_rand01(self._h, _ptr(k), _ptr(out), k.shape[0]), "mc_test_rand01")
        return out

    def test_ds_op(self, op, a, b):
        a = np.ascontiguousarray(a, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(b, np.float32).reshape(-1, 2)
        out = np.empty(a.shape, np.float32)
        _check(test_lib().mc_test_ds_op(self._h, DS_OPS[op], _ptr(a), _ptr(b), _ptr(out),
                                   a.shape[0]), "mc_test_ds_op")
        return out

    def test_mandel_refine(self, d_plane, iters_bytes, width, height, d_list, d_count, stream=0):
        """mc_hook_mandel_refine: the refine list of the W x H count plane at device pointer d_plane into d_list (device, W * H uint32), its
        length into d_count (device, one uint32).  Asynchronous on `stream`; the list's order is unspecified."""
        _check(test_lib().mc_hook_mandel_refine(self._h, d_plane, iters_bytes, width, height, d_list, d_count, stream), "mc_hook_mandel_refine")


    def test_mandel_block_audit(self, p, sabotage=False):
        """mc_hook_mandel_block_audit: the (tile rows, W, 4) uint32 array (n, accepted_blocks, raised_blocks, first_bad) of p's pixels,
        each audited alone (F32, DS, F64; include/mc_compute_test.h).  sabotage: needs_exact taken as false."""
        out = np.empty((tile_rows(p), p.width, 4), np.uint32)
        _check(test_lib().mc_hook_mandel_block_audit(self._h, C.byref(p), int(bool(sabotage)), _ptr(out)), "mc_hook_mandel_block_audit")
        return out

    def test_mandel_perturb_block_audit(self, Z, ux, uy, max_iter, deep=False, exp2=0, sabotage=False):
        """mc_hook_mandel_perturb_block_audit: the (lanes, 4) uint32 array (n, accepted_blocks, raised_blocks, first_bad) of the lanes with
        offsets (ux[k], uy[k]) against the orbit table Z ((L + 1, 2) float64; any values).  deep: the rescaled loop with E = exp2."""
        Z = np.ascontiguousarray(Z, np.float64).reshape(-1, 2)
        ux = np.ascontiguousarray(ux, np.float64).ravel()
        uy = np.ascontiguousarray(uy, np.float64).ravel()
        if ux.size != uy.size:
            raise ValueError("Context.test_mandel_perturb_block_audit: ux and uy differ in length")
        out = np.empty((ux.size, 4), np.uint32)
        _check(test_lib().mc_hook_mandel_perturb_block_audit(self._h, _ptr(Z), Z.shape[0] - 1, int(bool(deep)), int(exp2), _ptr(ux), _ptr(uy),
                                                             ux.size, int(max_iter), int(bool(sabotage)), _ptr(out)),
               "mc_hook_mandel_perturb_block_audit")
        return out


class Zoom:
    """mc_mandelbrot_zoom: two keyframe slots on a context's device.  push(p) renders a keyframe (each at exactly half the previous one's
    scale); frame(r) composes the frame whose scale is r times the wider held keyframe's (r from zoom_ratio).  Closing the context closes the zooms
    made on it first."""

    def __init__(self, ctx, width, height):
        self._h = C.c_void_p()
        self._ctx = ctx   # (kept alive: the slots are freed on its device)
        self.width, self.height = int(width), int(height)
        _check(lib().mc_mandelbrot_zoom_create(ctx._h, self.width, self.height, C.byref(self._h)), "mc_mandelbrot_zoom_create")
        ctx._zooms = [r for r in ctx._zooms if r() is not None] + [weakref.ref(self)]

    def push(self, p):
        _check(lib().mc_mandelbrot_zoom_push(self._h, C.byref(p)), "mc_mandelbrot_zoom_push")

    def frame(self, r, want_rgba=True, want_rgba8=False):
        """(rgba float32 (H, W, 4), rgba8 uint8 (H, W, 4)), None where not wanted."""
        rgba = np.empty((self.height, self.width, 4), np.float32) if want_rgba else None
        rgba8 = np.empty((self.height, self.width, 4), np.uint8) if want_rgba8 else None
        _check(lib().mc_mandelbrot_zoom_frame(self._h, float(r), _ptr(rgba), _ptr(rgba8)), "mc_mandelbrot_zoom_frame")
        return rgba, rgba8

    def frame_filtered(self, r, filter, want_rgba=True, want_rgba8=False):
        """mc_mandelbrot_zoom_frame_filtered: frame(r) with a filter (ZOOM_FILTER_BILINEAR: frame's own bits; ZOOM_FILTER_AREA)."""
        rgba = np.empty((self.height, self.width, 4), np.float32) if want_rgba else None
        rgba8 = np.empty((self.height, self.width, 4), np.uint8) if want_rgba8 else None
        _check(lib().mc_mandelbrot_zoom_frame_filtered(self._h, float(r), int(filter), _ptr(rgba), _ptr(rgba8)),
               "mc_mandelbrot_zoom_frame_filtered")
        return rgba, rgba8

    def close(self):
        if self._h:   # (the context is still open: Context.close closes its zooms before itself)
            lib().mc_mandelbrot_zoom_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ZoomCounts:
    """mc_mandelbrot_zoom_counts: two count-keyframe slots on a context's device, each with its rank or knot map.  push(p) renders a
    keyframe's count plane (each at exactly half the previous one's scale; the first fixes colouring, max_iter and k_color);
    frame(step, steps_per_octave) composes a frame through ONE map, blended from the two keyframes' maps on the device.  Closing the
    context closes the sequences made on it first."""

    def __init__(self, ctx, width, height):
        self._h = C.c_void_p()
        self._ctx = ctx   # (kept alive: the slots are freed on its device)
        self.width, self.height = int(width), int(height)
        self._entries = 0
        _check(lib().mc_mandelbrot_zoom_counts_create(ctx._h, self.width, self.height, C.byref(self._h)), "mc_mandelbrot_zoom_counts_create")
        ctx._zooms = [r for r in ctx._zooms if r() is not None] + [weakref.ref(self)]

    def push(self, p):
        _check(lib().mc_mandelbrot_zoom_counts_push(self._h, C.byref(p)), "mc_mandelbrot_zoom_counts_push")
        self._entries = int(p.max_iter) + 1

    def frame(self, step, steps_per_octave, want_rgba=True, want_rgba8=False):
        """(rgba float32 (H, W, 4), rgba8 uint8 (H, W, 4)), None where not wanted."""
        rgba = np.empty((self.height, self.width, 4), np.float32) if want_rgba else None
        rgba8 = np.empty((self.height, self.width, 4), np.uint8) if want_rgba8 else None
        _check(lib().mc_mandelbrot_zoom_counts_frame(self._h, int(step), int(steps_per_octave), _ptr(rgba), _ptr(rgba8)),
               "mc_mandelbrot_zoom_counts_frame")
        return rgba, rgba8

    def frame_filtered(self, step, steps_per_octave, filter, want_rgba=True, want_rgba8=False):
        """mc_mandelbrot_zoom_counts_frame_filtered: frame(step, steps_per_octave) with a filter (ZOOM_FILTER_BILINEAR, ZOOM_FILTER_AREA)."""
        rgba = np.empty((self.height, self.width, 4), np.float32) if want_rgba else None
        rgba8 = np.empty((self.height, self.width, 4), np.uint8) if want_rgba8 else None
        _check(lib().mc_mandelbrot_zoom_counts_frame_filtered(self._h, int(step), int(steps_per_octave), int(filter), _ptr(rgba), _ptr(rgba8)),
               "mc_mandelbrot_zoom_counts_frame_filtered")
        return rgba, rgba8

    def maps(self):
        """(wide map, deep map), uint32 (max_iter + 1) each: the rank or knot maps of the keyframes held (one held: twice that one's)."""
        wide = np.empty(max(self._entries, 1), np.uint32)
        deep = np.empty(max(self._entries, 1), np.uint32)
        _check(lib().mc_mandelbrot_zoom_counts_maps(self._h, _ptr(wide), _ptr(deep)), "mc_mandelbrot_zoom_counts_maps")
        return wide, deep

    def close(self):
        if self._h:   # (the context is still open: Context.close closes its sequences before itself)
            lib().mc_mandelbrot_zoom_counts_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Multi:
    """mc_multi wrapper: single-process multi-GPU render with an RCCL gather to device 0."""

    def __init__(self, n_devices):
        self._h = C.c_void_p()
        _check(lib().mc_multi_create(n_devices, C.byref(self._h)), "mc_multi_create")
        self.n = n_devices

    def close(self):
        if self._h:
            lib().mc_multi_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def mandelbrot(self, p, want_rgba=True, want_iters=True):
        rgba = np.empty((p.height, p.width, 4), np.float32) if want_rgba else None
        iters = np.empty((p.height, p.width), np.uint32) if want_iters else None
        _check(lib().mc_multi_mandelbrot_render(self._h, C.byref(p), _ptr(rgba), _ptr(iters)), "mc_multi_mandelbrot_render")
        return rgba, iters

    def pathtrace(self, p, planes=None, spheres=None):
        if planes is None or spheres is None:
            planes, spheres = default_scene()
        planes = np.ascontiguousarray(planes, np.float32).reshape(-1)
        spheres = np.ascontiguousarray(spheres, np.float32).reshape(-1)
        out = np.empty((p.height, p.width, 4), np.float32)
        _check(lib().mc_multi_pathtrace_render(self._h, C.byref(p), _ptr(planes), planes.size // 12, _ptr(spheres),
                                               spheres.size // 12, _ptr(out)), "mc_multi_pathtrace_render")
        return out

    def pathtrace_rgba8(self, p, planes=None, spheres=None):
        """mc_multi_pathtrace_render_rgba8: the finished image as saveRenderedImage converts and rotates it, 4 B/pixel exchanged."""
        if planes is None or spheres is None:
            planes, spheres = default_scene()
        planes = np.ascontiguousarray(planes, np.float32).reshape(-1)
        spheres = np.ascontiguousarray(spheres, np.float32).reshape(-1)
        out = np.empty((p.height, p.width, 4), np.uint8)
        _check(lib().mc_multi_pathtrace_render_rgba8(self._h, C.byref(p), _ptr(planes), planes.size // 12, _ptr(spheres),
                                                     spheres.size // 12, _ptr(out)), "mc_multi_pathtrace_render_rgba8")
        return out

    def mandelbrot_rgba8(self, p):
        out = np.empty((p.height, p.width, 4), np.uint8)
        _check(lib().mc_multi_mandelbrot_render_rgba8(self._h, C.byref(p), _ptr(out)), "mc_multi_mandelbrot_render_rgba8")
        return out
