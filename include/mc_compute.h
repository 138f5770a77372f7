/*
 * mc_compute.h — C ABI of libmc_compute.so: the MI355X (gfx950) replacement for the Vulkan compute
 * runtime + GLSL shaders of pjhusky/vulkan-compute-tests.
 *
 * The reference has no FFI; the boundary this library sits behind is the C++ virtual surface of
 * `VulkanComputeApp` (src/vulkanComputeApp.h:30-67) as driven by src/main.cpp:28-33.  Each entry
 * point below cites the reference code it replaces (paths relative to the reference checkout).
 * The C++ mirror of the reference interface lives in vulkan-compute-tests_amd/host/ and calls only
 * these functions; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions: plain pointers and sizes, no exceptions, no STL, no torch types.  Every function
 * returns MC_OK (0) or an mc_status error code; mc_error_string() renders it; mc_last_error_detail()
 * gives the HIP/RCCL message of the last failure on the calling thread.  All calls are blocking
 * unless the name ends in _async.  A context is not thread-safe; use one per thread/device.
 *
 * Buffer layout (the reference's storage-buffer contract): row-major, one `vec4` fp32 per pixel
 * (16 B, src/mandelbrotApp.h:187-189, shaders/mandelbrot.comp:10-17,59, shaders/pathTracer.comp:71),
 * rows are STORAGE rows (for the path tracer storage row r holds pix.y = H-1-r, pathTracer.comp:349).
 * Tile calls take [row_begin,row_end) in storage rows and a pointer to the FIRST ROW OF THE TILE.
 */
#ifndef MC_COMPUTE_H_
#define MC_COMPUTE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3, un-bumped additions since: MC_PRECISION_PERTURB with mc_mandelbrot_orbit_* and mc_context_bind_mandelbrot_orbit; then
 * mc_mandelbrot_orbit_create_deep (scales down to 2^-8192); then MC_PRECISION_PERTURB_BLA with mc_mandelbrot_orbit_bla and
 * mc_mandelbrot_orbit_bla_copy; then MC_PRECISION_PERTURB_BLA_DEEP with mc_mandelbrot_orbit_bla_deep and mc_mandelbrot_orbit_bla_deep_copy;
 * then MC_MANDEL_COLOUR_EQUALISED with mc_mandelbrot_histogram_device_async, mc_mandelbrot_equalise_map and
 * mc_mandelbrot_recolour_device_async; then MC_MANDEL_SUPERSAMPLE with mc_mandelbrot_supersample_params and
 * mc_mandelbrot_resolve_device_async; then MC_MANDEL_SUPERSAMPLE_ADAPTIVE with mc_context_last_refined; then
 * mc_mandelbrot_orbit_create_device with mc_context_last_orbit_timing; then MC_MANDEL_COLOUR_SMOOTH_EQUALISED with
 * mc_mandelbrot_render_smooth_equalised, mc_mandelbrot_smooth_histogram_device_async, mc_mandelbrot_smooth_equalise_map,
 * mc_mandelbrot_smooth_remap and mc_mandelbrot_smooth_remap_device_async (the newest); before it MC_MANDEL_COLOUR_SMOOTH with mc_mandelbrot_render_smooth,
 * mc_mandelbrot_render_smooth_device_async, mc_mandelbrot_smooth_count and mc_mandelbrot_smooth_colour; then MC_MANDEL_COLOUR_DISTANCE with
 * mc_mandelbrot_render_distance, mc_mandelbrot_distance_device_async, mc_mandelbrot_distance_plane and mc_mandelbrot_distance_colour; then
 * zoom sequences: mc_mandelbrot_zoom_ratio, mc_mandelbrot_zoom_compose, mc_mandelbrot_zoom_compose_device_async and mc_mandelbrot_zoom_create,
 * _push, _frame and _destroy; then the path tracer's denoiser, noise plane and BVH calls (their sections say so); then per-pixel sample
 * budgets: mc_pathtrace_budget_params with mc_pathtrace_budget_default_params, _levels, _resolve, their _device_async forms and
 * mc_pathtrace_budget_lists_device_async, mc_pathtrace_render_list_device_async, mc_pathtrace_render_budgeted, mc_context_last_budget;
 * then zoom sequences from count keyframes: mc_mandelbrot_zoom_blend_map, mc_mandelbrot_zoom_compose_counts,
 * mc_mandelbrot_zoom_compose_counts_device_async and mc_mandelbrot_zoom_counts_create, _push, _frame, _maps and _destroy; then the area
 * filter of the minified deep keyframe: MC_MANDEL_ZOOM_FILTER_BILINEAR / _AREA with mc_mandelbrot_zoom_compose_filtered,
 * mc_mandelbrot_zoom_compose_filtered_device_async, mc_mandelbrot_zoom_compose_counts_filtered,
 * mc_mandelbrot_zoom_compose_counts_filtered_device_async, mc_mandelbrot_zoom_frame_filtered and mc_mandelbrot_zoom_counts_frame_filtered;
 * then MC_MANDEL_SUPERSAMPLE_SMOOTH with mc_mandelbrot_resolve_smooth_device_async and mc_mandelbrot_resolve_smooth; then the Buddhabrot:
 * mc_buddhabrot_params and mc_buddhabrot_stats with mc_buddhabrot_default_params, _density, _density_device_async, _render, _sqrt_map,
 * _tonemap and _tonemap_device_async; then its importance map and guided sampling: mc_buddhabrot_guide_params and _guide_info with
 * mc_buddhabrot_importance, _importance_device_async, _importance_cells, _density_guided, _density_guided_device_async,
 * _guide_default_params and _render_guided; then dives: mc_mandelbrot_orbit_rescale, and BLA tables built on the device with
 * mc_context_bind_mandelbrot_orbit_tables, mc_context_last_table_timing, mc_context_bound_bla_copy and mc_context_bound_bla_deep_copy;
 * then exact counts of sampled pixels: mc_mandelbrot_exact_pixel_offsets, mc_mandelbrot_exact_counts, mc_mandelbrot_exact_counts_device
 * and mc_context_last_exact_timing; then atom domains: mc_mandelbrot_render_atom, mc_mandelbrot_render_atom_device_async,
 * mc_mandelbrot_atom_scan, mc_mandelbrot_atom_domains, mc_mandelbrot_atom_domains_device_async, mc_mandelbrot_nucleus_refine and
 * mc_mandelbrot_orbit_offset_text.
 * 3 (end of round 6): + mc_mandelbrot_render_banded, row bands in mc_mandelbrot_render_rgba8, scene-class bit 32 (MC_PT_SCENE_SPECULAR),
 * bit 1 of mc_context_warmup_mandelbrot's last argument.
 * 2 (round 6): + mc_assemble_rgba8_device_async, mc_context_warmup_*; since 1 (round 5 additions, un-bumped then): mc_build_id,
 * mc_host_alloc / mc_host_free, mc_context_last_timing, math_mode 2, scene-class bit 16; the measurement flag enums moved to
 * mc_compute_test.h.  A binder checks mc_abi_version() against the MC_ABI_VERSION it was written for. */
#define MC_ABI_VERSION 3

typedef enum mc_status {
    MC_OK = 0,
    MC_ERR_INVALID_ARGUMENT = 1, /* NULL pointer, zero size, row range outside the image ...          */
    MC_ERR_NO_DEVICE = 2,        /* no HIP device / device index out of range (vulkanComputeApp.cpp:78) */
    MC_ERR_HIP = 3,              /* a HIP runtime call failed; see mc_last_error_detail()             */
    MC_ERR_RCCL = 4,             /* an RCCL call failed                                               */
    MC_ERR_UNSUPPORTED = 5,      /* e.g. scene larger than the on-chip scene store                    */
    MC_ERR_OUT_OF_MEMORY = 6     /* a device allocation failed; mc_host_alloc: more than this process may still take */
} mc_status;

typedef struct mc_context mc_context; /* opaque: device, stream, scratch, LUT cache, (optional) RCCL comms */

/* ---- lifecycle: replaces VulkanComputeApp::init() (vulkanComputeApp.cpp:443-449: createInstance,
 *      findPhysicalDevice, createDevice) and cleanupVulkanResources() (:673-695) -------------------- */
int mc_abi_version(void);
/* Which build is this: "pt=<id> mandel=<id> lib=<id>", each id 16 hex digits of the SHA-256 of the sources that kernel family (path
 * tracer, Mandelbrot, whole library) was compiled from, and of the compiler flags.  Measurement records kept beside the code
 * (profiles/ *_pmc_summary.json) carry the id of the library they were taken on; bench.py quotes them only for a matching build. */
const char* mc_build_id(void);
int mc_device_count(int* count);
int mc_context_create(int device, mc_context** out_ctx);
int mc_context_destroy(mc_context* ctx);
const char* mc_error_string(int status);
const char* mc_last_error_detail(void);
/* Device name / CU count of the context's device (vulkanComputeApp.cpp:163 picks devices[0]). */
int mc_context_device_info(mc_context* ctx, char* name, size_t name_len, int* compute_units, int* clock_khz);

/* Page-locked host memory for the storage buffer the application owns — what stands where the reference allocates its output buffer
 * HOST_VISIBLE | HOST_COHERENT (VulkanComputeApp::createBuffer, vulkanComputeApp.cpp:489-533; mapped by getRenderedImage,
 * mandelbrotApp.h:153 / pathtracerApp.h:206; freed at vulkanComputeApp.cpp:684-685).  The buffer lives in HBM while the kernels
 * write it, so 16 B/pixel cross PCIe once, at the end of mc_*_render; into page-locked memory that copy needs no staging and no
 * page pinning by the runtime.  Buffers of 32 MB and more are huge-page mappings first-touched in parallel and then registered with
 * the runtime (K4's 629 MB: 4 ms instead of hipHostMalloc's 86, same copy rate; profiles/r06_hostmem_probe.txt), smaller ones
 * hipHostMalloc.  Any host pointer is accepted by the render calls — a pageable one is copied at nearly the same rate once its pages
 * are resident, at half of it while they are not — so these two are an ownership convention, not a requirement.
 * Usable before any context exists; the memory is visible to every device of the node.  Every page handed out is touched or pinned:
 * a request beyond what the process may still take (MemAvailable, the room under a cgroup memory limit) returns MC_ERR_OUT_OF_MEMORY
 * before a page is touched (mc_last_error_detail names both figures) — it would otherwise meet the out-of-memory killer. */
int mc_host_alloc(size_t bytes, void** out_ptr);
int mc_host_free(void* ptr);

/* Device time of the LAST blocking host-buffer call on this context (mc_mandelbrot_render, mc_pathtrace_render, mc_*_render_rgba8):
 * kernel_ms = first launch to last kernel end (render, and the on-device conversion of the _rgba8 forms), copy_ms = the device -> host
 * copy that follows.  Measured with HIP events on the context's stream and recorded by the call itself once its stream is idle: this one
 * only reads the record, and a call that fails after its launch clears it.  Either pointer may be NULL.  MC_ERR_INVALID_ARGUMENT before
 * the first such call.  (The reference times nothing, vulkanComputeApp.cpp:451-466 only prints progress; the apps print these next to run().) */
int mc_context_last_timing(mc_context* ctx, double* kernel_ms, double* copy_ms);

/* Shader clock (MHz) the device holds with every SIMD busy on fp32 VALU work, measured in-kernel (s_memtime against the
 * constant 100 MHz s_memrealtime over ~2 ms).  MI355X boxes differ by >10 % here (DVFS), and VALU-issue-bound kernels with
 * them; bench.py prints it next to every timing so that runs on different boxes can be compared (no reference counterpart). */
int mc_context_measure_clock(mc_context* ctx, double* sclk_mhz);

/* ---- Mandelbrot: replaces shaders/mandelbrot.comp:21-60 + the dispatch recorded in
 *      MandelbrotApp::createCommandBuffer (src/mandelbrotApp.h:137-147) ----------------------------- */
enum { MC_PRECISION_F32 = 0, MC_PRECISION_DS = 1 /* two-float, emulateDouble.h.glsl:59-139 */,
       MC_PRECISION_F64 = 2 /* native IEEE double (emulateDouble.h.glsl:13, USE_NATIVE_FP64) */ };
/* MC_PRECISION_F64, exactly (what tests/mandel_f64_ref.py restates):
 *  - view: the same words as MC_PRECISION_DS, read as doubles: centre_x = (double)centre_x_hi + (double)centre_x_lo, and the same for
 *    centre_y, scale_x and scale_y.  With hi = (float)d, lo = (float)(d - hi) that sum is exact, so a view means the same thing in DS
 *    and F64 and no new packing exists.  The centre carries about 48 significant bits: that only shifts the view by less than
 *    2^-48 |centre|; the pixel grid itself (the scale, the per-pixel offsets below) is computed in full double.
 *  - per-pixel c, IEEE double, no contraction: x = (double)gx / (double)W, c.x = centre_x + (x - 0.5) * scale_x; the same for y with
 *    gy, H, centre_y, scale_y.
 *  - loop (mandelbrot.comp:40-46 in double, source order), z = 0, sx = sy = 0, n = 0; for i in [0, M):
 *      nzx = (sx - sy) + c.x;  nzy = ((2 * zx) * zy) + c.y;  zx = nzx;  zy = nzy;  sx = zx * zx;  sy = zy * zy;
 *      if (sx + sy > 2.0) break;  n++
 *    n is the number of iterations that did not escape, in [0, M].
 *  - colour: the fp32 table of mc_mandelbrot_colour_lut (t = n / M in fp32), so the RGBA f32, RGBA8 and PNG outputs are the same
 *    functions of n as for the other two precisions. */
/* MC_PRECISION_PERTURB (3): deep zooms past fp64 by perturbation (what tests/mandel_perturb_ref.py restates).  A
 * reference orbit Z_0 .. Z_L is computed once on the host in multi-limb fixed point (mc_mandelbrot_orbit_create) and bound to the
 * context; every pixel iterates its offset from that orbit in IEEE double.
 *  - view: the bound orbit's centre c_ref and scale (sx, sy).  The params' eight view words must all be zero (a stale F32/DS/F64 view is
 *    an error, not silently ignored), an orbit must be bound and p->max_iter <= the orbit's max_iter: MC_ERR_INVALID_ARGUMENT otherwise.
 *  - per pixel, IEEE double, no contraction, source order (gx column, gy storage row, as F64's c table):
 *      dcx = ((double)gx / (double)W - 0.5) * sx;  dcy = ((double)gy / (double)H - 0.5) * sy;   (the pixel's c is c_ref + (dcx, dcy))
 *      dx = dy = 0, m = 0; for i in [0, M):
 *        ax = (Z[m].x + Z[m].x) + dx;  ay = (Z[m].y + Z[m].y) + dy;
 *        ndx = ((ax * dx) - (ay * dy)) + dcx;  ndy = ((ax * dy) + (ay * dx)) + dcy;
 *        m = m + 1;  zx = Z[m].x + ndx;  zy = Z[m].y + ndy;  r = (zx * zx) + (zy * zy);
 *        if (r > 2.0) break;                                                       (n = i: the iterations that did not escape)
 *        if (m == L || r < ((ndx * ndx) + (ndy * ndy))) { dx = zx; dy = zy; m = 0; }   (rebase onto the orbit's start)
 *        else { dx = ndx; dy = ndy; }
 *    n = M when the loop runs out.  fp64 denormals are kept.  The colour is lut[n] of mc_mandelbrot_colour_lut, as for the others.
 *  - interior pixels run all M iterations: the state includes m, so the Brent cycle exit of the other precisions does not apply.
 *  - accuracy: n is exactly the loop above, not always the count of c iterated exactly.  In particular a reference orbit that escapes with
 *    |Z_L|^2 within double rounding of 2 has that last comparison decided in double for every pixel that follows it, so such a view can be
 *    wrong as a whole; choose a centre whose orbit clears 2 (or stays bounded).  High counts near the boundary also diverge from exact
 *    iteration pixel by pixel, as any finite precision does (DESIGN.md §3.6 gives measured agreement).
 *  - every single-device entry point that takes mc_mandelbrot_params renders it (row tiles, interleaved tiles, MC_MANDEL_ITERS_U16,
 *    _device_async, _rgba8, _banded, mc_context_warmup_mandelbrot).  mc_multi_* refuse it with MC_ERR_UNSUPPORTED: multi-GPU
 *    perturbation is out of scope (no two-GPU machine to test it on).
 *  - the loop above renders every orbit whose min(|scale_x|, |scale_y|) >= 2^-960.  An orbit of mc_mandelbrot_orbit_create_deep below
 *    that (what tests/mandel_perturb_deep_ref.py restates) renders by RESCALED perturbation instead, in the same
 *    IEEE double with no contraction.  pow2(k) = ldexp(1.0, k): 0 below 2^-1074, inf above 2^1023; ldexp is correctly rounded
 *    (subnormals kept); frexp_exp(a) = the e of a = f * 2^e, f in [0.5, 1) (0 for a = 0); fmax/fabs as in C.  T = 2^-500.
 *      ux = ((double)gx / (double)W - 0.5) * mx;  uy = ((double)gy / (double)H - 0.5) * my;   (the scale is (mx, my) * 2^E: dc = u 2^E)
 *      w = d = 0, S = E, scaled = 1, m = 0, zm = Z[0]; for i in [0, M):          (delta = w * 2^S exactly; d = ldexp(w, S))
 *        if (scaled && zm == (0, 0)) {                                            (a fresh exponent at Z_m = 0)
 *          S' = max(2S, E);  px = pow2(2S - S');  pu = pow2(E - S');
 *          nwx = (((wx * wx) - (wy * wy)) * px) + (ux * pu);  nwy = (((wx * wy) + (wy * wx)) * px) + (uy * pu);
 *        } else {                                                                 (plain phase: S = 0, StatePerturb op for op)
 *          S' = S;  pu = pow2(E - S);  ax = (zm.x + zm.x) + dx;  ay = (zm.y + zm.y) + dy;
 *          nwx = ((ax * wx) - (ay * wy)) + (ux * pu);  nwy = ((ax * wy) + (ay * wx)) + (uy * pu);
 *        }
 *        ndx = ldexp(nwx, S');  ndy = ldexp(nwy, S');  m = m + 1;  zx = Z[m].x + ndx;  zy = Z[m].y + ndy;  r = (zx * zx) + (zy * zy);
 *        if (r > 2.0) break;                                                       (n = i)
 *        if (m == L || r < ((ndx * ndx) + (ndy * ndy))) {                          (rebase: m = 0, zm = Z[0], d = z)
 *          a = fmax(fabs(zx), fabs(zy));
 *          if (a >= T) { scaled = 0; S = 0; w = z; }
 *          else { scaled = 1; S = (a == 0 ? E : frexp_exp(a)); w = (ldexp(zx, -S), ldexp(zy, -S)); }
 *        } else {
 *          zm = Z[m];  w = nw;  d = nd;  S = S';
 *          if (scaled && fmax(fabs(ndx), fabs(ndy)) >= T) { scaled = 0; S = 0; w = nd; }          (enter the plain phase)
 *          else if (scaled) { a = fmax(fabs(nwx), fabs(nwy));
 *            if (a > 2^256 || a < 2^-256) { e = frexp_exp(a); w = (ldexp(nwx, -e), ldexp(nwy, -e)); S = S' + e; } }   (renormalise)
 *        }
 *    In the plain phase this is the loop above with dc = u * pow2(E) (for an orbit of the old scale, E = 0: exactly it).  A term that
 *    underflows is dropped harmlessly: |2 Z_m| >= 2^-959 whenever Z_m is nonzero (the tiny-entry refusal below), and in the plain
 *    phase |delta| >= T or a rebase has reset it.  No cycle exit, as above. */
#define MC_PRECISION_PERTURB 3u

/* The reference orbit of MC_PRECISION_PERTURB.  Host only: touches no device, usable without a GPU.
 *  - centre_x / centre_y: decimal text, [+-]? (digits [. digits?] | . digits) ([eE] [+-]? digits)?, at most 4096 characters, |value| <= 4.
 *    Anything else (empty, hex, inf, nan, spaces, a trailing e, |value| > 4): MC_ERR_INVALID_ARGUMENT.
 *  - scale_x / scale_y: finite and nonzero (MC_ERR_INVALID_ARGUMENT); min(|scale_x|, |scale_y|) < 2^-960: MC_ERR_UNSUPPORTED (a
 *    pixel offset could leave the normal doubles).  max_iter >= 1.
 *  - arithmetic: binary fixed point with `bits` = max(64, ceil(-log2 min(|scale_x|, |scale_y|)) + 96) fractional bits — carried as whole
 *    64-bit limbs, so the words hold `bits` rounded up to a multiple of 64 — and a 64-bit integer limb (|Z| <= 8).  Each decimal is
 *    rounded ONCE into that format by round-to-odd (truncate; set the last bit when anything nonzero was dropped): that sticky bit makes
 *    the later rounding to double correct, so Z_1 = c_ref is the correctly rounded double of the decimal (strtod, Python's float(s))
 *    whenever the coordinate is 0 or at least 2^(55 - bits) in magnitude.  Products are rounded to nearest.
 *  - Z_0 = 0, Z_{j+1} = Z_j^2 + c_ref; L = the first j >= 1 with |Z_j|^2 > 2 in that precision, or max_iter if there is none.  The table
 *    holds Z_0 .. Z_L, each part rounded to the nearest double (ties to even).  Three multi-limb products per iteration: measured in
 *    DESIGN.md §3.6.
 * mc_mandelbrot_orbit_create_deep: the same orbit for the scale (scale_x * 2^scale_exp2, scale_y * 2^scale_exp2), exact for any
 * int32 exponent.  The mantissas must be finite and nonzero (MC_ERR_INVALID_ARGUMENT); min |scale| < 2^-8192 is MC_ERR_UNSUPPORTED
 * (the fixed point stops at 130 fractional limbs); bits is the formula above, from the frexp exponents plus scale_exp2, and the centre
 * rules are the same.  When both scales are doubles and min |scale| >= 2^-960 the orbit IS mc_mandelbrot_orbit_create's for
 * (scale_x * 2^scale_exp2, scale_y * 2^scale_exp2) and renders by the loop above (a scale above the double range there:
 * MC_ERR_UNSUPPORTED).  Below 2^-960 the orbit is DEEP and renders by the rescaled loop, with one more refusal, beside "a reference
 * on the hair": an entry Z_j (1 <= j <= L) that is nonzero with both parts below 2^-960 in magnitude is MC_ERR_UNSUPPORTED
 * (mc_last_error_detail names j).  The table stays double2, and such an entry cannot be rounded to a double without losing the offset
 * the view resolves: it happens when the centre sits on a nucleus far more closely than the view needs.  Exactly zero entries are
 * exact and accepted (centre 0; centre -1, orbit 0, -1, 0, ...).
 * mc_mandelbrot_orbit_copy writes (length + 1) * 2 doubles (re, im per entry).  mc_context_bind_mandelbrot_orbit copies the table to the
 * context's device after draining the context's launch streams (a running launch never sees it replaced); the orbit object may be
 * destroyed afterwards.  NULL unbinds. */
typedef struct mc_mandelbrot_orbit mc_mandelbrot_orbit;
int mc_mandelbrot_orbit_create(const char* centre_x, const char* centre_y, double scale_x, double scale_y,
                               uint32_t max_iter, mc_mandelbrot_orbit** out);
int mc_mandelbrot_orbit_create_deep(const char* centre_x, const char* centre_y, double scale_x, double scale_y, int32_t scale_exp2,
                                    uint32_t max_iter, mc_mandelbrot_orbit** out);
/* mc_mandelbrot_orbit_create_device: the SAME object as mc_mandelbrot_orbit_create_deep with the same arguments (the plain constructor's
 * orbit where that one forwards to it), its iteration loop run on ctx's device instead of the host (it pays from
 * the limb count measured there upward, and loses on shallow orbits).  Pure integer arithmetic: bits, length, max_iter, the scale fields
 * and every bit of the table Z_0 .. Z_L are the host constructor's, signed zeros and subnormals included, and everything that takes an orbit
 * takes this one, on any context.  The refusals are mc_mandelbrot_orbit_create_deep's, with the same status and the same text after
 * the function's name in mc_last_error_detail, and every refusal of the arguments comes before anything is launched; ctx == NULL is
 * MC_ERR_INVALID_ARGUMENT.  Blocking, on the context's stream; neither the context's bound orbit nor its render scratch is touched.  The
 * orbit is computed by one workgroup in several launches of at most C / (k + 1)^2 iterations each, clamped to [1, 65536] (k + 1 = the
 * limb count, C sized so that a launch stays near 50 ms at most); the state between launches lives in device memory, the host reads
 * its status word and j (8 bytes) and the launch's table entries (16 B each) after every launch and stops on escape or refusal.
 * mc_context_last_orbit_timing: the last successful device orbit of the context: device_ms = first launch to the end of the last kernel
 * (HIP events; the reads between launches included), the number of launches, and the limb count k + 1.  Any pointer may be NULL;
 * MC_ERR_INVALID_ARGUMENT before the first such call. */
int mc_mandelbrot_orbit_create_device(mc_context* ctx, const char* centre_x, const char* centre_y, double scale_x, double scale_y,
                                      int32_t scale_exp2, uint32_t max_iter, mc_mandelbrot_orbit** out);
int mc_context_last_orbit_timing(mc_context* ctx, double* device_ms, uint32_t* launches, uint32_t* limbs);
int mc_mandelbrot_orbit_destroy(mc_mandelbrot_orbit* o);
int mc_mandelbrot_orbit_info(const mc_mandelbrot_orbit* o, uint32_t* length, uint32_t* max_iter, uint32_t* bits);
int mc_mandelbrot_orbit_copy(const mc_mandelbrot_orbit* o, double* out_z /* (length+1)*2: re, im */);
int mc_context_bind_mandelbrot_orbit(mc_context* ctx, const mc_mandelbrot_orbit* o);   /* NULL unbinds */
/* mc_mandelbrot_orbit_rescale: a new orbit object that carries o's table Z_0 .. Z_L, length, max_iter and bits unchanged under another
 * scale of the same centre, (scale_x * 2^scale_exp2, scale_y * 2^scale_exp2): what a dive needs, whose keyframes share one centre, so
 * that the orbit is computed once, for the deepest keyframe.  Host only.  The scale fields of the new object (the doubles, or the
 * mantissas with their exponent, and whether it is deep) are the ones mc_mandelbrot_orbit_create_deep stores for that scale, the folding
 * into plain doubles when min |scale| >= 2^-960 included.  It carries no BLA table; o is untouched and may be destroyed afterwards.
 *  - refusals of the scale are mc_mandelbrot_orbit_create_deep's, with the same status and the same text after the function's name:
 *    mantissas finite and nonzero (MC_ERR_INVALID_ARGUMENT), min |scale| < 2^-8192 and a plain scale above the double range
 *    (MC_ERR_UNSUPPORTED).  NULL o or out: MC_ERR_INVALID_ARGUMENT.
 *  - one more, MC_ERR_UNSUPPORTED: the bits formula above applied to the new scale gives more than o's bits: o was computed for a
 *    shallower view and has too few bits for this one.  (So a deep object never comes from a plain one: the formula steps at 2^-960.)
 *  - accuracy: the table is the source's.  The fixed point is carried in whole 64-bit limbs, ceil(bits / 64) of them, so whenever both
 *    scales need the same number of limbs the table is bit for bit the one a fresh constructor makes for the new scale.  Across limb
 *    counts it is the table of the deeper, more precise orbit: each entry is the exact orbit's value rounded after a smaller
 *    accumulated error, and individual doubles may differ from the fresh constructor's in the last place (and L may differ where
 *    |Z_j|^2 sits within that error of 2).  Every kernel's contract is stated over the bound table, so renders stay exact
 *    restatements of it either way. */
int mc_mandelbrot_orbit_rescale(const mc_mandelbrot_orbit* o, double scale_x, double scale_y, int32_t scale_exp2,
                                mc_mandelbrot_orbit** out);

/* MC_PRECISION_PERTURB_BLA (4): MC_PRECISION_PERTURB with bilinear approximation (BLA): one step stands in for 2^k iterations while the
 * offset is small enough for the linear terms to dominate (what tests/mandel_bla_ref.py restates).
 *  - view and binding: PERTURB's rules (the eight view words zero, p->max_iter <= the orbit's max_iter, MC_MANDEL_ITERS_U16 needs
 *    p->max_iter <= 65535: MC_ERR_INVALID_ARGUMENT otherwise), and the bound orbit must carry its table (mc_mandelbrot_orbit_bla before
 *    mc_context_bind_mandelbrot_orbit): MC_ERR_INVALID_ARGUMENT otherwise.  Orbits with min |scale| >= 2^-960 only: a deep orbit
 *    (mc_mandelbrot_orbit_create_deep below 2^-960) is MC_ERR_UNSUPPORTED.  mc_multi_* refuse it with MC_ERR_UNSUPPORTED.
 *  - IEEE double, no contraction, source order, as PERTURB.  N1(v) = |v.x| + |v.y| (>= |v|, submultiplicative for complex products);
 *    cm = 0.5 * (|sx| + |sy|) with (sx, sy) the orbit's scale (it bounds N1(dc) of every pixel); eps = 2^-53.
 *  - the table, built on the host from Z_0 .. Z_L; an entry is (A, B, R), A and B complex, R >= 0 a radius:
 *      level 0: one entry per step j in [1, L-2] (Z_j -> Z_{j+1}):  A = (Z_j.x + Z_j.x, Z_j.y + Z_j.y);  B = (1, 0);
 *               R = eps * max(|A.x|, |A.y|)
 *      level k >= 1: an entry at each m = 1 + t * 2^k with m + 2^k <= L-1, composing x = (k-1, m) then y = (k-1, m + 2^(k-1)):
 *               A.x = (Ay.x * Ax.x) - (Ay.y * Ax.y);  A.y = (Ay.x * Ax.y) + (Ay.y * Ax.x);
 *               B.x = ((Ay.x * Bx.x) - (Ay.y * Bx.y)) + By.x;  B.y = ((Ay.x * Bx.y) + (Ay.y * Bx.x)) + By.y;
 *               q = (Ry - (N1(Bx) * cm)) / N1(Ax);
 *               R = min(Rx, q) if A.x, A.y, B.x, B.y and q are all finite, N1(Ax) > 0 and q > 0;  R = 0 otherwise
 *    so level k holds floor((L-2) / 2^k) entries (none when L < 3), the levels run while that is >= 1, and R_k(m) <= R_(k-1)(m).
 *  - per pixel: dc as PERTURB's;  dx = dy = 0, m = 0, i = 0;  while (i < M):
 *      K = the largest k >= 1 with: m >= 1, (m - 1) divisible by 2^k, m + 2^k <= L-1, i + 2^k <= M and (|dx| + |dy|) < R_k(m)
 *          (the levels that pass form a prefix 1 .. K, so K may be found by bisection);
 *      if there is one (a skip), with (A, B) = entry (K, m):
 *          dx' = ((A.x * dx) - (A.y * dy)) + ((B.x * dcx) - (B.y * dcy));  dy' = ((A.x * dy) + (A.y * dx)) + ((B.x * dcy) + (B.y * dcx));
 *          d = d';  m = m + 2^K;  i = i + 2^K          (no escape test and no rebase test inside the skip)
 *      else PERTURB's iteration i exactly (its a, new offset, m = m + 1, z, r; if (r > 2.0) n = i, stop; its rebase rule), then i = i + 1.
 *    n = M when the loop runs out; the colour is lut[n].  m <= L-1 at the top of every trip.
 *  - accuracy: a skip drops the d^2 terms of its 2^K iterations; R keeps |d| below about eps |2 Z_j| at every step it spans, so each
 *    dropped term is below about eps times the linear term beside it.  No escape and no rebase is tested inside a skip: a skip never
 *    reaches Z_L (m + 2^K <= L-1), but an intermediate z = Z_j + d with |Z_j|^2 within about |d| of 2, or |Z_j| within about |d| of 0,
 *    is not looked at.  n is this loop's, not PERTURB's; the two differ on pixels where such a test or double rounding decides
 *    (DESIGN.md §3.8 gives measured agreement).
 *  - interior pixels follow the orbit by skips until it ends, then run PERTURB's exact iterations: no cycle exit, as PERTURB.
 * mc_mandelbrot_orbit_bla builds the table once and keeps it in the orbit object (about 2L entries of 5 doubles; host only, no device);
 * *levels / *entries (either may be NULL) receive its shape.  A deep orbit: MC_ERR_UNSUPPORTED; an allocation failure:
 * MC_ERR_OUT_OF_MEMORY.  mc_mandelbrot_orbit_bla_copy writes it level-major, (A.x, A.y, B.x, B.y, R) per entry, level k's entry for m at
 * (sum over j < k of floor((L-2) / 2^j)) + (m - 1) / 2^k; MC_ERR_INVALID_ARGUMENT before mc_mandelbrot_orbit_bla.
 * mc_context_bind_mandelbrot_orbit uploads the table with the orbit when the orbit has one (PERTURB's bind is unchanged otherwise). */
#define MC_PRECISION_PERTURB_BLA 4u
int mc_mandelbrot_orbit_bla(mc_mandelbrot_orbit* o, uint32_t* levels, uint64_t* entries);
int mc_mandelbrot_orbit_bla_copy(const mc_mandelbrot_orbit* o, double* out /* entries * 5 */);

/* MC_PRECISION_PERTURB_BLA_DEEP (5): rescaled perturbation with bilinear skips, for every orbit PERTURB renders, shallow and deep
 * (what tests/mandel_bla_deep_ref.py restates).  Below 2^-960 A, B and R of the table above leave the double range
 * (|B| grows to about 2^-E, R shrinks below 2^-1074, cm is 2^E), so the table and the skip are carried in FLOATEXP.
 *  - floatexp: (x, y) * 2^e with x, y doubles and e an int32, NORMALISED: max(|x|, |y|) in [0.5, 1), or x = y = 0 with e = 0.  A real
 *    value has y = 0.  norm(x, y, e): a = max(|x|, |y|); a = 0 gives (0, 0, 0); else k = frexp_exp(a), (ldexp(x, -k), ldexp(y, -k), e + k).
 *    mul: the complex (or real) product of the mantissas in double, source order as below, at the exponent e1 + e2, then norm.
 *    add(p, q), mantissas in any range: a zero operand (both parts 0) gives norm of the other; else kp = ep + frexp_exp(max|p|),
 *    kq = eq + frexp_exp(max|q|), e = max(kp, kq), norm(ldexp(px, ep - e) + ldexp(qx, eq - e), ldexp(py, ep - e) + ldexp(qy, eq - e), e).
 *    less(a, b) for nonnegative reals: b = 0: no; a = 0: yes; else (ea, xa) < (eb, xb) lexicographically.  ldexp and frexp_exp as in
 *    PERTURB's rescaled loop above.  Each operation is double arithmetic on mantissas followed by exact power-of-two scaling, so wherever
 *    no mantissa operation (ldexp included) overflows or goes subnormal, a floatexp result IS the plain double result times a power of
 *    two: on such data this table and loop compute PRECISION_PERTURB_BLA's values bit for bit.
 *  - the table (mc_mandelbrot_orbit_bla_deep, host only): PERTURB_BLA's levels, entry positions and compositions, every value floatexp;
 *    cm = norm(0.5 * (|mx| + |my|), 0, E) (E = 0 and (mx, my) = the scale for an orbit of the old scale):
 *      level 0, step j:  A = norm(Z_j.x + Z_j.x, Z_j.y + Z_j.y, 0);  B = (0.5, 0, 1);  R = (max(|A.x|, |A.y|), 0, e_A - 53), 0 if A = 0
 *      level k, x = (k-1, m), y = (k-1, m + 2^(k-1)):
 *        A = norm((Ay.x * Ax.x) - (Ay.y * Ax.y), (Ay.x * Ax.y) + (Ay.y * Ax.x), eAy + eAx);
 *        B = add(((Ay.x * Bx.x) - (Ay.y * Bx.y), (Ay.x * Bx.y) + (Ay.y * Bx.x), eAy + eBx), By);
 *        na = |Ax.x| + |Ax.y|;  nb = |Bx.x| + |Bx.y|;  diff = add(Ry, (-(nb * cm.x), 0, eBx + e_cm));
 *        R = (na > 0 and diff.x > 0) ? min(Rx, norm(diff.x / na, 0, e_diff - eAx)) by less : 0
 *      and an entry with |e| > 2^20 in A, B or R is stored as A = B = R = 0 (every exponent then 0): exponents stay far from int32
 *      overflow on long orbits.  As in PERTURB_BLA, R_k(m) <= R_(k-1)(m) and no entry with R > 0 spans a step with Z_j = 0.
 *  - per pixel: u, E, and the state w, S, scaled, m of PERTURB's rescaled loop (the same start: w = d = 0, S = E, scaled = 1, m = 0);
 *    i = 0; while (i < M):
 *      K = PERTURB_BLA's largest level (m >= 1, alignment, m + 2^k <= L-1, i + 2^k <= M) whose radius test holds:
 *          ldexp(|wx| + |wy|, S - e_R) < R.x       (N1(w) 2^S < R, exact: R.x is 0 or in [0.5, 1))
 *      if there is one (a skip), with entry (A, B):
 *          P = ((A.x * wx) - (A.y * wy), (A.x * wy) + (A.y * wx), e_A + S);  Q = ((B.x * ux) - (B.y * uy), (B.x * uy) + (B.y * ux), e_B + E);
 *          (nx, ny, e) = add(P, Q);  m = m + 2^K;  i = i + 2^K;  no escape or rebase test, then
 *          n = 0:                                   w = d = 0, S = E, scaled = 1;
 *          max(|ldexp(nx, e)|, |ldexp(ny, e)|) >= T: d = w = (ldexp(nx, e), ldexp(ny, e)), S = 0, scaled = 0 (the plain phase);
 *          otherwise:                               w = (nx, ny), S = e, d = (ldexp(nx, e), ldexp(ny, e)), scaled = 1 (w is normalised:
 *                                                   inside the window, so the window rule changes nothing);
 *      else the rescaled iteration i above exactly (its fresh-exponent rule at Z_m = 0, escape: n = i, stop; rebase; phase change;
 *          window), then i = i + 1.
 *    n = M when the loop runs out; the colour is lut[n].  Since no skip spans a Z_j = 0 step, the fresh-exponent rule stays a rule of
 *    exact steps.  Accuracy as PERTURB_BLA's (DESIGN.md §3.9 gives measured agreement).
 *  - view and binding: PERTURB's rules (view words, max_iter, MC_MANDEL_ITERS_U16), and the bound orbit must carry this table
 *    (mc_mandelbrot_orbit_bla_deep before mc_context_bind_mandelbrot_orbit): MC_ERR_INVALID_ARGUMENT otherwise.  mc_multi_* refuse it
 *    with MC_ERR_UNSUPPORTED.  Every single-device entry point renders it.
 * mc_mandelbrot_orbit_bla_deep builds the table once and keeps it in the orbit beside any PERTURB_BLA table (one 64-byte record per
 * entry); *levels / *entries (either may be NULL) receive its shape.  NULL: MC_ERR_INVALID_ARGUMENT; an allocation failure:
 * MC_ERR_OUT_OF_MEMORY.  mc_mandelbrot_orbit_bla_deep_copy writes it in PERTURB_BLA's order: (A.x, A.y, B.x, B.y, R.x) per entry to
 * mant and (e_A, e_B, e_R) to exps; MC_ERR_INVALID_ARGUMENT before mc_mandelbrot_orbit_bla_deep.  mc_context_bind_mandelbrot_orbit
 * uploads it with the orbit when the orbit has one. */
#define MC_PRECISION_PERTURB_BLA_DEEP 5u
int mc_mandelbrot_orbit_bla_deep(mc_mandelbrot_orbit* o, uint32_t* levels, uint64_t* entries);
int mc_mandelbrot_orbit_bla_deep_copy(const mc_mandelbrot_orbit* o, double* mant /* entries * 5 */, int32_t* exps /* entries * 3 */);
/* BLA tables built on the device.
 * mc_context_bind_mandelbrot_orbit_tables is mc_context_bind_mandelbrot_orbit (drain the context's launch streams, upload Z, set the
 * binding, synchronise before returning) plus one thing: each table named in device_tables is computed on the context's device, from
 * the Z just uploaded and the orbit's scale, straight into the binding.  No host table is read, made, or stored in o.  A table not
 * named behaves as in the plain bind: uploaded if o holds it, released otherwise; device_tables = 0 IS the plain bind.
 * MC_ORBIT_TABLE_BLA on a deep orbit is MC_ERR_UNSUPPORTED (mc_mandelbrot_orbit_bla's text), unknown bits are
 * MC_ERR_INVALID_ARGUMENT, and every refusal comes before the current binding is touched.  L < 3 binds "a table with no entry", as
 * the host builders make it.
 *  - contract: the tables are the ones mc_mandelbrot_orbit_bla / mc_mandelbrot_orbit_bla_deep build from the same object, every field
 *    the same bits (one text of the arithmetic, compiled for both sides), with one exception: where the host's value is a NaN the
 *    device's is a NaN too, of any sign and payload (the two processors generate different default NaNs; PERTURB_BLA's table does
 *    produce inf - inf in A or B at high levels of a bounded orbit).  Such an entry has R = 0, the kernels never read A or B of an entry
 *    whose R is 0, so renders are bit-identical regardless.  R is never a NaN.
 *  - the build: one lane per entry; a workgroup carries 1024 adjacent entries of a level up through the ten levels above them with a
 *    block barrier between levels, so a launch builds eleven levels and every level of at most 1024 entries, with all above it, runs in
 *    a single workgroup.  No atomics.
 * mc_context_last_table_timing: the last such bind of the context that named a table: device_ms = first build launch to the end of the
 * last (HIP events), and the number of launches (0 and 0.0 for a table with no entry).  Either pointer may be NULL;
 * MC_ERR_INVALID_ARGUMENT before the first such bind.
 * mc_context_bound_bla_copy / mc_context_bound_bla_deep_copy read the context's bound tables back in exactly the layout of
 * mc_mandelbrot_orbit_bla_copy / mc_mandelbrot_orbit_bla_deep_copy, wherever the tables came from; *levels / *entries receive the
 * shape.  Any output pointer may be NULL (all NULL: query the shape).  MC_ERR_INVALID_ARGUMENT when nothing of that kind is bound. */
enum { MC_ORBIT_TABLE_BLA = 1u << 0, MC_ORBIT_TABLE_BLA_DEEP = 1u << 1 };
int mc_context_bind_mandelbrot_orbit_tables(mc_context* ctx, const mc_mandelbrot_orbit* o, uint32_t device_tables);
int mc_context_last_table_timing(mc_context* ctx, double* device_ms, uint32_t* launches);
int mc_context_bound_bla_copy(mc_context* ctx, double* out /* entries * 5 */, uint32_t* levels, uint64_t* entries);
int mc_context_bound_bla_deep_copy(mc_context* ctx, double* mant /* entries * 5 */, int32_t* exps /* entries * 3 */, uint32_t* levels,
                                   uint64_t* entries);

/* ---- exact counts of sampled pixels (the project's own addition, additions within ABI 3; what
 *      tests/mandel_exact_ref.py restates on Python integers).  Every deep mode returns ITS OWN loop's count; these calls iterate a
 *      pixel's c directly in the orbit's multi-limb fixed point and return the count that arithmetic gives, so a caller can spot-check
 *      a render, or find out whether its reference sits on the hair.
 *  - of the orbit object o three things are used: its centre c_ref AS THE FIXED-POINT NUMBER THE CONSTRUCTOR PARSED (sign, magnitude,
 *    round to odd: above), its `bits` and, for the offsets, its scale.  Never its table, length or max_iter.  An object of
 *    mc_mandelbrot_orbit_rescale carries its source's c_ref and bits.
 *  - limbs: k = ceil(bits / 64); n = k + 1 + extra_limbs 64-bit limbs are in use, F = 64 (n - 1) of their bits fractional; n > 131 is
 *    MC_ERR_UNSUPPORTED.  c_ref's limbs are extended by extra_limbs zero limbs at the low end: the same value.
 *  - per pixel: c = c_ref + (dcx, dcy) * 2^dc_exp2, dcx and dcy finite doubles (MC_ERR_INVALID_ARGUMENT otherwise), the sum EXACT: the
 *    offset times 2^F must be an integer.  If a bit of it would drop: MC_ERR_UNSUPPORTED, and mc_last_error_detail names the pixel's
 *    index (raise extra_limbs); nothing is ever truncated.  Either part of |c| above 4: MC_ERR_UNSUPPORTED, the index named likewise.
 *  - iteration, on integers scaled by 2^F, sign and magnitude: mul(a, b) = sign(a) sign(b) ((|a| |b| + 2^(F-1)) >> F), +0 when the
 *    magnitude is 0.
 *      zx = zy = sx = sy = 0; for j in [0, M):
 *        t = 2 mul(zx, zy);  zy' = t + cy;  zx' = (sx - sy) + cx;  sx = mul(zx', zx');  sy = mul(zy', zy');
 *        if (sx + sy > 2) { n = j; stop }
 *    n = M when the loop runs out: the counting of every render mode.  This is the orbit constructor's own loop without its doubles:
 *    for c = c_ref (offset 0), extra_limbs = 0 and M = the orbit's max_iter, n = L - 1 when the orbit escaped and M otherwise.
 *  - 1 <= n_pixels <= 2^20, 1 <= max_iter <= 2^32 - 2, no NULL pointer: MC_ERR_INVALID_ARGUMENT otherwise.  The offsets are the
 *    caller's: an F32 / DS / F64 render is checked with an orbit at centre "0", "0" of the view's scale and each pixel's double c as
 *    its offset.
 * mc_mandelbrot_exact_pixel_offsets (host only) writes the offsets THE PERTURBATION KERNELS USE for pixels (gx[i], gy[i]) of the
 * width x height view of o, the same expressions in source order: PERTURB's dc with *dc_exp2 = 0 for an orbit of the plain loop,
 * the rescaled loop's u with *dc_exp2 = E for a deep one.  gx[i] >= width or gy[i] >= height, width or height outside [1, 2^20],
 * n_pixels outside [1, 2^20], a NULL pointer: MC_ERR_INVALID_ARGUMENT.  Within that bound the 96 guard bits of the `bits` formula make
 * the conversion above exact with extra_limbs = 0: (g / W - 0.5) is a multiple of 2^-55 no smaller than 2^-22 when nonzero, so an offset's
 * last bit lies no lower than 2^-76 times the scale.
 * mc_mandelbrot_exact_counts: host, serial, no device: usable without a GPU; the reference form.
 * mc_mandelbrot_exact_counts_device: the same integers from ctx's device; blocking, on the context's stream; every refusal (the host
 * form's, with the same status and the same text after the function's name; ctx == NULL is MC_ERR_INVALID_ARGUMENT) comes before
 * anything is launched; neither the context's bound orbit nor its render scratch is touched.  The host builds every c and uploads the
 * limbs.  n <= 16: one pixel per WAVE (MC_EXACT_KERNEL_WAVE: a product's 4n <= 64 columns are the wave's lanes, its carries one ballot
 * word); n >= 17: one pixel per workgroup of 1024 threads, the device orbit's phases (MC_EXACT_KERNEL_WORKGROUP).  Iterations run in
 * slices of iters_per_launch, sized so that a launch stays near the device orbit's 50 ms; a pixel's state lives in device memory
 * between launches; the host reads one status / count word per pixel after each launch and stops when none is running.  That state
 * is 928 bytes per pixel for n <= 16 and 7424 bytes per pixel for n >= 17 whatever n is, once in host memory and once on the device
 * (2^20 pixels: 0.9 GiB and 7.3 GiB); MC_ERR_OUT_OF_MEMORY when either does not fit, before anything is launched.
 * mc_context_last_exact_timing: the last successful device call of the context (a call that fails leaves the record of the one
 * before): device_ms = first launch to the end of the last kernel
 * (HIP events; the reads between launches included), the launches, n, the slice length and which kernel ran.  Any pointer may be NULL;
 * MC_ERR_INVALID_ARGUMENT before the first such call. */
enum { MC_EXACT_KERNEL_WAVE = 1u, MC_EXACT_KERNEL_WORKGROUP = 2u };
int mc_mandelbrot_exact_pixel_offsets(const mc_mandelbrot_orbit* o, uint32_t width, uint32_t height, uint64_t n_pixels,
                                      const uint32_t* gx, const uint32_t* gy, double* dcx, double* dcy, int32_t* dc_exp2);
int mc_mandelbrot_exact_counts(const mc_mandelbrot_orbit* o, uint32_t max_iter, uint32_t extra_limbs, uint64_t n_pixels,
                               const double* dcx, const double* dcy, int32_t dc_exp2, uint32_t* out_n);
int mc_mandelbrot_exact_counts_device(mc_context* ctx, const mc_mandelbrot_orbit* o, uint32_t max_iter, uint32_t extra_limbs,
                                      uint64_t n_pixels, const double* dcx, const double* dcy, int32_t dc_exp2, uint32_t* out_n);
int mc_context_last_exact_timing(mc_context* ctx, double* device_ms, uint32_t* launches, uint32_t* limbs, uint32_t* iters_per_launch,
                                 uint32_t* kernel);
enum {
    /* bit 0 is a measurement switch of this repository (include/mc_compute_test.h), never set by a binding */
    MC_MANDEL_ITERS_U16 = 1u << 1,/* device form: d_iters is a uint16_t plane (max_iter <= 65535) — the multi-GPU exchange  */
                                  /* format, half of the 4-B plane and an eighth of the vec4 (mc_mandelbrot_assemble_...)  */
    /* bits 2 and 3 are measurement switches too */
    MC_MANDEL_COLOUR_EQUALISED = 1u << 4,/* histogram-equalised colouring of a WHOLE image (mc_mandelbrot_render and            */
                                  /* mc_mandelbrot_render_rgba8; the contract is below, at mc_mandelbrot_equalise_map)      */
    MC_MANDEL_SUPERSAMPLE_ADAPTIVE = 1u << 5,/* with MC_MANDEL_SUPERSAMPLE(s): only pixels whose count differs from a neighbour's  */
                                  /* get their s x s samples (the contract is below, at mc_context_last_refined)            */
    MC_MANDEL_COLOUR_SMOOTH = 1u << 6,/* smooth colouring by a fractional escape count (the contract is below, at           */
                                  /* mc_mandelbrot_render_smooth)                                                           */
    MC_MANDEL_COLOUR_DISTANCE = 1u << 7,/* the smooth colour shaded by a boundary distance estimate, of a WHOLE image (the      */
                                  /* contract is below, at mc_mandelbrot_render_distance); set WITHOUT MC_MANDEL_COLOUR_SMOOTH */
    /* bits 8-11: MC_MANDEL_SUPERSAMPLE(s) below */
    MC_MANDEL_COLOUR_SMOOTH_EQUALISED = 1u << 12,/* the smooth count ranked among a WHOLE image's escaped pixels (the contract is  */
                                  /* below, at mc_mandelbrot_render_smooth_equalised); set WITHOUT MC_MANDEL_COLOUR_SMOOTH     */
    MC_MANDEL_SUPERSAMPLE_SMOOTH = 1u << 13,/* with MC_MANDEL_SUPERSAMPLE(s) and ONE of the two smooth colourings: the s x s samples  */
                                  /* are smooth counts (the contract is below, at mc_mandelbrot_resolve_smooth_device_async)   */
    MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE = 1u << 14 /* with MC_MANDEL_SUPERSAMPLE(s) and ONE of the two smooth colourings, WITHOUT  */
                                  /* bits 5 and 13: only pixels whose smooth count is further than a threshold from a          */
                                  /* neighbour's get their s x s smooth samples (below, at mc_mandelbrot_render_adaptive_smooth) */
};
/* s x s supersampling, resolved on the device: bits 8-11 of flags hold s.  0 and 1: off (every call behaves as without the bits);
 * 2, 4, 8: valid; 3, 5, 6, 7, 9 .. 15: MC_ERR_INVALID_ARGUMENT.  The contract is below, at mc_mandelbrot_resolve_device_async. */
#define MC_MANDEL_SUPERSAMPLE(s) (((uint32_t)(s) & 15u) << 8)

typedef struct mc_mandelbrot_params {
    uint32_t width, height;   /* WIDTH/HEIGHT (mandelbrot.comp:5-6); reference 2000x2000 (main.cpp:20)  */
    uint32_t max_iter;        /* M (mandelbrot.comp:40); reference 128                                   */
    uint32_t precision;       /* MC_PRECISION_*                                                         */
    /* c = centre + (uv - 0.5) * scale (mandelbrot.comp:38); reference centre (-0.445, 0), scale 2.34   */
    /* on both axes.  *_lo are the low words for MC_PRECISION_DS and _F64 (hi=(float)d, lo=(float)(d-hi)). */
    float centre_x_hi, centre_x_lo, centre_y_hi, centre_y_lo;
    float scale_x_hi, scale_x_lo, scale_y_hi, scale_y_lo;
    float k_color[4];         /* push constant kColor (mandelbrotApp.h:139); reference {0.1,0.7,0.6,0}   */
    uint32_t row_begin, row_end; /* storage rows rendered by this call; 0,height for the whole image     */
    uint32_t row_block, row_stride; /* 0,0: the tile is the contiguous rows [row_begin,row_end).          */
                              /* Otherwise the tile is the rows row_begin + k*row_stride + j (j<row_block,   */
                              /* < row_end), stored compactly: tile row k*row_block + j (interleaved row     */
                              /* blocks, one residue class per GPU; see mc_tile_rows)                        */
    uint32_t flags;           /* MC_MANDEL_*                                                            */
    uint32_t reserved;
} mc_mandelbrot_params;

/* Fills p with the reference defaults for a W x H image (main.cpp:20, mandelbrot.comp:38-40). */
int mc_mandelbrot_default_params(uint32_t width, uint32_t height, mc_mandelbrot_params* p);

/* Host-buffer form (what MandelbrotApp::run + vkMapMemory give the reference, mandelbrotApp.h:149-155):
 * out_rgba_f32: (row_end-row_begin)*width*4 floats, may be NULL; out_iters: same pixel count of
 * uint32 iteration counts n in [0,max_iter], may be NULL.  At least one must be non-NULL. */
int mc_mandelbrot_render(mc_context* ctx, const mc_mandelbrot_params* p, float* out_rgba_f32, uint32_t* out_iters);

/* Device-buffer form (buffers already resident in HBM; pointers are device pointers on ctx's device).
 * Asynchronous on `stream` (a hipStream_t, NULL = the context's stream); either output may be NULL. */
int mc_mandelbrot_render_device_async(mc_context* ctx, const mc_mandelbrot_params* p, void* d_rgba_f32,
                                      void* d_iters, void* stream);

/* The (max_iter+1)-entry colour table: entry n = vec4 written for iteration count n
 * (mandelbrot.comp:50-56, evaluated on the host in fp32 source order).  lut_f32: (max_iter+1)*4. */
int mc_mandelbrot_colour_lut(uint32_t max_iter, const float k_color[4], float* lut_f32);

/* ---- histogram-equalised colouring (the project's own addition: the reference colours by t = n / M only, and on the views the deep
 *      precisions exist for the visible counts sit in a sliver of [0, M]; what tests/mandel_equalise_ref.py
 *      restates).  A pixel's palette position is its count's RANK among the image's escaped pixels.  For counts n in [0, M],
 *      M = max_iter, n = M meaning "did not escape":
 *  - hist[j], j in [0, M]: the number of pixels of the WHOLE image with n = j; uint32_t (an image has fewer than 2^32 pixels:
 *    width * height > 2^32 - 1 is MC_ERR_INVALID_ARGUMENT).
 *  - E = hist[0] + ... + hist[M-1] (the escaped pixels); C(j) = hist[0] + ... + hist[j-1], C(0) = 0.
 *  - the rank map, uint32_t map[M + 1]: map[M] = M; for j < M: map[j] = (M * C(j)) / E in unsigned 64-bit integer arithmetic, rounded
 *    down (both factors are below 2^32: the product cannot overflow); if E = 0, map[j] = 0 for j < M.  So map is non-decreasing, a
 *    count that occurs maps below M, and interior pixels keep the reference's t = 1 colour.
 *  - colour: lut[map[n]], lut the table of mc_mandelbrot_colour_lut(M, k_color): the equalised image draws from exactly the M + 1 vec4
 *    values the plain image draws from, and no new floating-point expression exists.  RGBA8 is mc_convert_rgba8's conversion (scale
 *    255, no rotation) of that, as for the plain colouring.
 * MC_MANDEL_COLOUR_EQUALISED in mc_mandelbrot_params.flags: mc_mandelbrot_render and mc_mandelbrot_render_rgba8 honour it for a whole
 * image (row_begin = 0, row_end = height, no interleave), in all six precisions: the count plane is rendered (no vec4 leaves the render
 * kernel), histogrammed, the table read back (4 (M + 1) bytes), mapped on the host, and the plane recoloured; out_iters still receives the
 * plain counts, and mc_context_last_timing's kernel time spans the whole chain, the table's round trip included.  Every call that cannot see
 * the whole image refuses the flag with MC_ERR_INVALID_ARGUMENT (mc_last_error_detail names the three calls below): a row tile or band of
 * those two, mc_mandelbrot_render_device_async, mc_mandelbrot_render_banded, mc_mandelbrot_assemble_device_async.  mc_multi_* refuse it
 * with MC_ERR_UNSUPPORTED.  mc_context_warmup_mandelbrot accepts it and makes the histogram and recolouring kernels resident too.
 * By hand (tiles, several devices, one palette over a zoom sequence), three calls:
 *
 * mc_mandelbrot_histogram_device_async ADDS the counts of n_pixels values at d_iters (iters_bytes = 2: uint16_t, 4: uint32_t; aligned to
 * their size) to d_hist, uint32_t[max_iter + 1] on the device, which the caller has zeroed: tiles, bands and devices accumulate into one
 * table.  A value above max_iter is counted in bin max_iter, never outside the table.  n_pixels > 2^32 - 1: MC_ERR_INVALID_ARGUMENT.  The
 * table is the same whatever order the adds arrive in.
 *
 * mc_mandelbrot_equalise_map (host only, no device): map from hist by the formula above.  NULL pointers or max_iter = 0:
 * MC_ERR_INVALID_ARGUMENT.  The histogram's total is NOT compared with any image's size (equalising over a crop, or over the frames of a
 * zoom sequence so that they share one palette, is a use); it is summed in 64 bits, and a total above 2^32 - 1 is
 * MC_ERR_INVALID_ARGUMENT (the product above could wrap).
 *
 * mc_mandelbrot_recolour_device_async writes lut[map[n]] to d_rgba_f32 for the tile p describes (contiguous or interleaved rows, stored
 * compactly, as everywhere); `map` is a HOST pointer to max_iter + 1 entries, each <= max_iter (MC_ERR_INVALID_ARGUMENT otherwise).
 * lut[map[.]] is composed on the host and kept as a device table of the context, like the colour table: one gather per pixel. */
int mc_mandelbrot_histogram_device_async(mc_context* ctx, const void* d_iters, uint32_t iters_bytes /* 2 or 4 */, uint64_t n_pixels,
                                         uint32_t max_iter, void* d_hist /* uint32_t[max_iter + 1] */, void* stream);
int mc_mandelbrot_equalise_map(uint32_t max_iter, const uint32_t* hist /* max_iter + 1 */, uint32_t* map /* max_iter + 1 */);
int mc_mandelbrot_recolour_device_async(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_iters, uint32_t iters_bytes,
                                        const uint32_t* map /* HOST, max_iter + 1 */, void* d_rgba_f32, void* stream);

/* ---- smooth colouring (the project's own addition: the reference colours by the integer count, one flat colour per count; DESIGN.md
 *      section 3.14; what tests/mandel_smooth_ref.py restates).  MC_MANDEL_COLOUR_SMOOTH in mc_mandelbrot_params.flags.  A pixel gets a
 *      SMOOTH COUNT q, a uint32_t in 24.8 fixed point: q / 256 is its fractional iteration count.
 *  - escape state: n is the pixel's count, unchanged.  For n < M (M = max_iter), (zx, zy) is the z of iteration i = n, the one whose test
 *    r > 2 succeeded, and (cx, cy) the pixel's c, both taken as doubles:
 *      F32: the two floats of z converted (exact); the pixel's float c from the c table, converted.
 *      DS: (double)hi + (double)lo of zx, zy; the same sum of the c table's pairs.
 *      F64: as they are; the c table's doubles.
 *      PERTURB, PERTURB_BLA: the loop's zx, zy (Z[m] + nd); c = (Z[1].x + dcx, Z[1].y + dcy).  Z_1 is c_ref correctly rounded.
 *      deep orbits, PERTURB_BLA_DEEP: the same zx, zy; c = (Z[1].x + ldexp(ux, E), Z[1].y + ldexp(uy, E)), ldexp correctly rounded, 0
 *      when it underflows.  For an orbit of the old scale this is the PERTURB row.
 *  - smooth_count(n, M, zx, zy, cx, cy), in IEEE double, no contraction, source order:
 *      if (n >= M) return 256 * M;
 *      k = 0;  r = (zx*zx) + (zy*zy);
 *      while (!(r > 65536.0) && k < 64) {            // a NaN keeps running to the cap
 *          t = ((zx*zx) - (zy*zy)) + cx;  zy = ((2.0*zx)*zy) + cy;  zx = t;  k++;  r = (zx*zx) + (zy*zy);
 *      }
 *      rf = (float)r;                                 // round to nearest even
 *      if (!(rf > 65536.0f)) rf = 65536.0f;           // the cap was hit, or NaN
 *      if (rf > FLT_MAX) rf = FLT_MAX;                // inf
 *      l = mc_log2(rf);  s = l * 0.0625f;  t = mc_log2(s);      // fp32; the strict log2 of the library (oracle: mc_math("log2")), op for op
 *      if (!(t > 0.0f)) t = 0.0f;  if (t > 1.0f) t = 1.0f;
 *      F = (uint32_t)(256.0f * (1.0f - t));          // 0 .. 256
 *      q = min(256 * (uint64_t)(n + k) + F, 256 * (uint64_t)M - 1);
 *    The fractional count is (n + k) + 1 - log2(log2 r / 16): continuous across the radius-256 threshold (r = 65536 gives +1, r = 65536^2
 *    gives +0, the value the pixel would have had one iteration earlier).  Interior pixels have q = 256 M exactly; an escaped pixel never
 *    reaches 256 M.  The flag needs max_iter <= 2^24 - 1 (MC_ERR_INVALID_ARGUMENT above).
 *  - colour: idx = q >> 8, fr = q & 255.  q = 256 M gives lut[M]; otherwise, per component, in fp32 with no contraction,
 *    a + ((b - a) * w) with a = lut[idx], b = lut[idx + 1], w = (float)fr * 0.00390625f, lut the table of mc_mandelbrot_colour_lut; alpha
 *    is 1.0f.  fr = 0 gives lut[idx].  RGBA8 is mc_convert_rgba8's conversion of that vec4, as everywhere.
 *  - KNOWN LIMIT: the reference's escape threshold is |z|^2 > 2, not 4, so some "escaped" pixels are in the set (the antenna near
 *    c = -1.9) or wander long before they leave.  Such pixels hit the 64-iteration cap and get q = 256 (n + 64) + 256: in F32, 52 of the
 *    115 093 escaped pixels of the reference view at 400 x 400, M = 128 (0.045 %; tests/test_mandel_smooth_host.py restates it); in F64,
 *    93 016 of the 39 321 599 escaped pixels of the K4 view at 7680 x 5120, M = 50 000 (0.24 %, measured on the device).  The continuation
 *    is 4 iterations in the median and 5 - 7 at the 95th percentile on those views.
 * Every single-device call that takes mc_mandelbrot_params honours the flag in all six precisions: mc_mandelbrot_render (out_iters still
 * receives n), mc_mandelbrot_render_device_async, mc_mandelbrot_render_rgba8 (whole images and bands), mc_mandelbrot_render_banded, row
 * tiles and interleaved tiles, MC_MANDEL_ITERS_U16 for the n plane, and mc_context_warmup_mandelbrot, which makes the smooth
 * instantiation resident.  Together with MC_MANDEL_COLOUR_EQUALISED, MC_MANDEL_SUPERSAMPLE(s >= 2) or MC_MANDEL_SUPERSAMPLE_ADAPTIVE it is
 * MC_ERR_INVALID_ARGUMENT (mc_last_error_detail says which: the rank map over fractional counts is MC_MANDEL_COLOUR_SMOOTH_EQUALISED, a flag
 * of its own, below; the resolve over fractional counts is asked for with MC_MANDEL_SUPERSAMPLE_SMOOTH beside the factor, further below); so it is
 * together with the measurement switch MC_MANDEL_FMA of mc_compute_test.h (the contraction switch has no smooth kernel).  The calls
 * that build colours from a plane of integer counts refuse it with MC_ERR_INVALID_ARGUMENT: mc_mandelbrot_recolour_device_async,
 * mc_mandelbrot_resolve_device_async, mc_mandelbrot_assemble_device_async (mc_mandelbrot_histogram_device_async takes no params and so
 * sees no flag: it counts whatever plane it is given).  mc_multi_* refuse it with MC_ERR_UNSUPPORTED.
 *
 * mc_mandelbrot_render_smooth / _device_async: p must carry the flag; any output may be NULL, at least one must be given; the smooth
 * plane is always uint32_t (the device form: aligned to 4), tiles are stored compactly as everywhere; the rest follows
 * mc_mandelbrot_render / mc_mandelbrot_render_device_async.
 * mc_mandelbrot_smooth_count and mc_mandelbrot_smooth_colour (host only, no device): the same source as the kernels' epilogue.
 * smooth_count: n <= max_iter <= 2^24 - 1.  smooth_colour writes count vec4 values for count q values; a q above 256 max_iter is
 * MC_ERR_INVALID_ARGUMENT. */
int mc_mandelbrot_render_smooth(mc_context* ctx, const mc_mandelbrot_params* p, float* out_rgba_f32, uint32_t* out_iters,
                                uint32_t* out_smooth);
int mc_mandelbrot_render_smooth_device_async(mc_context* ctx, const mc_mandelbrot_params* p, void* d_rgba_f32, void* d_iters,
                                             void* d_smooth, void* stream);
int mc_mandelbrot_smooth_count(uint32_t n, uint32_t max_iter, double zx, double zy, double cx, double cy, uint32_t* q);
int mc_mandelbrot_smooth_colour(uint32_t max_iter, const float k_color[4], const uint32_t* q, uint64_t count, float* out_rgba_f32);

/* ---- distance shading (the project's own addition: no colouring of counts shows filaments thinner than a pixel, a distance estimate does;
 *      DESIGN.md section 3.15; what tests/mandel_distance_ref.py restates).  MC_MANDEL_COLOUR_DISTANCE in mc_mandelbrot_params.flags.  The
 *      smooth count nu = q / 256 is the potential in disguise, G ~ 2^(-nu), so the exterior estimate d ~ 2 G / |grad G| is
 *      2 / (ln 2 |grad nu|): a function of the smooth plane alone, by finite differences between neighbouring pixels, in PIXEL PITCHES
 *      whatever the zoom depth, for every precision at once.
 *  - input: the WHOLE image's smooth plane q(y, x), uint32_t, W x H, storage rows; 256 M means interior (M = max_iter).
 *  - distance plane D, float per pixel, in pixel pitches:
 *      an interior pixel has D = 0.0f; an escaped pixel with an interior 4-neighbour inside the image has D = 0.0f; otherwise, differences
 *      as int64_t:
 *        gx = q(y, x+1) - q(y, x-1) for 0 < x < W-1; at a border the one-sided difference doubled: gx = 2 (q(y, 1) - q(y, 0)) at x = 0,
 *        gx = 2 (q(y, W-1) - q(y, W-2)) at x = W-1; gx = 0 when W = 1.  gy is the same along storage rows (y-1, y+1, H).
 *      then, in IEEE double, no contraction, source order:
 *        a = (double)gx;  b = (double)gy;  g2 = (a*a) + (b*b);
 *        g2 == 0: D = 4096.0f (above every other value: the largest, at g2 = 1, is 1477.3...);
 *        else D = (float)(1477.3197218702985 / sqrt(g2)), sqrt and the division correctly rounded, the conversion round-to-nearest-even.
 *      The constant is the double literal for 1024 / ln 2: the central difference spans two pixels and q carries 8 fractional bits.
 *      Differences reach 2^33, so g2 may exceed 2^53 and round: it is still one IEEE expression, the same on both sides.
 *  - colour, with threshold T (a finite float > 0, in pixels): an interior pixel gets lut[M], unchanged.  Every other pixel: base = the
 *    smooth colour of q (mc_mandelbrot_smooth_colour's expression); w = D >= T ? 1.0f : D / T, a correctly rounded fp32 division;
 *    rgb = base.rgb * w in fp32; alpha is 1.0f.  RGBA8 is mc_convert_rgba8's conversion of that vec4, as everywhere.
 *  - STATED LIMITS: pixel pitches assume square pixels; with scale_x / W != scale_y / H the two differences are each in their own pitch
 *    (documented, not corrected).  Below about two pixels the value is a shading weight, not a distance: it scatters and mostly reads low,
 *    i.e. darker (DESIGN.md section 3.15 has the measured agreement with the analytic estimate).  Smooth colouring's known limit carries
 *    over: pixels that hit the 64-iteration cap have steep q around them and come out dark.
 * The flag is a colouring of its own: it implies the smooth count and is set WITHOUT MC_MANDEL_COLOUR_SMOOTH.  mc_mandelbrot_render
 * (out_iters still receives n) and mc_mandelbrot_render_rgba8 honour it for WHOLE images only (row_begin = 0, row_end = height, no
 * interleave), in all six precisions, with T = 1.0f: the smooth render of the q plane through the existing kernels (no vec4 leaves the
 * render kernel), the stencil, for _rgba8 the conversion; q is scratch of the context, 4 bytes per pixel; mc_context_last_timing spans the
 * chain; max_iter <= 2^24 - 1 as for smooth.  MC_ERR_INVALID_ARGUMENT, mc_last_error_detail naming the flag and the calls to use: a row
 * tile or band of those two; the flag passed to mc_mandelbrot_render_device_async, mc_mandelbrot_render_banded,
 * mc_mandelbrot_render_smooth / _device_async, mc_mandelbrot_recolour_device_async, mc_mandelbrot_resolve_device_async or
 * mc_mandelbrot_assemble_device_async; the flag together with MC_MANDEL_COLOUR_SMOOTH, MC_MANDEL_COLOUR_EQUALISED,
 * MC_MANDEL_SUPERSAMPLE(s >= 2), MC_MANDEL_SUPERSAMPLE_ADAPTIVE or the measurement switch MC_MANDEL_FMA.  mc_multi_* refuse it with
 * MC_ERR_UNSUPPORTED.  mc_context_warmup_mandelbrot accepts it and makes the smooth instantiation and the stencil kernel resident;
 * mc_mandelbrot_supersample_params copies the bit like any other.
 *
 * mc_mandelbrot_render_distance: the blocking whole-image call with all four planes (colours, n, q, D); any output may be NULL, at least
 * one must be given; p must carry the flag; T = 1.0f.
 * mc_mandelbrot_distance_device_async: the stage by hand.  d_smooth is the WHOLE image's dense q plane (W x H uint32_t, aligned to 4),
 * what mc_mandelbrot_render_smooth_device_async wrote for the whole image; the outputs are the contiguous rows [row_begin, row_end) of p,
 * stored compactly, so a caller can band its output (interleave: MC_ERR_INVALID_ARGUMENT).  Either output may be NULL, not both;
 * d_distance_f32 is aligned to 4, d_rgba_f32 to 16; threshold_px must be finite and > 0; p carries the flag; the context's cached colour
 * table is used.
 * mc_mandelbrot_distance_plane and mc_mandelbrot_distance_colour (host only, no device): the same source as the kernel.  distance_plane
 * writes width * height floats; distance_colour writes count vec4 values from count (q, D) pairs.  A q above 256 max_iter, a NULL
 * pointer, a zero size, max_iter = 0 or above 2^24 - 1, or a threshold that is not finite and > 0: MC_ERR_INVALID_ARGUMENT. */
int mc_mandelbrot_render_distance(mc_context* ctx, const mc_mandelbrot_params* p, float* out_rgba_f32, uint32_t* out_iters,
                                  uint32_t* out_smooth, float* out_distance);
int mc_mandelbrot_distance_device_async(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_smooth, float threshold_px,
                                        void* d_distance_f32, void* d_rgba_f32, void* stream);
int mc_mandelbrot_distance_plane(uint32_t width, uint32_t height, uint32_t max_iter, const uint32_t* q, float* out_distance);
int mc_mandelbrot_distance_colour(uint32_t max_iter, const float k_color[4], const uint32_t* q, const float* distance, uint64_t count,
                                  float threshold_px, float* out_rgba_f32);

/* ---- smooth equalised colouring (the project's own addition; what tests/mandel_smooth_equalise_ref.py restates).
 *      MC_MANDEL_COLOUR_SMOOTH_EQUALISED in mc_mandelbrot_params.flags.  MC_MANDEL_COLOUR_EQUALISED uses the whole palette on a deep frame
 *      but draws one flat colour per count; MC_MANDEL_COLOUR_SMOOTH removes the steps but colours by q / (256 M), a sliver of the palette
 *      on such a frame.  This is the rank map over FRACTIONAL counts: the piecewise-linear cumulative distribution of the smooth plane with
 *      knots at the integer counts.  A function of the q plane alone, for every precision at once.  With M = max_iter <= 2^24 - 1 and q the
 *      smooth plane (256 M = interior, an escaped pixel has q <= 256 M - 1):
 *  - hist[j], j in [0, M]: the number of pixels of the WHOLE image with min(q >> 8, M) = j; uint32_t (width * height > 2^32 - 1 is
 *    MC_ERR_INVALID_ARGUMENT).  A q above 256 M counts in bin M.  This is NOT the histogram of n: the continuation's k iterations and a
 *    fraction F = 256 move pixels up, so q >> 8 is the key.
 *  - E = hist[0] + ... + hist[M-1] (the escaped pixels); C(j) = hist[0] + ... + hist[j-1], C(0) = 0.
 *  - the knot map, uint32_t qmap[M + 1]: qmap[M] = 256 M; for j < M: qmap[j] = (256 * M * C(j)) / E in unsigned 64-bit integer arithmetic,
 *    rounded down (256 * (2^24 - 1) * (2^32 - 1) < 2^64: the product cannot overflow); if E = 0, qmap[j] = 0 for j < M.
 *  - the remap q -> q': q >= 256 M gives q' = 256 M.  Otherwise j = q >> 8, f = q & 255, and
 *      q' = qmap[j] + (uint32_t)(((uint64_t)(qmap[j + 1] - qmap[j]) * f) >> 8).
 *  - CONSEQUENCES: q' is non-decreasing in q; an escaped pixel never reaches 256 M (bin j is occupied, so C(j) < E and qmap[j] < 256 M, and
 *    f <= 255 keeps q' below a larger next knot); qmap[j] >> 8 == mc_mandelbrot_equalise_map(hist)[j]; the share of escaped pixels below
 *    knot j is C(j) / E, and qmap[j] / (256 M) is within 1 / (256 M) of it.
 *  - colour: mc_mandelbrot_smooth_colour's expression applied to q'; no new floating-point expression exists, everything new is integer
 *    arithmetic.  RGBA8 is mc_convert_rgba8's conversion of that vec4, as everywhere.
 * The flag is a colouring of its own: it implies the smooth count and is set WITHOUT MC_MANDEL_COLOUR_SMOOTH
 * (MC_MANDEL_COLOUR_SMOOTH | MC_MANDEL_COLOUR_EQUALISED stays MC_ERR_INVALID_ARGUMENT).  mc_mandelbrot_render (out_iters still receives n)
 * and mc_mandelbrot_render_rgba8 honour it for WHOLE images only (row_begin = 0, row_end = height, no interleave), in all six precisions:
 * the smooth render of the q plane through the existing kernels (no vec4 leaves the render kernel), the histogram, the table's round trip
 * (4 (M + 1) bytes), the knot map on the host, the remap and its colour, for _rgba8 the conversion; n, q and q' are scratch of the context;
 * mc_context_last_timing spans the chain.  MC_ERR_INVALID_ARGUMENT, mc_last_error_detail naming the flag and the calls to use: a row tile
 * or band of those two; the flag passed to mc_mandelbrot_render_device_async, mc_mandelbrot_render_banded, mc_mandelbrot_render_smooth /
 * _device_async, mc_mandelbrot_render_distance, mc_mandelbrot_distance_device_async, mc_mandelbrot_recolour_device_async,
 * mc_mandelbrot_resolve_device_async or mc_mandelbrot_assemble_device_async; the flag together with MC_MANDEL_COLOUR_SMOOTH,
 * MC_MANDEL_COLOUR_EQUALISED, MC_MANDEL_COLOUR_DISTANCE, MC_MANDEL_SUPERSAMPLE(s >= 2), MC_MANDEL_SUPERSAMPLE_ADAPTIVE or the measurement
 * switch MC_MANDEL_FMA; max_iter > 2^24 - 1.  mc_multi_* refuse it with MC_ERR_UNSUPPORTED.  mc_context_warmup_mandelbrot accepts it and
 * makes the smooth instantiation and the two kernels below resident; mc_mandelbrot_supersample_params copies the bit like any other.
 *
 * mc_mandelbrot_render_smooth_equalised: the blocking whole-image call with all four planes (colours, n, q, q'); any output may be NULL, at
 * least one must be given; p must carry the flag.
 * By hand (tiles, one palette over a zoom sequence), three calls:
 * mc_mandelbrot_smooth_histogram_device_async ADDS the counts of n_pixels smooth counts at d_smooth (uint32_t, aligned to 4; any such
 * alignment) to d_hist, uint32_t[max_iter + 1] on the device, which the caller has zeroed: tiles and bands accumulate into one table.
 * n_pixels > 2^32 - 1 or max_iter > 2^24 - 1: MC_ERR_INVALID_ARGUMENT.  The table is the same whatever order the adds arrive in.
 * mc_mandelbrot_smooth_equalise_map (host only, no device): qmap from hist by the formula above.  NULL pointers, max_iter = 0 or above
 * 2^24 - 1: MC_ERR_INVALID_ARGUMENT.  The total is NOT compared with any image's size; it is summed in 64 bits, and a total above 2^32 - 1
 * is MC_ERR_INVALID_ARGUMENT.
 * mc_mandelbrot_smooth_remap (host only, no device): out_ranked[i] = q' of q[i] for count values.  A q above 256 max_iter, or a qmap that
 * decreases, has an entry above 256 max_iter or has qmap[max_iter] != 256 max_iter: MC_ERR_INVALID_ARGUMENT.
 * mc_mandelbrot_smooth_remap_device_async: q' (d_ranked, uint32_t, aligned to 4) and / or its colour (d_rgba_f32, aligned to 16) for the
 * tile p describes (contiguous or interleaved rows, stored compactly, as mc_mandelbrot_recolour_device_async); at least one output; p
 * carries the flag; `qmap` is a HOST pointer to max_iter + 1 knots, checked as mc_mandelbrot_smooth_remap checks them; a q above
 * 256 max_iter on the device is taken as interior.  The pairs (qmap[j], qmap[j + 1] - qmap[j]) are composed on the host and kept as a
 * device table of the context, like the colour table: one 8-byte gather per pixel. */
int mc_mandelbrot_render_smooth_equalised(mc_context* ctx, const mc_mandelbrot_params* p, float* out_rgba_f32, uint32_t* out_iters,
                                          uint32_t* out_smooth, uint32_t* out_ranked);
int mc_mandelbrot_smooth_histogram_device_async(mc_context* ctx, const void* d_smooth, uint64_t n_pixels, uint32_t max_iter,
                                                void* d_hist /* uint32_t[max_iter + 1] */, void* stream);
int mc_mandelbrot_smooth_equalise_map(uint32_t max_iter, const uint32_t* hist /* max_iter + 1 */, uint32_t* qmap /* max_iter + 1 */);
int mc_mandelbrot_smooth_remap(uint32_t max_iter, const uint32_t* qmap /* max_iter + 1 */, const uint32_t* q, uint64_t count,
                               uint32_t* out_ranked);
int mc_mandelbrot_smooth_remap_device_async(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_smooth,
                                            const uint32_t* qmap /* HOST, max_iter + 1 */, void* d_ranked /* or NULL */,
                                            void* d_rgba_f32 /* or NULL */, void* stream);

/* ---- s x s supersampling (the project's own addition: the reference takes ONE sample per pixel, at its corner, mandelbrot.comp:29-30;
 *      DESIGN.md section 3.11; what tests/mandel_supersample_ref.py restates).  MC_MANDEL_SUPERSAMPLE(s) in flags, s = 2, 4 or 8:
 *  - sample grid: an image W x H with factor s is sampled on the grid of the PLAIN image s*W x s*H with the same centre, scale, max_iter,
 *    precision and bound orbit: sample (s*y + i, s*x + j), i, j in [0, s), belongs to pixel (y, x), and its count is by definition the
 *    count the plain render of the s*W x s*H image gives at that position.  s*W and s*H must pass whatever the plain render demands.
 *  - colour of a pixel: with lut the M + 1 vec4 of mc_mandelbrot_colour_lut and n(i, j) the pixel's sample counts, per component in fp32,
 *    round-to-nearest, no contraction, sums by ADJACENT PAIRS, LEVEL BY LEVEL: tree(a_0 .. a_{k-1}) = a_0 for k = 1, else
 *    tree(a_0 + a_1, a_2 + a_3, ...); for k = 4: (a_0 + a_1) + (a_2 + a_3).  Row sums r_i = tree(lut[n(i,0)] .. lut[n(i,s-1)]), total
 *    t = tree(r_0 .. r_{s-1}), colour = t * (1.0f / (s*s)) — an exact scaling by a power of two.  A count above max_iter reads entry
 *    max_iter.  A pixel whose s*s samples share one count gets exactly lut[n], the plain colour (every partial sum is a power-of-two
 *    multiple of it): flat regions and the interior are bit-identical to the plain image; that is why only powers of two are offered.
 *    Alpha is exactly 1.0f.
 *  - with MC_MANDEL_COLOUR_EQUALISED: hist is the histogram of ALL s*s*W*H samples (s*s*W*H > 2^32 - 1: MC_ERR_INVALID_ARGUMENT), map is
 *    mc_mandelbrot_equalise_map of it, and lut[n] above becomes lut[map[n]].
 *  - RGBA8 is mc_convert_rgba8's conversion (scale 255, no rotation) of that vec4, as everywhere.
 * mc_mandelbrot_render (out_rgba_f32) and mc_mandelbrot_render_rgba8 honour the flag in all six precisions: the count plane of the sample
 * grid is rendered (uint16_t when max_iter <= 65535; no vec4 leaves the render kernel), [histogrammed and mapped when equalised,] and
 * resolved.  Plain colouring: whole images, contiguous row bands (render_rgba8) and row tiles (render) — a band's bytes are the whole
 * image's rows.  Equalised: whole images only.  out_iters with s >= 2 is MC_ERR_INVALID_ARGUMENT (a pixel has no single count: render
 * mc_mandelbrot_supersample_params' grid plainly).  mc_context_last_timing spans the whole chain.  The sample plane is scratch of the
 * context: 2 or 4 bytes x s*s x the tile's pixels (bound it with row bands, or with the device call below).
 * mc_mandelbrot_render_device_async, mc_mandelbrot_render_banded and mc_mandelbrot_assemble_device_async refuse s >= 2 with
 * MC_ERR_INVALID_ARGUMENT (mc_last_error_detail names the two calls below), mc_multi_* with MC_ERR_UNSUPPORTED.
 * mc_context_warmup_mandelbrot accepts it and makes the resolve kernel resident too.
 *
 * mc_mandelbrot_supersample_params (host only, no device): q = the plain-render parameters of p's sample grid: width, height, row_begin,
 * row_end, row_block and row_stride multiplied by s, the supersample bits, MC_MANDEL_COLOUR_EQUALISED and MC_MANDEL_SUPERSAMPLE_ADAPTIVE cleared, everything else copied
 * (q may be p; with MC_MANDEL_SUPERSAMPLE_SMOOTH set, see that bit's section below: the grid's smooth-render parameters).  A contiguous or interleaved tile of p is exactly the tile of q whose compact rows are, for each compact pixel row, its s
 * sample rows in order.  s = 0 or 1 multiplies by 1.  An invalid s, a product above 2^32 - 1 or a NULL pointer: MC_ERR_INVALID_ARGUMENT.
 *
 * mc_mandelbrot_resolve_device_async writes the colours of p's compact tile (p carries MC_MANDEL_SUPERSAMPLE(s), s = 2, 4, 8) to
 * d_rgba_f32 (16-byte aligned) from d_samples, what mc_mandelbrot_render_device_async(q) wrote for the same tile as counts of
 * iters_bytes = 4 (uint32_t) or 2 (uint16_t, MC_MANDEL_ITERS_U16; max_iter <= 65535), aligned to their size.  `map` is a HOST table of
 * max_iter + 1 entries, each <= max_iter, under mc_mandelbrot_recolour_device_async's rules and sharing its cached device table, or NULL
 * for the plain colouring.  Tiles, several devices and a caller's own banding compose this with the histogram call above. */
int mc_mandelbrot_supersample_params(const mc_mandelbrot_params* p, mc_mandelbrot_params* q);
int mc_mandelbrot_resolve_device_async(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_samples, uint32_t iters_bytes /* 2 or 4 */,
                                       const uint32_t* map /* HOST, max_iter + 1, or NULL */, void* d_rgba_f32, void* stream);

/* ---- adaptive supersampling (the project's own addition; what tests/mandel_adaptive_ref.py restates).
 *      MC_MANDEL_SUPERSAMPLE_ADAPTIVE in flags, valid only together with MC_MANDEL_SUPERSAMPLE(s), s = 2, 4 or 8 (alone:
 *      MC_ERR_INVALID_ARGUMENT from every call): a pixel gets its s*s samples only where its count differs from a neighbour's.
 *  - samples: the section above's, unchanged: sample (s*y + i, s*x + j) of pixel (y, x) has the count n(s*y + i, s*x + j) of the plain
 *    s*W x s*H render.
 *  - anchor: a(y, x) = n(s*y, s*x).  The anchor plane IS the plain W x H image's count plane, bit for bit, in every precision:
 *    (s*x) / (s*W) and x / W are the same float and the same double because s is a power of two, and the rest of a sample's arithmetic
 *    is a function of that quotient.
 *  - refined: pixel (y, x) is refined iff a(y', x') != a(y, x) for some (y', x') with |y' - y| <= 1, |x' - x| <= 1 inside the image
 *    (neighbours outside the image do not exist).
 *  - colour: a refined pixel gets the section above's colour of its s*s samples (the same pairwise tree, the same 1 / (s*s) scaling); any
 *    other pixel gets lut[a].  So the image equals the fully supersampled one on every pixel that is refined or whose samples share one
 *    count; the two differ only on unrefined pixels with mixed samples, which is the stated approximation.
 *  - with MC_MANDEL_COLOUR_EQUALISED: the histogram is the ANCHOR plane's (W*H values: the map is the plain equalised image's map), and
 *    lut[.] becomes lut[map[.]] for refined and unrefined pixels alike; an unrefined pixel is bit-identical to the plain equalised image.
 *  - the image is the same bits from run to run.
 * mc_mandelbrot_render (out_rgba_f32; out_iters refused as for every s >= 2) and mc_mandelbrot_render_rgba8 honour the bit in all six
 * precisions for WHOLE images only (row_begin = 0, row_end = height, no interleave; width * height <= 2^32 - 1, and s * width and
 * s * height <= 2^32 - 1 as for every s >= 2: the list render reads the sample grid's c table): a tile or band cannot
 * see its neighbours' anchors and is MC_ERR_INVALID_ARGUMENT, mc_last_error_detail saying so.  The chain: the plain W x H render (anchor
 * plane, uint16_t when max_iter <= 65535, and the plain colours), [its histogram, map and recolouring when equalised,] a device list of
 * the refined pixels, 4 bytes back to the host (the list's length), and a render of the list's samples that resolves each pixel between
 * the lanes that computed its samples; no sample plane exists (scratch: 2 or 4 bytes of anchor and 4 bytes of list per pixel).
 * mc_context_last_timing spans the whole chain.  mc_mandelbrot_resolve_device_async refuses the bit (it resolves a full plane); the calls
 * that refuse s >= 2 keep refusing; mc_multi_* answer MC_ERR_UNSUPPORTED.  mc_mandelbrot_supersample_params clears the bit in q.
 * mc_context_warmup_mandelbrot accepts it and makes the list and list-render kernels resident too.
 * It pays where the picture has bands or interior and costs where nearly every pixel is an edge (the plain pass comes on top): see the
 * use / do-not-use line of DESIGN.md section 3.12, and read the share of every call with:
 *
 * mc_context_last_refined: the refined pixels and the image's pixels of the context's last successful adaptive render; either pointer may
 * be NULL; MC_ERR_INVALID_ARGUMENT before the first such render. */
int mc_context_last_refined(mc_context* ctx, uint64_t* refined, uint64_t* pixels);

/* ---- smooth supersampling: the resolve over fractional counts (the project's own addition; what
 *      tests/mandel_smooth_supersample_ref.py restates).  MC_MANDEL_SUPERSAMPLE_SMOOTH in flags, valid only together with
 *      MC_MANDEL_SUPERSAMPLE(s), s = 2, 4 or 8, and EXACTLY ONE of MC_MANDEL_COLOUR_SMOOTH and MC_MANDEL_COLOUR_SMOOTH_EQUALISED: the
 *      anti-aliased, band-free image.  It composes two existing expressions and defines no new floating-point one.
 *  - samples: the supersampling section's, unchanged: sample (s*y + i, s*x + j) of pixel (y, x) is the pixel at that position of the
 *    plain smooth s*W x s*H render, and its smooth count q is whatever mc_mandelbrot_render_smooth gives there.
 *  - a sample's colour: mc_mandelbrot_smooth_colour's expression applied to q (a q >= 256 M gives lut[M]); with a knot map qmap, that
 *    expression applied to q', mc_mandelbrot_smooth_remap's expression of q.
 *  - a pixel's colour: the supersampling section's tree over those s*s vec4: sums by adjacent pairs, level by level, first inside a
 *    sample row, then over the row sums, then one multiply by 1.0f / (s*s); all fp32, round to nearest, no contraction; alpha is exactly
 *    1.0f.
 *  - CONSEQUENCES: (1) a pixel whose s*s samples share one q gets exactly the smooth colour of that q: interior and flat regions are
 *    bit-identical to the plain smooth image; (2) a plane whose fractions are all 0 (q = 256 n) gives, bit for bit, what
 *    mc_mandelbrot_resolve_device_async gives for the counts n; (3) the image does not depend on how pixels are grouped onto lanes.
 *  - ranked form (MC_MANDEL_COLOUR_SMOOTH_EQUALISED): hist is the histogram of min(q >> 8, M) over ALL s*s*W*H samples (more than
 *    2^32 - 1 samples: MC_ERR_INVALID_ARGUMENT), qmap is mc_mandelbrot_smooth_equalise_map of it, every sample is coloured through qmap.
 *  - limits: s in {2, 4, 8}; max_iter <= 2^24 - 1.
 * The pairs MC_MANDEL_COLOUR_SMOOTH | MC_MANDEL_SUPERSAMPLE(s) and MC_MANDEL_COLOUR_SMOOTH_EQUALISED | MC_MANDEL_SUPERSAMPLE(s) WITHOUT the
 * bit stay MC_ERR_INVALID_ARGUMENT as before (mc_last_error_detail now names the bit).  The bit alone, with s <= 1, with neither or both
 * colourings, or together with MC_MANDEL_SUPERSAMPLE_ADAPTIVE, MC_MANDEL_COLOUR_EQUALISED, MC_MANDEL_COLOUR_DISTANCE, MC_MANDEL_ITERS_U16
 * or the measurement switch MC_MANDEL_FMA is MC_ERR_INVALID_ARGUMENT, mc_last_error_detail naming the bit and what it needs.
 * mc_mandelbrot_render (out_rgba_f32; out_iters refused as for every s >= 2) and mc_mandelbrot_render_rgba8 honour it in all six
 * precisions.  MC_MANDEL_COLOUR_SMOOTH form: whole images, contiguous row bands and, for mc_mandelbrot_render, interleaved row tiles —
 * what plain supersampling serves; a band's bytes are the whole image's rows.  Ranked form: whole images only (the refusal is
 * MC_MANDEL_COLOUR_SMOOTH_EQUALISED's own).  The chain: the smooth render of the sample grid's q plane only (no n plane and no vec4 leave
 * the render kernel), [the smooth histogram over all samples, the table's round trip and the knot map when ranked,] the resolve, for
 * _rgba8 the conversion.  mc_context_last_timing spans the chain.  The q plane is scratch of the context and always uint32_t: 4 bytes x
 * s*s x the tile's pixels (7680 x 5120 at s = 4: 2.5 GB); bound it with row bands, or with the device call below.
 * mc_context_warmup_mandelbrot accepts the bit and makes the resolve kernel resident too; mc_mandelbrot_zoom_push renders through
 * mc_mandelbrot_render and so accepts it.  EVERY OTHER call that takes mc_mandelbrot_params refuses the bit by name with
 * MC_ERR_INVALID_ARGUMENT: mc_mandelbrot_render_device_async, _render_banded, _render_smooth / _device_async, _render_distance,
 * _distance_device_async, _render_smooth_equalised, _recolour_device_async, _resolve_device_async, _assemble_device_async,
 * _smooth_remap_device_async and the count-keyframe zoom calls; mc_multi_* answer MC_ERR_UNSUPPORTED.
 * mc_mandelbrot_supersample_params with the bit set clears it, keeps MC_MANDEL_COLOUR_SMOOTH and replaces
 * MC_MANDEL_COLOUR_SMOOTH_EQUALISED by MC_MANDEL_COLOUR_SMOOTH: q is directly the argument of mc_mandelbrot_render_smooth_device_async
 * for the sample grid.  Without the bit it behaves as before (the smooth bits are copied).
 *
 * mc_mandelbrot_resolve_smooth_device_async: the stage by hand, sibling of mc_mandelbrot_resolve_device_async.  p carries the bit, the
 * factor and one of the two colourings; d_smooth holds the compact sample rows of p's tile (contiguous or interleaved), uint32_t,
 * aligned to 4 (any such alignment); d_rgba_f32 is aligned to 16.  `qmap` is a HOST table of max_iter + 1 knots, checked as
 * mc_mandelbrot_smooth_remap_device_async checks it and sharing that call's cached pair table; it must be given exactly when p carries
 * MC_MANDEL_COLOUR_SMOOTH_EQUALISED.  The colour table is the context's cached one.  A q above 256 max_iter on the device is taken as
 * interior: no gather can leave a table.
 * mc_mandelbrot_resolve_smooth (host only, no device): the same source as the kernel.  q: (rows * s) x (s * width) smooth counts, dense;
 * qmap: max_iter + 1 knots or NULL; out_rgba_f32: rows * width vec4.  A NULL pointer (qmap excepted), a zero size, s outside {2, 4, 8},
 * max_iter = 0 or above 2^24 - 1, a q above 256 max_iter, or a qmap mc_mandelbrot_smooth_remap would refuse: MC_ERR_INVALID_ARGUMENT. */
int mc_mandelbrot_resolve_smooth_device_async(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_smooth,
                                              const uint32_t* qmap /* HOST, max_iter + 1, or NULL */, void* d_rgba_f32, void* stream);
int mc_mandelbrot_resolve_smooth(uint32_t max_iter, const float k_color[4], uint32_t s, uint32_t width, uint32_t rows, const uint32_t* q,
                                 const uint32_t* qmap /* max_iter + 1, or NULL */, float* out_rgba_f32);

/* ---- adaptive smooth supersampling: refine by a count threshold (the project's own addition, additions within ABI 3; what
 *      tests/mandel_adaptive_smooth_ref.py restates).  MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE in flags, valid only together with
 *      MC_MANDEL_SUPERSAMPLE(s), s = 2, 4 or 8, and EXACTLY ONE of MC_MANDEL_COLOUR_SMOOTH and MC_MANDEL_COLOUR_SMOOTH_EQUALISED, on a
 *      WHOLE image (row_begin = 0, row_end = height, no interleave), width * height <= 2^32 - 1, max_iter <= 2^24 - 1.  It is set WITHOUT
 *      MC_MANDEL_SUPERSAMPLE_ADAPTIVE (bit 5) and MC_MANDEL_SUPERSAMPLE_SMOOTH (bit 13).  It defines no new floating-point expression.
 *  - anchor: the anchor plane A is the plain smooth W x H render's q plane (uint32_t, 256 M = interior, M = max_iter), and
 *    a(y, x) = min(A(y, x), 256 M).  q of grid sample (s*y, s*x) IS A(y, x), bit for bit, in every precision (the argument of the
 *    adaptive section above, applied to the smooth count: a sample's q is a function of the same quotient).
 *  - refined: pixel (y, x) is refined iff |a(y, x) - a(y', x')| > tau for one of its up to eight neighbours (y', x') inside the image.
 *    The difference is formed without wrap (a > b ? a - b : b - a); tau is a uint32_t in units of 1/256 iteration.  tau = 0 is "differs
 *    at all"; tau >= 256 M refines nothing; an interior neighbour is just the value 256 M (there is no separate interior clause).
 *  - colour of a refined pixel: its s*s samples are the pixels (s*y + i, s*x + j) of the plain smooth s*W x s*H render (the smooth
 *    supersampling section's samples), each coloured by that section's sample colour, summed by the supersampling section's tree
 *    (adjacent pairs over the flattened index i*s + j) and multiplied once by 1.0f / (s*s); alpha is exactly 1.0f.  With
 *    MC_MANDEL_COLOUR_SMOOTH that is the full MC_MANDEL_SUPERSAMPLE_SMOOTH image's pixel, bit for bit.
 *  - colour of an unrefined pixel: the plain image's pixel, bit for bit (mc_mandelbrot_render with the colouring alone).
 *  - ranked form (MC_MANDEL_COLOUR_SMOOTH_EQUALISED): the histogram and the knot map are the ANCHOR plane's (W*H values: the plain
 *    smooth-equalised image's map, as the adaptive section does for MC_MANDEL_COLOUR_EQUALISED); unrefined pixels are that image's
 *    pixels and refined pixels send every sample through the same map.  This is NOT the full ranked MC_MANDEL_SUPERSAMPLE_SMOOTH call's
 *    map, which ranks all s*s*W*H samples: the two ranked images differ on refined pixels too.
 *  - the image does not depend on the order of the list or on how entries are grouped onto waves, and is the same bits from run to run.
 * MC_ERR_INVALID_ARGUMENT, mc_last_error_detail naming MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE and what it needs: the bit together with bit 5
 * or bit 13; with MC_MANDEL_COLOUR_EQUALISED, MC_MANDEL_COLOUR_DISTANCE, MC_MANDEL_ITERS_U16 or the measurement switch MC_MANDEL_FMA; the
 * bit alone, with s <= 1, or with neither or both colourings; a tile or band.  (Bits 5 and 13 together, without this bit, stay refused as
 * before.)
 * mc_mandelbrot_render (out_rgba_f32; out_iters refused as for every s >= 2) and mc_mandelbrot_render_rgba8 honour the bit in all six
 * precisions with the default tau = MC_MANDEL_ADAPTIVE_SMOOTH_THRESHOLD = 256: one iteration.  The chain: the plain smooth W x H render
 * (anchor plane, and the plain colours), [the anchor plane's smooth histogram, the table's round trip, the knot map and the plain ranked
 * colours,] a device list of the refined pixels, 4 bytes back to the host (the list's length), and a render of the list's samples that
 * resolves each pixel between the lanes that computed its samples.  No s*s-sized plane exists: the scratch is 4 bytes of anchor and 4
 * bytes of list per pixel beside the image.  mc_context_last_timing spans the chain; mc_context_last_refined reports the list's length
 * and width * height.  mc_context_warmup_mandelbrot accepts the bit and makes the refine and list kernels resident;
 * mc_mandelbrot_zoom_push renders through mc_mandelbrot_render and so accepts it.  mc_mandelbrot_supersample_params with the bit set clears
 * it, keeps MC_MANDEL_COLOUR_SMOOTH and replaces MC_MANDEL_COLOUR_SMOOTH_EQUALISED by it, exactly as for MC_MANDEL_SUPERSAMPLE_SMOOTH.
 * EVERY OTHER call that takes mc_mandelbrot_params refuses the bit by name with MC_ERR_INVALID_ARGUMENT: the calls listed for
 * MC_MANDEL_SUPERSAMPLE_SMOOTH above and mc_mandelbrot_resolve_smooth_device_async; mc_multi_* answer MC_ERR_UNSUPPORTED.
 * It pays where the picture has interior or slowly varying exterior and costs where nearly every pixel is refined (the plain pass comes on
 * top): see the use / do-not-use line of DESIGN.md section 3.28.
 *
 * mc_mandelbrot_render_adaptive_smooth: the same chain with the caller's tau.  p must carry the bit; at least one output must be given
 * (out_rgba_f32: width * height vec4; out_rgba8: width * height RGBA8, the conversion of mc_mandelbrot_render_rgba8).
 * mc_mandelbrot_refine_smooth (host only, no device): the rule on a caller's plane q of width * height smooth counts (values above
 * 256 max_iter are clamped, as the kernel clamps them).  mask: width * height bytes of 0 / 1, or NULL; refined: the number of refined
 * pixels, or NULL; not both NULL.  A zero size, max_iter = 0 or above 2^24 - 1, or a NULL q: MC_ERR_INVALID_ARGUMENT. */
#define MC_MANDEL_ADAPTIVE_SMOOTH_THRESHOLD 256u
int mc_mandelbrot_render_adaptive_smooth(mc_context* ctx, const mc_mandelbrot_params* p, uint32_t threshold,
                                         float* out_rgba_f32 /* or NULL */, uint8_t* out_rgba8 /* or NULL */);
int mc_mandelbrot_refine_smooth(uint32_t width, uint32_t height, uint32_t max_iter, const uint32_t* q, uint32_t threshold,
                                uint8_t* mask_or_NULL, uint64_t* refined_or_NULL);

/* ---- zoom sequences (the project's own addition: the reference renders one still; what tests/mandel_zoom_ref.py
 *      restates).  A zoom renders one KEYFRAME per octave (the scale halves from one to the next, the centre stays) and composes every
 *      frame in between from the two keyframes that bracket it: pure geometry in pixel units, one memory-bound kernel for all six
 *      precisions and every colouring.
 *  - inputs: two keyframes `wide` and `deep`, each W x H vec4 fp32 in storage rows, row-major, exactly what mc_mandelbrot_render writes;
 *    `deep` shows the same centre at half the scale of `wide` and may be absent (NULL).  r, a double in [0.5, 1]: the frame's scale is r
 *    times the wide keyframe's.
 *  - per output pixel (gx, gy), in IEEE double, no contraction, source order:
 *      X = (((double)gx - 0.5 * (double)W) * r) + 0.5 * (double)W;  Y the same with gy and H;
 *      r2 = r + r;  X2, Y2 the same expression with r2.
 *    source: the pixel reads `deep` at (X2, Y2) iff deep is present and 0 <= X2 <= W-1 and 0 <= Y2 <= H-1; otherwise `wide` at (X, Y).
 *  - taps at (X, Y) of the chosen image: x0 = clamp((int64)floor(X), 0, W-1), x1 = min(x0 + 1, W-1), rows the same with y0, y1;
 *    fx = (float)(X - (double)x0), fy likewise, converted round-to-nearest-even.  For W >= 2 the clamp of x0 never acts (X lies in
 *    [0, W-1]); it exists for W = 1 or H = 1.
 *  - value, per component in fp32, no contraction, a_yx the four taps, mix(a, b, f) = (f == 0.0f) ? a : a + ((b - a) * f):
 *      top = mix(a00, a01, fx);  bot = mix(a10, a11, fx);  v = mix(top, bot, fy);  alpha is exactly 1.0f.
 *    (The f == 0 case is what makes the identities below hold for EVERY input: the bare expression turns a -0.0f, which the distance
 *    shading writes, into +0.0f, and an infinite tap into NaN.  Everywhere else it is the bare expression.)
 *  - RGBA8 is mc_convert_rgba8's conversion (scale 255, no rotation) of that vec4.
 *  - consequences: r = 1 with deep absent gives `wide` bit for bit (X = gx exactly, every weight 0); r = 0.5 gives `deep` bit
 *    for bit on EVERY pixel (X2 = gx exactly); a linear ramp over the plane is reproduced to rounding.  On inputs in [0, 1] no component
 *    exceeds 1.0, so the byte conversion cannot wrap.
 *  - STATED LIMIT: the central region is `deep` minified by up to 2 x through one bilinear tap, which aliases; keyframes rendered with
 *    MC_MANDEL_SUPERSAMPLE are one answer, the area filter over the pixel's footprint the other (mc_mandelbrot_zoom_compose_filtered and
 *    mc_mandelbrot_zoom_frame_filtered with MC_MANDEL_ZOOM_FILTER_AREA, below; these calls themselves are unchanged).  MC_MANDEL_COLOUR_EQUALISED ranks each keyframe by
 *    itself, so the palette shifts between octaves (one map over a sequence: the by-hand histogram calls above; one map per FRAME that
 *    moves with the zoom: the count keyframes below, mc_mandelbrot_zoom_counts_*).
 *
 * mc_mandelbrot_zoom_ratio (host only): r = exp2(-(double)step / (double)steps_per_octave); exactly 1.0 at step 0 and exactly 0.5 at
 * step == steps_per_octave.  step > steps_per_octave or steps_per_octave == 0: MC_ERR_INVALID_ARGUMENT.  It exists so that an
 * application, a binding and a test take r from ONE place: two exp2 need not agree in the last bit, and one bit of r changes fx.
 * mc_mandelbrot_zoom_compose (host only, no device): the contract above on host buffers, the same source as the kernel.  At least one
 * output must be given; a NULL wide, a zero size, or r outside [0.5, 1] or NaN: MC_ERR_INVALID_ARGUMENT, mc_last_error_detail saying which.
 * mc_mandelbrot_zoom_compose_device_async: the stage by hand, on device pointers.  d_wide, d_deep and d_rgba_f32 are 16-byte aligned,
 * d_rgba8 4-byte aligned; either output may be NULL, not both; an output that overlaps a keyframe or the other output is refused;
 * asynchronous on `stream` (NULL: the context's).  The refusals above apply, all MC_ERR_INVALID_ARGUMENT.
 *
 * The sequence object.  mc_mandelbrot_zoom_create allocates two W x H vec4 slots on ctx's device (a failure: MC_ERR_OUT_OF_MEMORY); the
 * context must outlive it.  mc_mandelbrot_zoom_push renders p into a slot: exactly what mc_mandelbrot_render(ctx, p, out_rgba_f32, NULL)
 * would write, bit for bit, kept on the device with no host copy (the plain colouring renders straight into the slot; every other mode's
 * chain ends in the context's scratch and is copied device to device).  p is a whole image of the sequence's size (row_begin = 0,
 * row_end = height, no interleave, no MC_MANDEL_ITERS_U16: MC_ERR_INVALID_ARGUMENT otherwise) with any flag combination the blocking
 * whole-image render accepts with colours (plain, equalised, smooth, distance, smooth equalised, supersample, adaptive), in any precision - the three
 * perturbation precisions use the context's bound orbit - and the precision may change from one keyframe to the next.  The blocking
 * render's own refusals pass through unchanged.  The slots rotate: wide <- the previous keyframe, deep <- the new one.  From the second
 * push on the keyframe's scale must be EXACTLY half the previous keyframe's on both axes: for F32 / DS / F64 the view words read as
 * (double)hi + (double)lo, for the perturbation precisions the bound orbit's (scale_x, scale_y) * 2^scale_exp2, compared as (frexp
 * mantissa, exponent) pairs so that deep orbits compare exactly; a mismatch is MC_ERR_INVALID_ARGUMENT with both scales in
 * mc_last_error_detail, and the sequence is unchanged.  The CENTRE is the caller's responsibility: decimal text and float words cannot be
 * compared exactly, so it is not compared.  A push that is refused (MC_ERR_INVALID_ARGUMENT,
 * MC_ERR_UNSUPPORTED: its own refusals and the blocking render's) leaves the sequence as it was, with one keyframe held or two; after any
 * other failure (a HIP error, out of memory) the newest keyframe alone is left.
 * mc_mandelbrot_zoom_frame (blocking) composes the frame at r into either or both host outputs; with one keyframe pushed it composes from
 * that keyframe alone (deep absent), with none it is MC_ERR_INVALID_ARGUMENT.  The RGBA8 form is written by the compose kernel itself: no
 * vec4 frame is materialised.  Both calls fill mc_context_last_timing (push: copy_ms = 0) and use the context's scratch like any blocking
 * call; neither disturbs a later render on the context.  mc_multi_* is not involved. */
int mc_mandelbrot_zoom_ratio(uint32_t step, uint32_t steps_per_octave, double* r);
int mc_mandelbrot_zoom_compose(uint32_t width, uint32_t height, const float* wide, const float* deep /* or NULL */, double r,
                               float* out_rgba_f32 /* or NULL */, uint8_t* out_rgba8 /* or NULL */);
int mc_mandelbrot_zoom_compose_device_async(mc_context* ctx, uint32_t width, uint32_t height, const void* d_wide, const void* d_deep,
                                            double r, void* d_rgba_f32, void* d_rgba8, void* stream);
typedef struct mc_mandelbrot_zoom mc_mandelbrot_zoom;
int mc_mandelbrot_zoom_create(mc_context* ctx, uint32_t width, uint32_t height, mc_mandelbrot_zoom** out);
int mc_mandelbrot_zoom_push(mc_mandelbrot_zoom* z, const mc_mandelbrot_params* p);
int mc_mandelbrot_zoom_frame(mc_mandelbrot_zoom* z, double r, float* out_rgba_f32, uint8_t* out_rgba8);
int mc_mandelbrot_zoom_destroy(mc_mandelbrot_zoom* z);

/* ---- zoom sequences from COUNT keyframes (the project's own addition; what tests/mandel_zoom_counts_ref.py
 *      restates).  The sequence above keeps a keyframe as colours, so with the two equalised colourings an in-between frame shows two rank
 *      maps side by side, along the rectangle of the deep keyframe.  Here a keyframe is a plane of uint32_t - the count n, or for the two
 *      smooth colourings the smooth count q - and a frame colours the taps of BOTH keyframes through ONE map that moves with the zoom.  A
 *      count keyframe is 4 bytes per pixel instead of 16, so the same calls also serve the plain and the smooth colouring.
 *  - M = max_iter.  The colouring is the colour bits of p->flags: exactly one of 0 (plain), MC_MANDEL_COLOUR_EQUALISED,
 *    MC_MANDEL_COLOUR_SMOOTH, MC_MANDEL_COLOUR_SMOOTH_EQUALISED.
 *  - the moving map, mc_mandelbrot_zoom_blend_map (host only, no device): with s = step, S = steps_per_octave, S >= 1, s <= S,
 *      out[j] = (map_wide[j] * (S - s) + map_deep[j] * s) / S    in unsigned 64-bit arithmetic, rounded down, j < entries.
 *    Every entry must be <= 256 * (2^24 - 1) (MC_ERR_INVALID_ARGUMENT otherwise): entries and weights are below 2^32 and the weights sum
 *    to S, so no product and no sum can reach 2^64.  It serves the rank map (entries <= M) and the knot map (entries <= 256 M).
 *    Consequences: s = 0 gives map_wide and s = S gives map_deep, exactly; non-decreasing inputs give a non-decreasing output; out[j] lies
 *    between the two inputs; an entry equal in both (map[M] = M, qmap[M] = 256 M) is kept; for 0 < s < S a count that is occupied in
 *    either keyframe maps BELOW the top entry, because one of the two inputs is below it and its weight is at least 1, so an escaped tap
 *    never takes the interior colour.  STATED, not corrected: at s = 0 with a deep keyframe present, a deep tap whose count no wide pixel
 *    reaches may take the interior colour (the applications never compose that frame: step 0 is the previous octave's last frame).
 *  - a tap's colour, from a plane of uint32_t, lut being mc_mandelbrot_colour_lut(M, k_color):
 *      plain             lut[min(n, M)]
 *      equalised         lut[map[min(n, M)]]
 *      smooth            mc_mandelbrot_smooth_colour's expression of q
 *      smooth equalised  that expression of mc_mandelbrot_smooth_remap's q'
 *    No new floating-point expression exists.  `map` is NULL for plain and smooth and required for the other two (M + 1 entries, a HOST
 *    table), checked as mc_mandelbrot_recolour_device_async (no entry above M) and mc_mandelbrot_smooth_remap (non-decreasing knots, the
 *    last one 256 M) check theirs.  A q above 256 M is MC_ERR_INVALID_ARGUMENT on the host and is taken as interior on the device, as in
 *    mc_mandelbrot_smooth_remap_device_async.
 *  - a frame is mc_mandelbrot_zoom_compose's contract, unchanged, applied to those tap colours (positions, source test, taps, mix with
 *    its f == 0 case, alpha 1, the RGBA8 conversion).  Bit for bit:
 *      frame = mc_mandelbrot_zoom_compose(colour(wide), colour(deep), r).
 *
 * mc_mandelbrot_zoom_compose_counts (host only, the same source as the kernel) and mc_mandelbrot_zoom_compose_counts_device_async (the
 * stage by hand; asynchronous on `stream`, NULL: the context's).  p supplies width, height, max_iter, k_color and the colouring; it is a
 * whole image (row_begin = 0, row_end = height) with no interleave and no MC_MANDEL_ITERS_U16; precision and view words are not read.
 * Refusals, all MC_ERR_INVALID_ARGUMENT with mc_last_error_detail naming the call: mc_mandelbrot_zoom_compose_device_async's (here the
 * keyframes and d_rgba8 4-byte aligned, d_rgba_f32 16-byte aligned; an output that overlaps a keyframe or the other output; r outside
 * [0.5, 1] or NaN; no output); more than one colour bit; MC_MANDEL_COLOUR_DISTANCE, MC_MANDEL_SUPERSAMPLE(s >= 2),
 * MC_MANDEL_SUPERSAMPLE_ADAPTIVE or the measurement switch of mc_compute_test.h that contracts the fp32 render; a map where none belongs,
 * or none where one does; max_iter above 2^24 - 1 for the two smooth colourings.
 *
 * The sequence object.  mc_mandelbrot_zoom_counts_create allocates two slots of 4 bytes per pixel on ctx's device (a failure:
 * MC_ERR_OUT_OF_MEMORY; width * height above 2^32 - 1: MC_ERR_INVALID_ARGUMENT); the context must outlive it.
 * mc_mandelbrot_zoom_counts_push renders p's count plane straight into a slot through the device forms (the n plane alone, or for the two
 * smooth colourings the q plane alone; no vec4 leaves the render kernel), in all six precisions - the perturbation precisions use the
 * context's bound orbit.  For the two equalised colourings it then runs the histogram kernel over the slot, reads the table back
 * (4 (M + 1) bytes) and builds the rank map (mc_mandelbrot_equalise_map) or the knot map (mc_mandelbrot_smooth_equalise_map) on the host;
 * the map is kept with the slot, on the host and on the device.  mc_mandelbrot_zoom_push's rules carry over: a whole image of the
 * sequence's size, the exact-halving test on (frexp mantissa, exponent) pairs from the second push on, the slots' rotation, and the state
 * after a refusal (the sequence as it was) or any other failure (the newest keyframe alone).  The first push fixes the colouring,
 * max_iter and k_color; a later push that differs in one of them is MC_ERR_INVALID_ARGUMENT.  The precision may change between keyframes.
 * mc_context_last_timing spans the chain, copy_ms = 0.
 * mc_mandelbrot_zoom_counts_frame (blocking) composes the frame at r = mc_mandelbrot_zoom_ratio(step, steps_per_octave) into either or
 * both host outputs.  With two keyframes the frame's map is the blend above at (step, steps_per_octave), built ON THE DEVICE from the two
 * device maps by a table kernel (one thread per entry) that writes lut[map_f[.]] or the (knot, step) pairs the remap gathers from; then
 * the compose kernel and the copy to the host, with no other host round trip.  With one keyframe: that keyframe alone with its own map, at
 * any step.  With none: MC_ERR_INVALID_ARGUMENT.
 * mc_mandelbrot_zoom_counts_maps copies the maps of the keyframes held, M + 1 entries each (either pointer may be NULL; with one keyframe
 * held it is both the wide and the deep one).  MC_ERR_INVALID_ARGUMENT for the plain or the smooth colouring, or before a push.
 * Identities: frame(step = steps_per_octave) is the deep keyframe's own mc_mandelbrot_render image with that colouring, bit for bit;
 * frame(0) with one keyframe is that keyframe's image; in EVERY frame a pixel whose four taps share one count n gets exactly the tap
 * colour of n under the frame's map, whichever keyframe it read (no seam: the vec4 sequence violates this wherever the two keyframes' maps
 * differ).
 * STATED LIMITS: a palette position still changes over time at a fixed point of the plane, continuously, through the blend; the blend is
 * linear in step, not in the histograms; in these calls one bilinear tap still aliases the minified centre and count keyframes cannot be
 * supersampled: mc_mandelbrot_zoom_compose_counts_filtered and mc_mandelbrot_zoom_counts_frame_filtered with MC_MANDEL_ZOOM_FILTER_AREA
 * (below) filter it over the pixel's footprint (distance shading, supersampling and adaptive supersampling stay with the vec4
 * sequence); one GPU. */
int mc_mandelbrot_zoom_blend_map(uint32_t entries, const uint32_t* map_wide, const uint32_t* map_deep, uint32_t step,
                                 uint32_t steps_per_octave, uint32_t* out);
int mc_mandelbrot_zoom_compose_counts(const mc_mandelbrot_params* p, const uint32_t* wide, const uint32_t* deep /* or NULL */,
                                      const uint32_t* map /* or NULL */, double r, float* out_rgba_f32 /* or NULL */,
                                      uint8_t* out_rgba8 /* or NULL */);
int mc_mandelbrot_zoom_compose_counts_device_async(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_wide, const void* d_deep,
                                                   const uint32_t* map /* HOST, or NULL */, double r, void* d_rgba_f32, void* d_rgba8,
                                                   void* stream);
typedef struct mc_mandelbrot_zoom_counts mc_mandelbrot_zoom_counts;
int mc_mandelbrot_zoom_counts_create(mc_context* ctx, uint32_t width, uint32_t height, mc_mandelbrot_zoom_counts** out);
int mc_mandelbrot_zoom_counts_push(mc_mandelbrot_zoom_counts* z, const mc_mandelbrot_params* p);
int mc_mandelbrot_zoom_counts_frame(mc_mandelbrot_zoom_counts* z, uint32_t step, uint32_t steps_per_octave, float* out_rgba_f32,
                                    uint8_t* out_rgba8);
int mc_mandelbrot_zoom_counts_maps(mc_mandelbrot_zoom_counts* z, uint32_t* wide_map /* or NULL */, uint32_t* deep_map /* or NULL */);
int mc_mandelbrot_zoom_counts_destroy(mc_mandelbrot_zoom_counts* z);

/* ---- zoom sequences: the area filter of the minified deep keyframe (the project's own addition, additions within ABI 3; DESIGN.md section
 *      3.23; what tests/mandel_zoom_filter_ref.py restates).  A frame at r reads the deep keyframe minified by r2 = 2 r in [1, 2]: an output
 *      pixel's footprint there is a box of width r2, and one bilinear tap (a box of width 1) skips up to half of the texels.  Each call
 *      below is its unfiltered namesake with one more argument, `filter`:
 *        MC_MANDEL_ZOOM_FILTER_BILINEAR (0): exactly what the namesake returns - the same bits, the same statuses, the same detail text after
 *          the function's name, the same kernel.
 *        MC_MANDEL_ZOOM_FILTER_AREA (1): the box filter below on the pixels that read `deep`.
 *      Any other value is MC_ERR_INVALID_ARGUMENT with the value in mc_last_error_detail.  Every refusal of the namesake carries over
 *      (alignment, overlap, r outside [0.5, 1] or NaN, no output, the colouring rules of the count calls) and is checked before the filter.
 *  - MC_MANDEL_ZOOM_FILTER_AREA.  Positions, r2, X2, Y2 and the source test are mc_mandelbrot_zoom_compose's, unchanged.  A pixel that reads
 *    `wide` is computed exactly as there (wide is magnified: its footprint is under one texel, and a box of width 1 over texel cells is
 *    the bilinear tap).  A pixel that reads `deep` takes the box of width r2 centred at (X2, Y2) over the texel cells [k - 0.5, k + 0.5].
 *  - per axis (columns with X2 and W, rows with Y2 and H), in IEEE double, no contraction, source order:
 *      h = 0.5 * r2;  a = X2 - h;  b = X2 + h;
 *      fl = floor(a);  k0 = (int64)fl + (a >= fl + 0.5 ? 1 : 0);
 *    (k0 is floor(a + 0.5) without that sum's rounding: fl and fl + 0.5 are exact, so k0 is exactly the cell that holds a, a lower end on
 *    a cell boundary going to the cell above.)  Three cells k = k0, k0 + 1, k0 + 2 - an interval of length at most 2 that starts in cell
 *    k0 touches no other - each with
 *      lo = max(a, (double)k - 0.5);  hi = min(b, (double)k + 0.5);  d = hi - lo;  w_k = (float)(d > 0 ? d : 0)
 *    converted round-to-nearest-even, and the tap index clamp(k, 0, W-1): the border replicates, because the footprint may reach half a
 *    texel past the image (cell -1 or W).  A box that ends exactly on a cell boundary leaves the cell above at weight 0.
 *  - value, per component in fp32, no contraction, a_yx the nine taps, wy_y and wx_x the weights above: visit the taps in row-major
 *    order (y outer, x inner); p = wy_y * wx_x; a tap with p == 0.0f is skipped; the first tap kept sets acc = p * a_yx and sw = p, every
 *    later one acc = acc + (p * a_yx) and sw = sw + p;  v = acc / sw, correctly rounded;  alpha is exactly 1.0f.  RGBA8 is
 *    mc_convert_rgba8's conversion (scale 255, no rotation) of that vec4, as everywhere.  (The skip is what makes the identities hold for
 *    EVERY input: 0 * inf is NaN, and -0.0f + 0.0f loses the sign.  A NaN tap of non-zero weight gives NaN; which NaN is not specified.)
 *  - consequences, for every input, -0.0f, infinite and NaN taps included: r = 0.5 gives `deep` bit for bit on EVERY pixel (X2 = gx
 *    exactly, a = gx - 0.5, one tap of weight 1.0f, (1 * a) / 1; a NaN tap comes back a NaN); r = 1 with deep absent gives `wide` bit
 *    for bit; on no pixel outside the deep-sourced rectangle does the AREA frame differ from the BILINEAR frame.  A constant plane c is reproduced exactly where c is
 *    0 or a power of two (every product p * c is exact, so acc = c * sw through the same roundings), and otherwise to within the
 *    roundings of at most nine products, eight additions in each sum and one division: (1 + 2^-24)^19 - 1 < 2^-21 relative; the restatement
 *    measures at most 6.3 x 2^-24.  On inputs in [0, 1] no component exceeds 1.0 (each p * a_yx is at most p, rounding and addition are
 *    monotone, so acc <= sw), so the byte conversion cannot wrap.
 *  - count keyframes: the tap colours are the count keyframes' own, unchanged (plain, equalised, smooth, smooth equalised through the
 *    frame's one map), nine per deep-sourced pixel; no new floating-point expression exists beyond the filter above.  Bit for bit:
 *      frame = mc_mandelbrot_zoom_compose_filtered(colour(wide), colour(deep), r, filter).
 *
 * mc_mandelbrot_zoom_compose_filtered and mc_mandelbrot_zoom_compose_counts_filtered are host only, the same source as the kernels.
 * The _device_async forms are the stages by hand.  mc_mandelbrot_zoom_frame_filtered and mc_mandelbrot_zoom_counts_frame_filtered compose
 * from the existing sequence objects (nothing about push changes) and fill mc_context_last_timing as the _frame calls do; the RGBA8 form
 * is written by the kernel itself.  frame_filtered(r = 0.5), or (step = steps_per_octave), is the deep keyframe's own render, bit for bit,
 * with either filter.
 * STATED LIMITS: one GPU; no filter wider than the footprint (a box, not a windowed kernel: it removes what one tap skips, it does not
 * band-limit); with keyframes of one sample per pixel the sharpness of the centre still varies over an octave (the last frame before a
 * keyframe is a box of width ~1, the first a box of width 2; DESIGN.md section 3.23 has the measured table); distance shading and
 * supersampling stay with colour keyframes. */
enum { MC_MANDEL_ZOOM_FILTER_BILINEAR = 0, MC_MANDEL_ZOOM_FILTER_AREA = 1 };
int mc_mandelbrot_zoom_compose_filtered(uint32_t width, uint32_t height, const float* wide, const float* deep /* or NULL */, double r,
                                        uint32_t filter, float* out_rgba_f32 /* or NULL */, uint8_t* out_rgba8 /* or NULL */);
int mc_mandelbrot_zoom_compose_filtered_device_async(mc_context* ctx, uint32_t width, uint32_t height, const void* d_wide, const void* d_deep,
                                                     double r, uint32_t filter, void* d_rgba_f32, void* d_rgba8, void* stream);
int mc_mandelbrot_zoom_compose_counts_filtered(const mc_mandelbrot_params* p, const uint32_t* wide, const uint32_t* deep /* or NULL */,
                                               const uint32_t* map /* or NULL */, double r, uint32_t filter,
                                               float* out_rgba_f32 /* or NULL */, uint8_t* out_rgba8 /* or NULL */);
int mc_mandelbrot_zoom_compose_counts_filtered_device_async(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_wide,
                                                            const void* d_deep, const uint32_t* map /* HOST, or NULL */, double r,
                                                            uint32_t filter, void* d_rgba_f32, void* d_rgba8, void* stream);
int mc_mandelbrot_zoom_frame_filtered(mc_mandelbrot_zoom* z, double r, uint32_t filter, float* out_rgba_f32, uint8_t* out_rgba8);
int mc_mandelbrot_zoom_counts_frame_filtered(mc_mandelbrot_zoom_counts* z, uint32_t step, uint32_t steps_per_octave, uint32_t filter,
                                             float* out_rgba_f32, uint8_t* out_rgba8);

/* ---- atom domains: locating minibrots (the project's own addition, additions within ABI 3; what
 *      tests/mandel_atom_ref.py restates).  Every deep call needs a centre written to about as many digits as its depth; these calls find
 *      one.  The ATOM-DOMAIN PERIOD of a pixel is the iteration index at which |z| is smallest: atom domains surround every nucleus
 *      (the centre of a minibrot, where z_p(c) = 0) and are far larger than the minibrot itself, so a coarse render finds them; Newton's
 *      method on z_p(c) = 0 from the domain's best pixel lands on the nucleus; the nucleus written as text is the centre of the dive.
 *      New entry points only: no flag bit selects any of this and mc_mandelbrot_params.flags must be 0 here.
 *
 * THE PERIOD PLANE.  mc_mandelbrot_render_atom (blocking, on the context's stream) and mc_mandelbrot_render_atom_device_async render p's
 * whole image into up to three row-major planes (any may be NULL, not all): the counts n (uint32_t), the periods (uint32_t) and amin (double).
 *  - the per-precision loop is unchanged; n is the count every render returns, and the n plane is bit for bit the plain render's.
 *  - z_m (m = 1 .. n) is the z that the m-th iteration formed and whose escape test failed, handed over as two doubles exactly as the
 *    smooth kernels' escape z is: exact conversions of the two floats for F32, the doubles themselves for F64, and for PERTURB
 *    Z[m] + d with the loop's m and d after the iteration's rebase decision, d itself after a rebase (m = 0: Z_0 = 0 is not added).
 *  - a_m = max(|x_m|, |y_m|) in double: exact, two abs and one max.  The max-norm and not x^2 + y^2 on purpose: at a scale of 1e-280 the
 *    |z|^2 of a pixel near a nucleus underflows double, the max-norm does not.
 *  - period = the smallest m in [1, n] with a_m < a_j for all j < m and a_m <= a_j for all j: start from best = +inf, period = 0 and
 *    take (a_m, m) when a_m < best, strictly, for m = 1 .. n in order.  A z_m with a NaN part never updates.  amin = that a_m.
 *    n = 0 (or nothing but NaNs) gives period 0 and amin = +inf.  Interior pixels use n = max_iter.
 *  - F32 and F64 keep their cycle exit: a lane found to cycle has already seen every value its orbit will ever take, and the update is
 *    strict, so the planes are those of the loop run to max_iter (DESIGN.md section 3.33 gives the argument, a test holds it).
 *  - precisions: MC_PRECISION_F32, MC_PRECISION_F64, and MC_PRECISION_PERTURB with a bound orbit of the plain loop (min |scale| >= 2^-960;
 *    PERTURB's rules for the view words, the binding and max_iter: MC_ERR_INVALID_ARGUMENT).  MC_ERR_UNSUPPORTED, named in
 *    mc_last_error_detail: MC_PRECISION_DS; a deep bound orbit (its z leaves the double range; a floatexp amin is a follow-up);
 *    MC_PRECISION_PERTURB_BLA and MC_PRECISION_PERTURB_BLA_DEEP (a skip does not visit its iterations).
 *  - MC_ERR_INVALID_ARGUMENT: any nonzero flags; rows other than the whole image (row_begin = 0, row_end = height, no interleave); all
 *    three outputs NULL; a zero width, height or max_iter.
 *  - every iteration of these kernels is an exact step (the plain kernels' fast blocks are not used: a block that carries the minimum
 *    through its accumulator is an optimisation left out), so the period plane costs more than a frame of the same size: render it
 *    coarse.  Atom domains are large.
 * mc_mandelbrot_atom_scan (host only) runs the same update, the one source the kernels compile, over a caller's sequence
 * z_1 .. z_n (n x 2 doubles: re, im); z may be NULL when n = 0.
 * Inside a hyperbolic component the minimum can fall on a MULTIPLE of the component's period (pixels of the period-2 disc report 4, and
 * Newton with p = 4 goes to the same nucleus, -1): the plane is as defined above; sorting out multiples is the caller's policy. */
int mc_mandelbrot_render_atom(mc_context* ctx, const mc_mandelbrot_params* p, uint32_t* out_iters, uint32_t* out_period, double* out_amin);
int mc_mandelbrot_render_atom_device_async(mc_context* ctx, const mc_mandelbrot_params* p, void* d_iters, void* d_period, void* d_amin,
                                           void* stream);
int mc_mandelbrot_atom_scan(const double* z /* n x 2 */, uint32_t n, uint32_t* period, double* amin);
/* THE DOMAINS OF A PLANE: for each period v in [0, max_iter], over the n_pixels < 2^32 pixels of a period plane and its amin plane,
 *    count[v] = the number of pixels with period == v;
 *    amin[v]  = the smallest amin among those pixels, +inf when there is none;
 *    pixel[v] = the lowest linear index among the pixels attaining it, 0xffffffff when there is none.
 * amin values are ordered by their bit patterns as uint64_t, which for the values the atom render writes (non-negative, or +inf) is their
 * numeric order; a value whose pattern lies above +inf's (a negative, a NaN) is counted but takes no part in amin[v] or pixel[v].
 * mc_mandelbrot_atom_domains: host planes into host tables of max_iter + 1 entries each; a period above max_iter is
 * MC_ERR_INVALID_ARGUMENT (the pixel is named).  mc_mandelbrot_atom_domains_device_async: device planes into device tables, which it
 * initialises itself, in stream order: count is mc_mandelbrot_histogram_device_async's histogram of the period plane (so a period above
 * max_iter is counted in count[max_iter], that call's clamp) and is IGNORED by amin and pixel; max_iter >= 1; planes and tables aligned
 * to their element sizes.  Min and add commute: the three tables do not depend on the schedule. */
int mc_mandelbrot_atom_domains(const uint32_t* period, const double* amin, uint64_t n_pixels, uint32_t max_iter, uint32_t* count,
                               double* amin_table, uint32_t* pixel);
int mc_mandelbrot_atom_domains_device_async(mc_context* ctx, const void* d_period, const void* d_amin, uint64_t n_pixels, uint32_t max_iter,
                                            void* d_count, void* d_amin_table, void* d_pixel, void* stream);
/* NEWTON IN PERTURBATION SPACE (host only).  mc_mandelbrot_nucleus_refine refines offset = (ox, oy), the position of c relative to the
 * orbit's centre in PERTURB's dc units (c = c_ref + offset), toward a zero of z_p(c), p = period.  IEEE double throughout, one operation
 * at a time in the order written, no contraction.  Per Newton step:
 *    d = 0, m = 0, D = 0;  for k = 0 .. p - 1:
 *      z_k = Z[m] + d, or d when m = 0 (z_0 = 0);  t = z_k + z_k;
 *      D = (((t.x * D.x) - (t.y * D.y)) + 1, (t.x * D.y) + (t.y * D.x))                   (both parts from the old D)
 *      one iteration of PERTURB's loop above with dc = offset, operation for operation, the rebase rule with its m == L case included
 *      (no escape test: the orbit table's last entry stands in for every index past it, as in the kernels);
 *    z_p = Z[m] + d, or d when m = 0;  q = z_p / D by Smith's division (|D|^2 overflows at 1e-150 and below):
 *      |D.x| >= |D.y|:  r = D.y / D.x;  den = D.x + (D.y * r);  q = ((z.x + (z.y * r)) / den, (z.y - (z.x * r)) / den)
 *      otherwise:       r = D.x / D.y;  den = D.y + (D.x * r);  q = (((z.x * r) + z.y) / den, ((z.y * r) - z.x) / den)
 *    offset = offset - q.
 * It stops after the step whose max(|q.x|, |q.y|) <= 2^-52 * max(|ox|, |oy|) (the new offset), or after max_steps, and returns MC_OK
 * either way: *steps is the number of steps taken and last_step the last q, which tell the two apart.  A non-finite D, q or offset is
 * MC_ERR_UNSUPPORTED with the step named in mc_last_error_detail (offset then holds the last finite value).  MC_ERR_INVALID_ARGUMENT: a
 * deep orbit, period = 0, period > the orbit's max_iter, max_steps = 0, a non-finite start, a NULL pointer.
 * A shallow (F32 / F64) view uses an orbit at centre "0", "0" and the pixel's own c as the offset, as mc_mandelbrot_exact_counts does.
 * An offset carries 53 bits: to go deeper, recentre on the text below and refine again from offset 0, about 40 bits per round. */
int mc_mandelbrot_nucleus_refine(const mc_mandelbrot_orbit* o, uint32_t period, uint32_t max_steps,
                                 double offset[2] /* in: start, out: refined */, uint32_t* steps, double last_step[2]);
/* THE CENTRE AS TEXT (host only).  mc_mandelbrot_orbit_offset_text writes c = c_ref + (ox, oy) as two decimals a constructor accepts:
 * c_ref is the fixed-point number the constructor parsed (as for mc_mandelbrot_exact_counts), the sum is EXACT, made on the centre's stored
 * limbs extended at the low end by as many zero limbs as the offset's lowest bit needs (nothing is refused for depth, nothing dropped),
 * and each part is written as [-]digits.digits with frac_digits fractional digits (frac_digits = 0: no point), truncated toward zero; a
 * zero value has no sign.  For a deep orbit (ox, oy) are in units of 2^scale_exp2, the rescaled loop's u: c = c_ref + (ox, oy) *
 * 2^scale_exp2; otherwise they are PERTURB's dc.  Both strings are NUL-terminated and need max(len) + 1 bytes each: a smaller capacity
 * is MC_ERR_INVALID_ARGUMENT with the needed size in mc_last_error_detail, and nothing is written.  MC_ERR_INVALID_ARGUMENT also for a
 * non-finite offset, a NULL pointer, frac_digits above 1 000 000. */
int mc_mandelbrot_orbit_offset_text(const mc_mandelbrot_orbit* o, double ox, double oy, uint32_t frac_digits, char* out_x, char* out_y,
                                    size_t capacity);

/* ---- Buddhabrot: the orbit-density plane of the same iteration (the project's own addition: the reference has no counterpart and no
 *      picture to match; additions within ABI 3; what tests/buddhabrot_ref.py restates).  Every point of every
 *      ESCAPING orbit of pseudo-randomly sampled c adds one to the bin of the plane it lands in: a scatter through atomic integer adds,
 *      where every other render of this library is a gather.  Integer adds commute, so the plane and the statistics do not depend on
 *      which lane takes which sample nor on the order the adds arrive in: every call below is exact to the bit, host and device alike.
 *      Everything is IEEE double in the order written, no contraction, denormals kept, unless stated otherwise.
 *
 *  SAMPLE k (k in [sample_begin, sample_end), a 64-bit index):
 *   - x = (uint32_t)k, y = (uint32_t)(k >> 32), z = seed;
 *   - three rounds of the integer hash of the path tracer's generator (pathTracer.comp:107-110), all three words at once per round:
 *       x' = ((x >> 8) ^ y) * 1103515245,  y' = ((y >> 8) ^ z) * 1103515245,  z' = ((z >> 8) ^ x) * 1103515245   (mod 2^32);
 *   - the INTEGERS are kept: ux = x, uy = y after the rounds (the generator's conversion to float is not used);
 *   - tx = ((double)ux + 0.5) * 2^-32,  cx = sample_centre_x + ((tx - 0.5) * sample_scale_x);  cy likewise from uy with
 *     sample_centre_y and sample_scale_y.
 *  INTERIOR SKIP (part of the contract, not a shortcut): with xm = cx - 0.25, y2 = cy * cy, q = (xm * xm) + y2, xp = cx + 1.0 the
 *     sample is skipped and contributes nothing when (q * (q + xm)) <= (0.25 * y2) [the main cardioid] or ((xp * xp) + y2) <= 0.0625
 *     [the period-2 disc].
 *  CLASSIFY: zx = zy = sx = sy = 0; for i in [0, M), M = max_iter:
 *       nzx = (sx - sy) + cx;  nzy = ((2 * zx) * zy) + cy;  zx = nzx;  zy = nzy;  sx = zx * zx;  sy = zy * zy;
 *       if (sx + sy > 4.0) { n = i; escaped; stop }
 *     The step is MC_PRECISION_F64's, operation for operation.  The radius is 4.0 (|z|^2 > 4), NOT the 2.0 the Mandelbrot renders
 *     inherit from the reference: points with |z|^2 in (2, 4] belong to bounded orbits too, and this picture is the project's own with no
 *     reference image to match.  A sample that never escapes within M steps contributes nothing.
 *  PLOT, only for an escaped sample with n >= min_iter: the same steps again from z = 0, and for each of z_1 .. z_n (the n points that
 *     did not escape; the escaping point z_(n+1) is not plotted):
 *       fx = ((zx - view_centre_x) * kx) + ox,  kx = (double)width / view_scale_x (ONE IEEE division, on the host),  ox = 0.5 * (double)width;
 *       fy = ((zy - view_centre_y) * ky) + oy,  ky = (double)height / view_scale_y,  oy = 0.5 * (double)height;
 *       inside iff fx >= 0 && fx < (double)width && fy >= 0 && fy < (double)height (a NaN is outside);
 *       if inside: plane[(uint32_t)fy * width + (uint32_t)fx] += 1.
 *     The plane is uint32_t[height][width], storage rows as everywhere.  Counts WRAP modulo 2^32; they do not saturate.
 *  The calls ADD to the plane (and to the device statistics) they are given: sample ranges, seeds and devices compose by plain addition,
 *  as the histogram call's tiles do, and a progressive render is a loop of calls.
 *  STATISTICS (all order-independent, so exact): samples = the k in range; skipped = removed by the interior test; contributing =
 *  samples that escaped with min_iter <= n; points = the sum of n over the contributing samples; added = the points inside the view.
 *  VALIDATION: MC_ERR_INVALID_ARGUMENT, mc_last_error_detail naming the field, for NULL pointers; width or height = 0 or
 *  width * height > 2^32 - 1; max_iter = 0 or > 2^24; a scale that is not finite or is zero; a centre that is not finite (negative scales
 *  are allowed: they mirror); sample_end < sample_begin or more than 2^40 samples in one call; unknown flag bits.  min_iter >= max_iter
 *  is valid and adds nothing.
 *  FLAGS: measurement bits only, as bits 0 - 15 of the path tracer's flags are: MC_BUDDHA_KERNEL_PLAIN runs the device call's plain form
 *  (one sample per lane, a grid-stride loop, classify then replay), MC_BUDDHA_KERNEL_POOLED its pooled form (each wave owns a run of
 *  sample indices; a lane that has finished its sample takes the wave's next one; classification and plotting share one loop body).
 *  Neither bit: the shipped choice (DESIGN.md section 3.26 says which and on what measurement); both: MC_ERR_INVALID_ARGUMENT.  The
 *  plane and the statistics are the same bits either way; the host call ignores the two bits.
 *  STATED LIMITS: uint32 counts that wrap; one GPU (ranges compose, so a multi-GPU render is an addition of planes by the caller;
 *  mc_multi_* has no form of it).  The calls of this block sample the window uniformly; a zoomed view, which few c reach, is what the
 *  importance map and the guided calls further down (mc_buddhabrot_importance*, _density_guided*, _render_guided) are for. */
enum { MC_BUDDHA_KERNEL_PLAIN = 1u << 0, MC_BUDDHA_KERNEL_POOLED = 1u << 1 };
typedef struct mc_buddhabrot_params {
    double view_centre_x, view_centre_y, view_scale_x, view_scale_y;         /* the window the density plane covers */
    double sample_centre_x, sample_centre_y, sample_scale_x, sample_scale_y; /* the window c is drawn from */
    uint64_t sample_begin, sample_end;   /* sample indices k in [begin, end) */
    uint32_t width, height;              /* the plane: uint32_t[height][width] */
    uint32_t max_iter, min_iter;         /* M; an orbit contributes iff it escapes after n iterations, min_iter <= n < M */
    uint32_t seed, flags;
} mc_buddhabrot_params;                  /* 104 bytes */
typedef struct mc_buddhabrot_stats {
    uint64_t samples, skipped, contributing, points, added;
} mc_buddhabrot_stats;                   /* 40 bytes: the device form is uint64_t[5] in this order */
/* View centre (-0.5, 0), view scale (3, 3 * height / width), sample window centre (-0.5, 0) and scale (4, 4), max_iter 1000, min_iter 0,
 * seed 1, flags 0, the range [0, samples). */
int mc_buddhabrot_default_params(uint32_t width, uint32_t height, uint64_t samples, mc_buddhabrot_params* out);
/* Host only, usable without a GPU: the same __host__ __device__ body the kernels are built from, in a translation unit without HIP.  ADDS
 * to plane, and to *stats_or_NULL. */
int mc_buddhabrot_density(const mc_buddhabrot_params* p, uint32_t* plane, mc_buddhabrot_stats* stats_or_NULL);
/* ADDS to d_plane (uint32_t[height][width], 4-byte aligned) and to d_stats (uint64_t[5], 8-byte aligned; may be NULL) on the device. */
int mc_buddhabrot_density_device_async(mc_context* ctx, const mc_buddhabrot_params* p, void* d_plane, void* d_stats, void* stream);
/* Blocking: zeroes a device plane of the context, launches, copies the plane (and the statistics) out: out_plane RECEIVES the density
 * of p's range, it is not added to.  mc_context_last_timing spans it. */
int mc_buddhabrot_render(mc_context* ctx, const mc_buddhabrot_params* p, uint32_t* out_plane, mc_buddhabrot_stats* out_stats_or_NULL);
/* Importance map and guided sampling, for views that few c reach (additions within ABI 3; what
 * tests/buddhabrot_guided_ref.py restates).  Everything stays integer adds and a deterministic function of k, so every call below is
 * exact to the bit, independent of the schedule, and composes by addition, as the calls above do.
 *  CELLS: grid_log2 = g in 1 .. 12, G = 2^g.  The sample window is cut into G x G cells by the top g bits of the hash words:
 *       cell = (uy >> (32 - g)) * G + (ux >> (32 - g)),
 *     ux, uy the integers SAMPLE k keeps.  Row-major; the cell rows follow cy (uy), the columns cx (ux).
 *  IMPORTANCE MAP (mc_buddhabrot_importance, host; mc_buddhabrot_importance_device_async): the samples, the statistics and the plane of
 *     mc_buddhabrot_density / _density_device_async for the same p, bit for bit, and in addition a map uint32_t[G * G]: every
 *     contributing sample k whose added_k (its points inside the view) is above 0 does map[cell(k)] += added_k — on the device one
 *     relaxed agent-scope atomic per such sample, at the end of its plot phase.  The map WRAPS modulo 2^32.  The calls ADD to the map, so
 *     ranges and seeds compose by addition; sum(map) == the added the same calls report (mod 2^32), and the map of g is the map of g + 1
 *     summed 2 x 2.  plane / d_plane may be NULL: then no plane add is issued at all and the statistics, added included, are still
 *     exact (a pilot's normal use).  Both kernel forms honour it through the MC_BUDDHA_KERNEL_* bits.
 *  CELL LIST (mc_buddhabrot_importance_cells, host only, deterministic): the cells with map[cell] >= threshold (threshold >= 1), grown by
 *     `dilate` (0 .. 8) rings of the 8-neighbourhood clipped at the grid's edge, in ASCENDING index order.  flags bit 0,
 *     MC_BUDDHA_CELLS_COMPLEMENT: the cells NOT in that set instead (list and complement partition the grid).  *n_cells receives the
 *     count; cells_out may be NULL to query it, else it has room for that many (G * G always suffices).  An empty result is valid.
 *  GUIDED DENSITY (mc_buddhabrot_density_guided, host; mc_buddhabrot_density_guided_device_async): for sample k in [sample_begin,
 *     sample_end):
 *       j = k mod n_cells (k the 64-bit index),  cell = cells[j];
 *       ux, uy = SAMPLE k's hash words, exactly as above;
 *       ux' = ((cell mod G) << (32 - g)) | (ux >> g),   uy' = ((cell / G) << (32 - g)) | (uy >> g)
 *     — the hash's HIGH bits, shifted down, fill the cell — and everything after that is the contract above applied to ux', uy': tx, cx,
 *     INTERIOR SKIP, CLASSIFY, PLOT.  Each plotted point adds `weight` (>= 1) instead of 1, modulo 2^32; the statistics count samples and
 *     points as ever (added counts POINTS, not weight).  A range that is a multiple of n_cells gives every listed cell the same number of
 *     samples; a list may repeat a cell.  A cell index >= G * G is MC_ERR_INVALID_ARGUMENT: the host call checks its list; the async
 *     device form takes a DEVICE list (4-byte aligned, caller-owned, alive until the launch has run) and cannot, so there it is the
 *     caller's precondition — its kernels clamp the index to G * G - 1, so that a broken list gives wrong samples, never a wild access.
 *     WEIGHT makes an unbiased picture a sum of two calls: the list at N samples per cell and weight 1, plus its complement at N / B
 *     samples per cell and weight B, have in their sum the expectation of the uniform density of N * G * G samples (every cell's orbits
 *     at the same expected weight per unit of sample area; the complement's at B times the variance).  The list ALONE is biased by
 *     whatever the pilot missed: orbits from cells outside the list are absent from it (DESIGN.md section 3.27 has measured shares).
 *  THE CHAIN (mc_buddhabrot_render_guided, blocking): (1) zero a map of the context; (2) the pilot: the uniform samples
 *     [0, pilot_samples) of p->seed with p's view, window, M, min_iter and flags, no plane; (3) copy the map out; (4) the list by
 *     mc_buddhabrot_importance_cells(g, map, threshold, dilate, 0), uploaded; (5) the guided render of p's range over it at weight 1 into
 *     a zeroed plane; (6) if complement_weight B > 0 and the complement is not empty: a second guided call over the complement list,
 *     range [sample_end, sample_end + ceil(samples * n_complement / (n_cells * B))), samples = sample_end - sample_begin, at weight B,
 *     into the same plane.  out_plane receives the plane, out_stats the statistics of step 5 alone; out_info the two counts, the pilot's
 *     statistics and the complement pass's (zeros when it did not run).  An EMPTY list is MC_OK with a zero plane, zero statistics and
 *     n_cells = 0.  mc_context_last_timing spans the chain.
 *  VALIDATION beyond p's: grid_log2 outside 1 .. 12; NULL map, cells, n_cells, guide; threshold = 0; dilate > 8; unknown flags;
 *     n_cells = 0; weight = 0; pilot_samples > 2^40; a complement range above 2^40 samples or past 2^64. */
enum { MC_BUDDHA_CELLS_COMPLEMENT = 1u << 0 };
typedef struct mc_buddhabrot_guide_params {
    uint32_t grid_log2, dilate;          /* g; rings of dilation */
    uint64_t pilot_samples;              /* the pilot's range is [0, pilot_samples) */
    uint32_t threshold;                  /* a cell is listed when its map word is at least this */
    uint32_t complement_weight;          /* B; 0: no complement pass */
} mc_buddhabrot_guide_params;            /* 24 bytes */
typedef struct mc_buddhabrot_guide_info {
    uint32_t n_cells, n_complement;
    mc_buddhabrot_stats pilot, complement;
} mc_buddhabrot_guide_info;              /* 88 bytes */
/* ADDS to map (uint32_t[G * G]), to plane_or_NULL and to *stats_or_NULL.  Host only, usable without a GPU. */
int mc_buddhabrot_importance(const mc_buddhabrot_params* p, uint32_t grid_log2, uint32_t* map, uint32_t* plane_or_NULL,
                             mc_buddhabrot_stats* stats_or_NULL);
/* ADDS to d_map (4-byte aligned), to d_plane (may be NULL) and to d_stats (uint64_t[5], 8-byte aligned; may be NULL) on the device. */
int mc_buddhabrot_importance_device_async(mc_context* ctx, const mc_buddhabrot_params* p, uint32_t grid_log2, void* d_map, void* d_plane,
                                          void* d_stats, void* stream);
int mc_buddhabrot_importance_cells(uint32_t grid_log2, const uint32_t* map, uint32_t threshold, uint32_t dilate, uint32_t flags,
                                   uint32_t* cells_out_or_NULL, uint32_t* n_cells);
/* ADDS to plane and to *stats_or_NULL.  Host only, usable without a GPU. */
int mc_buddhabrot_density_guided(const mc_buddhabrot_params* p, const uint32_t* cells, uint32_t n_cells, uint32_t grid_log2,
                                 uint32_t weight, uint32_t* plane, mc_buddhabrot_stats* stats_or_NULL);
/* d_cells: a DEVICE list of n_cells words.  ADDS to d_plane and to d_stats (may be NULL) on the device. */
int mc_buddhabrot_density_guided_device_async(mc_context* ctx, const mc_buddhabrot_params* p, const void* d_cells, uint32_t n_cells,
                                              uint32_t grid_log2, uint32_t weight, void* d_plane, void* d_stats, void* stream);
/* g = 8, pilot_samples = 2^24, threshold 1, dilate 1, complement_weight 0. */
int mc_buddhabrot_guide_default_params(mc_buddhabrot_guide_params* out);
int mc_buddhabrot_render_guided(mc_context* ctx, const mc_buddhabrot_params* p, const mc_buddhabrot_guide_params* guide,
                                uint32_t* out_plane, mc_buddhabrot_stats* out_stats_or_NULL, mc_buddhabrot_guide_info* out_info_or_NULL);
/* Tone mapping, deliberately small: a density d becomes map[min(d, L)] / L through a table of L + 1 entries, L = levels in 1 .. 2^20.
 *  - mc_buddhabrot_sqrt_map (host only): map[j] = (uint32_t)((double)L * sqrt((double)j / (double)L)), clamped to L.
 *  - mc_buddhabrot_tonemap (host) and mc_buddhabrot_tonemap_device_async: per pixel and channel c the output is
 *    (float)m_c[min(d_c, L)] / (float)L — exact conversions and one IEEE fp32 division — and alpha is 1.  The three planes may be the
 *    same pointer (grey: one plane three times) or three renders of different max_iter (the "Nebulabrot"); a map entry above L is
 *    MC_ERR_INVALID_ARGUMENT.  The device form takes three DEVICE planes and three HOST maps; the quotients are formed on the host and
 *    kept as a device table of the context, the way mc_mandelbrot_recolour_device_async keeps its table.
 *  - the rank map needs no new call: a density plane is a count plane, so mc_mandelbrot_histogram_device_async(ctx, d_plane, 4,
 *    width * height, L, d_hist) (densities above L count in bin L) followed by mc_mandelbrot_equalise_map(L, hist, map) yields a valid
 *    map (map[L] = L; lower densities by their rank among the bins below L). */
int mc_buddhabrot_sqrt_map(uint32_t levels, uint32_t* map /* levels + 1 */);
int mc_buddhabrot_tonemap(uint32_t width, uint32_t height, const uint32_t* d0, const uint32_t* d1, const uint32_t* d2, uint32_t levels,
                          const uint32_t* m0, const uint32_t* m1, const uint32_t* m2, float* out_rgba_f32);
int mc_buddhabrot_tonemap_device_async(mc_context* ctx, uint32_t width, uint32_t height, const void* d0, const void* d1, const void* d2,
                                       uint32_t levels, const uint32_t* m0 /* HOST, levels + 1 */, const uint32_t* m1, const uint32_t* m2,
                                       void* d_rgba_f32, void* stream);

/* ---- Path tracer: replaces shaders/pathTracer.comp:343-458 and the spp-dispatch loop of
 *      PathtracerApp::createCommandBuffer (src/pathtracerApp.h:358-378), fused into one launch ------ */
enum {
    MC_PT_MATH_STRICT = 0, /* IEEE div/sqrt + the explicit "mc math" sin/cos/pow: bit-identical to the oracle */
    MC_PT_MATH_FAST = 1,   /* toleranced parity (RMSE <= 0.5, 99.9-percentile per-pixel L2 <= 4 of 255 at 500 spp).  */
                           /* The library renders the request with the tier MEASURED to hold that bound on scenes like the one given: */
                           /* the fast tier (gfx950 hardware rcp/rsq/sqrt/sin/cos/exp/log, a*b+c contracted) for a scene with no more  */
                           /* specular surface than the reference scene's (mc_pathtrace_scene_class: up to three spheres, diffuse     */
                           /* walls, mirror / glass spheres no larger) — the reference scene reads 2.49, 174 random scenes of that     */
                           /* class at most 3.8 but for two at 4.2: met where it was stated, measured and not guaranteed around it;     */
                           /* the careful tier below everywhere else (at most 1.8 on every scene measured); the strict kernels for a  */
                           /* light all but enclosed by an opaque sphere.  mc_pathtrace_select_kernel reports which                     */
                           /* (mc_pathtrace_kernel_info.math_mode).  A caller that needs the margin on EVERY scene asks for the tier below. */
    MC_PT_MATH_FAST_CAREFUL = 2 /* the fast mode's careful tier on request: the same kernels and shortcuts, division / sqrt / 1/sqrt */
                           /* rounded as the reference rounds them and no contraction — a sample differs from the reference's by far  */
                           /* fewer roundings and takes another path correspondingly less often; 1.14 - 1.43 x the fast tier's time  */
};

/* mc_pathtrace_params.flags: MC_PT_PRECISION(x) below (bits 16-19) is the one field a binding sets.  Bits 0-15 belong to this
 * repository's measurement tools (kernel-selection A/B switches, include/mc_compute_test.h: not part of the boundary — a binding
 * leaves them zero, and then every request is rendered by the kernel the host selects, inside the mode's parity contract);
 * every other bit is reserved and refused with MC_ERR_INVALID_ARGUMENT. */
/* Sphere-test precision branch of pathTracer.comp:132-256.  The reference compiles every variant OUT
 * (emulateDouble.h.glsl:13-26 are all FALSE) and enables one by hand together with the
 * TEST_PRECISION_WITH_LARGE_SPHERE_WALLS scene (pathtracerApp.h:11,28-35).  This DOES change results. */
enum {
    MC_PT_PREC_F32 = 0,  /* the default build: fp32 test only (pathTracer.comp:316-331)              */
    MC_PT_PREC_FP64 = 1, /* USE_NATIVE_FP64 (pathTracer.comp:132-143)                                 */
    MC_PT_PREC_DS = 2,   /* DS_f32_f32 (pathTracer.comp:144-213, emulateDouble.h.glsl:28-223)          */
    MC_PT_PREC_DF64 = 3  /* DF64_F32_F32 (pathTracer.comp:214-256, emulateDouble.h.glsl:225-356)       */
};
#define MC_PT_PRECISION(x) ((uint32_t)(x) << 16)

typedef struct mc_pathtrace_params {
    uint32_t width, height;            /* push constant imgdim (pathtracerApp.h:44-47,58-59)            */
    uint32_t spp;                      /* push constant samps.y (pathtracerApp.h:61; main.cpp:22)        */
    uint32_t sample_begin, sample_end; /* samps.x range rendered by this call; 0,spp = whole render.     */
                                       /* sample_begin>0 continues the accumulator already in the buffer */
    uint32_t max_depth;                /* maxDepth, 12 (pathTracer.comp:367)                             */
    uint32_t row_begin, row_end;       /* storage rows; 0,height for the whole image                    */
    uint32_t row_block, row_stride;    /* interleaved row blocks, as in mc_mandelbrot_params             */
    uint32_t math_mode;                /* MC_PT_MATH_*                                                   */
    uint32_t flags;
} mc_pathtrace_params;

int mc_pathtrace_default_params(uint32_t width, uint32_t height, uint32_t spp, mc_pathtrace_params* p);

/* The reference's default scene tables (pathtracerApp.h:14-39): 12 floats per object
 * (plane: equation.xyzw | emission.xyz0 | colour.rgb,material; sphere: centre.xyz,radius | ... ). */
int mc_pathtrace_default_scene(const float** planes, uint32_t* n_planes, const float** spheres, uint32_t* n_spheres);

/* Host-buffer form: planes/spheres are the host tables PathtracerApp::preRun memcpy's into its SSBOs
 * (pathtracerApp.h:152-161,189-198); out_rgba_f32 receives (row_end-row_begin)*width*4 floats. */
int mc_pathtrace_render(mc_context* ctx, const mc_pathtrace_params* p, const float* planes, uint32_t n_planes,
                        const float* spheres, uint32_t n_spheres, float* out_rgba_f32);

/* Device-buffer form: d_rgba_f32 is a device pointer to the tile; scene tables are still host
 * pointers (432 B, passed as kernel constants).  Asynchronous on `stream` (NULL = context stream). */
int mc_pathtrace_render_device_async(mc_context* ctx, const mc_pathtrace_params* p, const float* planes,
                                     uint32_t n_planes, const float* spheres, uint32_t n_spheres, void* d_rgba_f32,
                                     void* stream);

/* ---- Host post-process on the GPU: replaces the scalar loops of
 *      getRenderedImage (mandelbrotApp.h:149-170, pathtracerApp.h:202-223) and the 180-degree
 *      rotation (pathtracerApp.h:236-243).  u8 = (uint8_t)(scale*c) with the x86-64 semantics the
 *      reference binary has (cvttss2si, low byte), alpha = 255.  rotate180 != 0 applies the PT swap. */
int mc_convert_rgba8_device_async(mc_context* ctx, const void* d_rgba_f32, uint32_t width, uint32_t height,
                                  float scale, int rotate180, void* d_rgba8, void* stream);
int mc_convert_rgba8(mc_context* ctx, const float* rgba_f32, uint32_t width, uint32_t height, float scale,
                     int rotate180, uint8_t* rgba8);
/* Render + post-process fused on the device: the whole image is rendered, converted exactly as the reference's
 * saveRenderedImage would (Mandelbrot: scale 255, mandelbrotApp.h:159-174; path tracer: scale 1 and the
 * 180-degree rotation, pathtracerApp.h:202-243) and only the RGBA8 image (4 B/pixel instead of 16) is copied to
 * out_rgba8 (width*height*4 bytes, host).  The path tracer: whole image only (row_begin = 0, row_end = height, no interleave).
 * The Mandelbrot set, which is not rotated: also a contiguous band of rows [row_begin, row_end) (no interleave) — out_rgba8 then receives
 * (row_end-row_begin)*width*4 bytes, the band's rows of the whole image's RGBA8 (the app renders band by band while its PNG workers run). */
int mc_mandelbrot_render_rgba8(mc_context* ctx, const mc_mandelbrot_params* p, uint8_t* out_rgba8);
/* The same image (rows [row_begin, row_end), no interleave) rendered in bands of band_rows rows, PIPELINED: band k + 1 is launched on a second
 * stream before band k has finished — it fills the device while band k's last tiles drain and while band k's rows travel to the host — and
 * on_rows(rows_done, user) is called on the calling thread as each band has ARRIVED, in order (rows [row_begin, rows_done) of the output are
 * final): the caller's own work on the image — the app's PNG workers — runs beside the rest of the render.  Exactly one of out_rgba_f32
 * (the storage buffer, 16 B/pixel) and out_rgba8 (converted on the device, 4 B/pixel) is non-NULL; on_rows may be NULL.  Blocking; the
 * bytes are those of mc_mandelbrot_render / mc_mandelbrot_render_rgba8.  mc_context_last_timing then reports kernel = first launch to the end
 * of the last kernel, copy = what of the copies was not hidden behind a kernel.  mc_context_warmup_mandelbrot(ctx, p, rgba8 | 2) prepares it. */
typedef void (*mc_rows_ready_fn)(uint32_t rows_done, void* user);
int mc_mandelbrot_render_banded(mc_context* ctx, const mc_mandelbrot_params* p, float* out_rgba_f32, uint8_t* out_rgba8, uint32_t band_rows,
                                mc_rows_ready_fn on_rows, void* user);
int mc_pathtrace_render_rgba8(mc_context* ctx, const mc_pathtrace_params* p, const float* planes, uint32_t n_planes,
                              const float* spheres, uint32_t n_spheres, uint8_t* out_rgba8);

/* ---- Path-tracer denoiser (no reference counterpart; additions within ABI 3) ------------------------------
 * An edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch 2010) over a vec4 plane, steered by two guide planes that hold
 * what the CENTRE ray of each pixel hits.  Everything here is strict arithmetic whatever the render's math_mode: every operation one
 * IEEE-754 fp32 operation in the order stated (no contraction, correctly rounded divide and square root), so that the host calls, the
 * device kernels and tests/pt_denoise_ref.py agree bit for bit.  csrc/pt_denoise.h is the one source of both.
 *
 * THE GUIDES.  Per pixel (gx, gy) of a width x height image the camera ray of pathTracer.comp:352-362 with the sub-sample bracket
 * (0.5 + vec2((samps.x/2)%2, samps.x%2) + tent) replaced by the constant 1.0:
 *     sx = (((float)gx + 0.5f) / (float)width - 0.5f) * 0.036f;   sy = (((float)gy + 0.5f) / (float)height - 0.5f) * 0.024f;
 *     spos = (cam.o + cx * sx) + cy * sy;   d = normalize(lc - spos);   ray (lc, d),
 *   cam.o, cx, cy, lc as the shader forms them (:352-353, :360), dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z, normalize(a) = a * (1 / sqrt(dot(a, a))).
 *   intersect() of pathTracer.comp:112-131, 316-341 with the fp32 sphere test, planes then spheres in table order: the hit id and t are the
 *   ones the strict path tracer finds for that ray.  x = lc + d * t;  n = the plane's equation.xyz, or normalize(x - centre) of a sphere;
 *   nl = dot(n, d) < 0 ? n : -n (:390).
 *     normal_t    = (nl.x, nl.y, nl.z, t)
 *     position_id = (x.x, x.y, x.z, (float)id)      id: planes 0 .. n_planes-1, spheres n_planes + i
 *   a miss writes (0, 0, 0, 1e20) and (0, 0, 0, -1).  Both planes are in STORAGE order, element (height - 1 - gy) * width + gx (:349), so
 *   they line up with the render's buffer.  Any scene of up to 2^20 objects; either table may be empty.
 *
 * THE FILTER.  P = passes passes over W x H planes in storage coordinates, pass i = 0 .. P-1 with step s = 2^i reading the previous pass's
 * plane (pass 0: rgba).  kc_i = (float)4^i / (sigma_colour * sigma_colour): the colour tolerance halves every pass.  For pixel p = (x, y):
 *   - id_p = position_id[p].w < 0: out[p] = in[p], all four components.
 *   - otherwise sw = sr = sg = sb = 0, and for the 25 taps in row-major order (b = -2 .. 2 outer, a = -2 .. 2 inner), q = (x + s*a, y + s*b):
 *       skip q outside the image; skip q with id_q != id_p;
 *       dc2 = (dr*dr + dg*dg) + db*db over in[q].rgb - in[p].rgb;  dn2 likewise over the normals;  dx2 likewise over the positions;
 *       e = (dc2 * kc_i + dn2 * k_normal) + dx2 * k_position;   w = (h[b] * h[a]) * exp2(-e),  h = {1/16, 1/4, 3/8, 1/4, 1/16};
 *       sw = sw + w;  sr = sr + w * in[q].r;  sg and sb likewise;
 *     out[p].rgb = (sr / sw, sg / sw, sb / sw);  out[p].w = in[p].w.  The centre tap has e = 0, so sw >= 9/64.
 *   exp2 is the library's strict exp2 (the one behind the strict path tracer's pow): 0 below -125, else n = rint(y), f = y - n, a degree-6
 *   polynomial in f by fma, times 2^n.
 * sigma_colour is in units of the plane being filtered: the default, 128, suits the final buffer of a render (0 .. 255.5, gamma-encoded);
 * a caller that filters a partial linear accumulator passes its own.
 *
 * mc_pathtrace_denoise_default_params: passes = 5, sigma_colour = 128, k_normal = 8, k_position = 4, flags = 0.
 * mc_pathtrace_guides, mc_pathtrace_denoise: host only, no device, usable without a GPU, the same source as the kernels.  out may be rgba.
 * mc_pathtrace_guides_device_async, mc_pathtrace_denoise_device_async: on device pointers (16-byte aligned vec4 planes), asynchronous on
 *   `stream` (NULL: the context's); the scene tables are host pointers, copied to the device before the call returns.  Their scratch (the
 *   scene records; two planes between the passes) is the context's, shared with the blocking calls: calls on one context follow one
 *   another on one stream, as everywhere.  d_out may equal d_rgba; otherwise every input is left as it was, and an output that overlaps
 *   an input in any other way is refused.
 * mc_pathtrace_render_denoised (blocking): the render of p (any math_mode), the guides, the filter, and for out_rgba8 the conversion and
 *   rotation of mc_pathtrace_render_rgba8 - that is, exactly the chain of the separate calls.  Exactly one of out_rgba_f32 (width*height*4
 *   floats) and out_rgba8 (width*height*4 bytes) is non-NULL.  Whole images and whole renders only: row_begin = 0, row_end = height, no
 *   interleave, sample_begin = 0, sample_end = spp (the filter runs on the final, encoded buffer: the last sample encodes in place, :453);
 *   d->width and d->height equal p's.  mc_context_last_timing covers all of it; mc_context_warmup_pathtrace prepares its render as ever.
 * Refused with MC_ERR_INVALID_ARGUMENT and a detail string: a NULL pointer, a zero size, passes outside 1 .. 8, a sigma_colour that is not
 *   finite and above 0 (or whose fp32 square is not), a negative or non-finite k_normal or k_position, flags other than 0, a row tile or a
 *   sample range in mc_pathtrace_render_denoised.  More than 2^20 objects: MC_ERR_UNSUPPORTED.
 * STATED LIMITS: a mirror or glass first hit is guided by the sphere's own surface, so what is seen in it or through it is protected by
 *   the colour weight alone.  mc_multi_* has no denoised form: gather the image, then filter it on one device. */
typedef struct mc_pathtrace_denoise_params {
    uint32_t width, height;
    uint32_t passes;        /* 1..8 */
    float sigma_colour;     /* > 0 */
    float k_normal;         /* >= 0 */
    float k_position;       /* >= 0 */
    uint32_t flags;         /* 0 */
} mc_pathtrace_denoise_params;
int mc_pathtrace_denoise_default_params(uint32_t width, uint32_t height, mc_pathtrace_denoise_params* d);
int mc_pathtrace_guides(uint32_t width, uint32_t height, const float* planes, uint32_t n_planes, const float* spheres, uint32_t n_spheres,
                        float* out_normal_t, float* out_position_id);
int mc_pathtrace_guides_device_async(mc_context* ctx, uint32_t width, uint32_t height, const float* planes, uint32_t n_planes,
                                     const float* spheres, uint32_t n_spheres, void* d_normal_t, void* d_position_id, void* stream);
int mc_pathtrace_denoise(const mc_pathtrace_denoise_params* d, const float* rgba, const float* normal_t, const float* position_id, float* out);
int mc_pathtrace_denoise_device_async(mc_context* ctx, const mc_pathtrace_denoise_params* d, const void* d_rgba, const void* d_normal_t,
                                      const void* d_position_id, void* d_out, void* stream);
int mc_pathtrace_render_denoised(mc_context* ctx, const mc_pathtrace_params* p, const mc_pathtrace_denoise_params* d, const float* planes,
                                 uint32_t n_planes, const float* spheres, uint32_t n_spheres, float* out_rgba_f32, uint8_t* out_rgba8);

/* ---- Path-tracer denoiser, colour tolerance from a measured noise plane (no reference counterpart; additions within ABI 3; DESIGN.md
 *      section 3.19) ---------------------------------------------------------------------------------------------------------------
 * The filter above uses one colour tolerance, sigma_colour, whatever noise the render still has: right for 16 spp, too wide for a cleaner
 * render, which it goes on blurring.  The calls below take the tolerance per pixel from a MEASUREMENT of the noise.  Sample ranges compose
 * bit for bit, so a render made as [0, h), a copy of the accumulator, then [h, spp) is the plain render plus the linear accumulator of its
 * first h samples; the first part, encoded as if it were the whole, differs from the finished buffer by the noise that is left.
 * Strict arithmetic whatever the render's math_mode, as above: one IEEE-754 fp32 operation per operation stated, in that order, no
 * contraction, correctly rounded divide; host calls, device kernels and tests/pt_noise_ref.py agree bit for bit (one source: csrc/pt_noise.h).
 *
 * THE NOISE PLANE.  half: a vec4 plane in storage order, the linear accumulator a render leaves after sample_end = h < spp.  full: the
 * finished, encoded buffer of the same render.  scale = (float)spp / (float)h, formed by the caller (exactly 2 for an even spp).  For each
 * pixel q and c in r, g, b:
 *     x = half[q].c * scale;   cl = min(max(x, 0), 1)   with max(x, 0) = x < 0 ? 0 : x and min(y, 1) = 1 < y ? 1 : y (GLSL's);
 *     E = pow045(cl) * 255 + 0.5   (pathTracer.comp:453 as the strict kernels perform it: pow045(c) = exp2(0.45f * log2(c)), log2 and exp2
 *                                   the library's strict ones; exp2 is the filter's);
 *     e_c = E - full[q].c;         v_q = (e_r*e_r + e_g*e_g) + e_b*e_b.
 *   V_p is the mean of v over the (2 radius + 1)^2 window around p = (x, y): sum = cnt = 0; taps q = (x + a, y + b) in row-major order
 *   (b = -radius .. radius outer, a likewise inner), taps outside the image skipped: sum = sum + v_q, cnt = cnt + 1.0f; V_p = sum / cnt.
 *   The window ignores the guide ids: noise is a property of the lighting, not of the surface.  radius is 0 .. 4.  out_variance: one float
 *   per pixel, storage order, in units of the encoded buffer squared.  The planes are not checked for finiteness: finite planes give a
 *   finite V >= 0 (or +inf where a sum overflows).
 *
 * THE NOISE-GUIDED FILTER.  Exactly THE FILTER above with one change: the per-pass constant kc_i = 4^i / sigma_colour^2 becomes the per-pixel
 *     kc_i(p) = (float)4^i / ((k_noise * k_noise) * V_p + 1.0f)
 *   taken at the CENTRE pixel p and used for all of p's taps.  The + 1 is one encoded unit squared: a noiseless pixel (the visible light)
 *   gets a tolerance of one unit, not a division by zero.  Taps, ids, the other two terms of e, exp2, the sums, the divisions, miss pixels
 *   copied, d_out == d_rgba: all as above.  d->sigma_colour must still be valid (it is checked as above) but is NOT USED.
 *
 * mc_pathtrace_noise_default_params: k_noise = 4, radius = 3 (DESIGN.md section 3.19 has the sweep they come from).
 * mc_pathtrace_noise, mc_pathtrace_denoise_adaptive: host only, no device, usable without a GPU, the same source as the kernels.
 * mc_pathtrace_noise_device_async, mc_pathtrace_denoise_adaptive_device_async: on device pointers (vec4 planes aligned to 16 bytes, the
 *   variance plane to 4), asynchronous on `stream` (NULL: the context's); their scratch (one float plane; two vec4 planes between the
 *   passes) is the context's, shared with every other call as the filter's is.  An output that overlaps an input is refused, d_out ==
 *   d_rgba excepted.
 * mc_pathtrace_render_denoised_adaptive (blocking), on the context's stream in this order: the guides; the render of [0, h), h = spp / 2
 *   rounded down; a device copy of that plane; the render of [h, spp) continuing it; the noise plane with scale = (float)spp / (float)h;
 *   the noise-guided filter in place; for out_rgba8 the conversion and rotation of mc_pathtrace_render_rgba8.  Outputs and d as in
 *   mc_pathtrace_render_denoised.  In MC_PT_MATH_STRICT the plane the filter receives is mc_pathtrace_render's bit for bit (ranges
 *   compose), so the result is the host filter applied to that render, the host noise plane of its [0, h) part and the host guides.  In
 *   the fast modes the promise is the weaker one: the result is that of the same chain made from the separate public calls
 *   (mc_pathtrace_render_device_async twice, a copy, the two calls above).  It is not tied to the one-call render because a fast-math
 *   kernel is chosen per request, and two ranges need not be rendered by the kernel the whole would get, nor round like it (see
 *   mc_pathtrace_select_kernel).  mc_context_last_timing covers all of it.
 * Refused with MC_ERR_INVALID_ARGUMENT and a detail string: a NULL pointer, a zero size, radius above 4, a k_noise that is not finite and
 *   above 0 or whose fp32 square is not finite, everything the filter above refuses (passes outside 1 .. 8, flags other than 0, ...), and in
 *   mc_pathtrace_render_denoised_adaptive spp < 2, a row tile, an interleave, a sample range. */
int mc_pathtrace_noise_default_params(float* k_noise, uint32_t* radius);
int mc_pathtrace_noise(uint32_t width, uint32_t height, const float* half, float scale, const float* full, uint32_t radius, float* out_variance);
int mc_pathtrace_noise_device_async(mc_context* ctx, uint32_t width, uint32_t height, const void* d_half, float scale, const void* d_full,
                                    uint32_t radius, void* d_variance, void* stream);
int mc_pathtrace_denoise_adaptive(const mc_pathtrace_denoise_params* d, float k_noise, const float* rgba, const float* normal_t,
                                  const float* position_id, const float* variance, float* out);
int mc_pathtrace_denoise_adaptive_device_async(mc_context* ctx, const mc_pathtrace_denoise_params* d, float k_noise, const void* d_rgba,
                                               const void* d_normal_t, const void* d_position_id, const void* d_variance, void* d_out,
                                               void* stream);
int mc_pathtrace_render_denoised_adaptive(mc_context* ctx, const mc_pathtrace_params* p, const mc_pathtrace_denoise_params* d, float k_noise,
                                          uint32_t radius, const float* planes, uint32_t n_planes, const float* spheres, uint32_t n_spheres,
                                          float* out_rgba_f32, uint8_t* out_rgba8);

/* ---- Path tracer, per-pixel sample budgets from the measured noise plane (no reference counterpart; additions within ABI 3; DESIGN.md
 *      section 3.20) ---------------------------------------------------------------------------------------------------------------
 * Every render above gives every pixel the same spp.  The calls below spend samples where the noise plane says the noise is: a pilot of
 * n0 samples per pixel, one noise plane, a LEVEL l per pixel, then l doublings for the pixels that need them, so that a pixel of level l
 * ends with n0 << l samples.  Three facts make the result exact (checked in the CPU oracle, tests/test_pt_budget_host.py):
 *   1. A sample does not depend on spp but for the divisor (pathTracer.comp:357,393,452), and dividing by 2 n instead of n is an exact
 *      scaling by 1/2 that IEEE addition commutes with.  So the plane a render with spp = 2 n0 leaves after samples [0, n0) is exactly half
 *      the plain spp = n0 linear accumulator, encode_strict(2 * plane) is the finished plain n0 render, and its [0, n0 / 2) part gives the
 *      plain render's noise plane, bit for bit.
 *   2. A doubling continues exactly: the accumulator at divisor 2 n after samples [0, n), plus samples [n, 2 n) at divisor 2 n, is the plain
 *      spp = 2 n accumulator; times 0.5 it is the start of the next doubling.
 *   3. The noise plane's V compares half of the samples with all of them: the variance of the n0-sample estimate, halving per doubling.
 * THE ONE CONDITION: no accumulator component may be a non-zero value below 2^(-126 + max_level + 1) in magnitude, so that every halving
 *   stays exact (nothing becomes subnormal).  The reference scene's smallest non-zero component is of the order of 1e-2.
 * Strict arithmetic whatever the render's math_mode: one IEEE-754 fp32 operation per operation stated, in that order, no contraction; host
 * calls, device kernels and tests/pt_budget_ref.py agree bit for bit (one source: csrc/pt_budget.h).
 *
 * LEVELS.  tau2 = target * target in fp32.  Per pixel, from its V_p (mc_pathtrace_noise's plane):
 *     t = V_p;  l = 0;  while (l < max_level && t > tau2) { t = t * 0.5f;  l = l + 1; }
 *   One uint8_t per pixel, storage order.  NaN gives 0 (no comparison holds), +inf gives max_level.  The pixel's budget is n0 << l.
 *   max_level is 0 .. 8; target must be finite and above 0 with a finite fp32 square.  target is in units of the encoded buffer, as
 *   sqrt(V) is: the noise a pixel may keep.
 * LISTS.  A uint32_t list of the W * H storage indices bucketed by level, HIGHEST LEVEL FIRST, and the count of every level 0 .. max_level
 *   in counts[0 .. max_level] (counts: room for 9).  The pixels of level >= r are then the prefix [0, C_r), C_r = counts[r] + ... +
 *   counts[max_level].  The order inside a bucket is unspecified.  A level byte above max_level counts as max_level.
 * LIST RENDER (the hot kernel).  mc_pathtrace_render_list_device_async: for every entry idx of d_list[0 .. n_list), with row = idx / width,
 *   gx = idx % width, gy = height - 1 - row:  acc = d_acc[idx] * prescale, all four components (sample_begin == 0: acc = 0 and the plane
 *   is not read); then samples [sample_begin, sample_end) are added in sample order as accrad / spp, exactly as the plain render folds
 *   them (pathTracer.comp:451-452); d_acc[idx] = acc.  NEVER the final encode (:453), even when sample_end == spp: the plane stays
 *   linear.  Pixels that are not listed are not touched.  Entries must be distinct; an entry >= width * height is skipped, so a bad list
 *   cannot reach memory outside the plane.  An S-lane group (S = 1, 4, 16) takes one entry.  The kernels are the round-synchronous
 *   families (slab for six axis-aligned planes + 1 .. 8 spheres, generic with the records in LDS or in memory otherwise) in the tier
 *   mc_pathtrace_select_kernel reports for the request; S is MC_PT_FORCE_S's if given, else the plain render's rule applied to n_list
 *   entries.  In MC_PT_MATH_STRICT every sample is the oracle's, so the result does not depend on S or the family.  Whole-image addressing
 *   only (a row tile or an interleave: MC_ERR_INVALID_ARGUMENT); MC_PT_PRECISION variants and more than 2^31 pixels are refused;
 *   n_list == 0 launches nothing and returns MC_OK.  d_acc aligned to 16 bytes, d_list to 4.
 * RESOLVE.  out[p].rgb = encode_strict(acc[p].rgb * (level[p] == 0 ? 2.0f : 1.0f)), out[p].w = acc[p].w; encode_strict is the noise plane's
 *   E (above) of one component.  A pixel of level 0 still holds the pilot's plane, half its n0 accumulator (fact 1).  out may be acc.
 * THE CHAIN.  mc_pathtrace_render_budgeted (blocking), p->spp = n0, on the context's stream in this order: the render of [0, n0 / 2) with
 *   the spp field set to 2 n0; a device copy of that plane; the render of [n0 / 2, n0) continuing it (plane A); a scratch plane
 *   encode_strict(2 A); the noise plane of the two with scale = (float)(2 n0) / (float)(n0 / 2) and radius b->radius; levels; lists; a
 *   read-back of the counts; for r = 1 .. max_level with C_r > 0 a list render over the prefix C_r with spp = n0 << r, samples
 *   [n0 << (r - 1), n0 << r) and prescale 1 for r = 1, 0.5 after (a round with C_r = 0 launches nothing); the resolve in place; for
 *   out_rgba8 the conversion and rotation of mc_pathtrace_render_rgba8.  Exactly one of out_rgba_f32 and out_rgba8; out_levels (one byte
 *   per pixel, storage order) may be NULL.  mc_context_last_timing covers all of it, the read-back included; mc_context_last_budget
 *   reports the pixels per level and the mean samples per pixel of the last call.
 *   THE PROMISE.  In MC_PT_MATH_STRICT out[p] is mc_pathtrace_render at spp = n0 << level[p], bit for bit, and level is
 *   mc_pathtrace_budget_levels of mc_pathtrace_noise of the plain n0 render.  No pilot sample is thrown away.  In the fast modes the
 *   promise is the weaker one of the noise-guided filter: the bits of the same chain made from the separate public calls; the encode is
 *   the strict one in every mode.  Levels come from the same samples they extend, the usual bias of adaptive sampling.
 *   Refused with MC_ERR_INVALID_ARGUMENT and a detail string: n0 odd or below 2, n0 << max_level above 2^20, max_level above 8, a row
 *   tile, an interleave, a sample range, radius above 4, a bad target, flags other than 0, NULL pointers, both or neither image output.
 *   Not offered: mc_multi_*, budgets other than n0 times a power of two.  (mc_pathtrace_accel scenes: mc_pathtrace_render_accel_budgeted.)
 * mc_pathtrace_budget_default_params: max_level = 4, target = 32, radius = 3 (mc_pathtrace_noise_default_params'), flags = 0.
 * mc_pathtrace_budget_levels, mc_pathtrace_budget_resolve: host only, usable without a GPU, the same source as the kernels.
 * The _device_async forms of levels, lists and resolve: on device pointers (vec4 planes aligned to 16 bytes, float and uint32_t planes
 *   to 4), asynchronous on `stream` (NULL: the context's); the lists' cursors are scratch of the context, shared with every other call.
 *   An output that overlaps an input is refused, d_out == d_acc of the resolve excepted. */
typedef struct mc_pathtrace_budget_params {
    uint32_t max_level;   /* 0 .. 8: a pixel gets at most spp << max_level samples                          */
    float target;         /* the noise a pixel may keep, in units of the encoded buffer (compare sqrt(V_p)) */
    uint32_t radius;      /* of the noise plane's window, 0 .. 4                                            */
    uint32_t flags;       /* 0                                                                              */
} mc_pathtrace_budget_params;
int mc_pathtrace_budget_default_params(mc_pathtrace_budget_params* b);
int mc_pathtrace_budget_levels(uint32_t width, uint32_t height, const float* variance, float target, uint32_t max_level, uint8_t* out_levels);
int mc_pathtrace_budget_resolve(uint32_t width, uint32_t height, const float* acc, const uint8_t* levels, float* out);
int mc_pathtrace_budget_levels_device_async(mc_context* ctx, uint32_t width, uint32_t height, const void* d_variance, float target,
                                            uint32_t max_level, void* d_levels, void* stream);
int mc_pathtrace_budget_lists_device_async(mc_context* ctx, uint32_t width, uint32_t height, const void* d_levels, uint32_t max_level,
                                           void* d_list, void* d_counts, void* stream);
int mc_pathtrace_budget_resolve_device_async(mc_context* ctx, uint32_t width, uint32_t height, const void* d_acc, const void* d_levels,
                                             void* d_out, void* stream);
int mc_pathtrace_render_list_device_async(mc_context* ctx, const mc_pathtrace_params* p, const float* planes, uint32_t n_planes,
                                          const float* spheres, uint32_t n_spheres, const void* d_list, uint32_t n_list, float prescale,
                                          void* d_acc, void* stream);
int mc_pathtrace_render_budgeted(mc_context* ctx, const mc_pathtrace_params* p, const mc_pathtrace_budget_params* b, const float* planes,
                                 uint32_t n_planes, const float* spheres, uint32_t n_spheres, float* out_rgba_f32, uint8_t* out_rgba8,
                                 uint8_t* out_levels);
int mc_context_last_budget(mc_context* ctx, uint64_t per_level[9], double* mean_spp);

/* ---- Path tracer through a bounding-volume hierarchy over the spheres (no reference counterpart; additions within ABI 3; DESIGN.md
 *      section 3.18) ---------------------------------------------------------------------------------------------------------------
 * The plain calls test every object for every ray, as the shader's loop does (pathTracer.comp:112-131).  An mc_pathtrace_accel holds a
 * scene's tables and a tree over its spheres; the calls below render through it and return WHAT THE PLAIN CALLS RETURN: in
 * MC_PT_MATH_STRICT the same bits as mc_pathtrace_render, hence as the oracle.  A sphere's hit parameter depends on the ray and that sphere
 * alone, so the loop returns the smallest one, ties to the lowest table index, planes before spheres; the walk visits a subset of the spheres,
 * breaks ties by index, and skips a node only where no sphere in it can pass the fp32 test below the parameter held (csrc/pt_bvh.h has the
 * proof: boxes grown per ray and per node by eta_ray * (an upper bound of |c - o| + |r|), eta_ray = 1.01 (sqrt(2e-6 + 1.3 | |d|^2 - 1 |) + 1e-6),
 * at most 2^-9 for | |d|^2 - 1 | <= 2^-20; a direction with | |d|^2 - 1 | > 0.01 or a NaN culls nothing).  Planes stay a linear list tested
 * first; a sphere whose box cannot be formed (a centre or radius that is not finite, an edge that overflows) stays on a second linear list.
 *
 * mc_pathtrace_accel_create / _destroy / _info / _copy / _intersect: host only, no device, usable without a GPU.  create copies the tables
 *   (12 floats per object, as mc_pathtrace_render takes them); the build is deterministic — the same tables give the same bytes (_copy
 *   writes them: nodes, leaf spheres, leaf indices, the unboxed list; mc_pathtrace_accel_stats.bytes in all).  destroy(NULL) is MC_OK.
 * mc_pathtrace_accel_intersect: intersect() for n_rays rays (origins, dirs: 3 floats each; out_id: -1 or planes 0 .. n_planes-1, spheres
 *   n_planes + i; out_t: the parameter, 1e20-or-above for a miss as the loop leaves it) by the SAME source the kernels run.
 * mc_pathtrace_render_accel, _render_accel_device_async, _render_accel_rgba8: as mc_pathtrace_render, _render_device_async and
 *   _render_rgba8 with the object in place of the tables: sample ranges, row tiles and interleaved row blocks are honoured and compose bit
 *   for bit (strict) with one another and with the plain calls' parts.  MC_PT_MATH_STRICT runs the strict tier; MC_PT_MATH_FAST and
 *   MC_PT_MATH_FAST_CAREFUL both run the careful tier, and mc_pathtrace_accel_select_kernel reports it (kernel = MC_PT_KERNEL_BVH).
 *   The device copy of an object is made once per (object, context), on first use, and freed by mc_pathtrace_accel_destroy or by
 *   mc_context_destroy of that context, whichever comes first (mc_pathtrace_accel_stats.device_copies counts them).
 * Refused with a detail string: a NULL pointer, an object that is not live (destroyed), an empty image / row range / sample range, flags
 *   other than 0 (MC_ERR_INVALID_ARGUMENT); more than 2^20 objects, MC_PT_PRECISION(x) with x != MC_PT_PREC_F32 — named in the detail —
 *   (MC_ERR_UNSUPPORTED).  The automatic choice of mc_pathtrace_render* is unchanged: it never selects this kernel. */
typedef struct mc_pathtrace_accel mc_pathtrace_accel;
typedef struct mc_pathtrace_accel_stats {
    uint32_t n_planes, n_spheres; /* the tables' sizes; n_planes is the length of the first linear list                       */
    uint32_t nodes, depth, leaves; /* of the tree (depth: nodes on the longest root-to-leaf path; 0, 0, 0 without boxed spheres) */
    uint32_t boxed;               /* spheres in the tree                                                                      */
    uint32_t unboxed;             /* spheres on the second linear list                                                        */
    uint32_t device_copies;       /* contexts holding a device copy at the moment                                            */
    uint64_t bytes;               /* of the structure: 32 per node, 20 per boxed sphere, 4 per unboxed sphere                 */
} mc_pathtrace_accel_stats;
int mc_pathtrace_accel_create(const float* planes, uint32_t n_planes, const float* spheres, uint32_t n_spheres, mc_pathtrace_accel** out);
int mc_pathtrace_accel_destroy(mc_pathtrace_accel* a);
int mc_pathtrace_accel_info(const mc_pathtrace_accel* a, mc_pathtrace_accel_stats* out);
int mc_pathtrace_accel_copy(const mc_pathtrace_accel* a, void* out_bytes, uint64_t capacity);
int mc_pathtrace_accel_intersect(const mc_pathtrace_accel* a, uint64_t n_rays, const float* origins, const float* dirs, int32_t* out_id,
                                 float* out_t);
int mc_pathtrace_render_accel(mc_context* ctx, const mc_pathtrace_accel* a, const mc_pathtrace_params* p, float* out_rgba_f32);
int mc_pathtrace_render_accel_device_async(mc_context* ctx, const mc_pathtrace_accel* a, const mc_pathtrace_params* p, void* d_rgba_f32,
                                           void* stream);
int mc_pathtrace_render_accel_rgba8(mc_context* ctx, const mc_pathtrace_accel* a, const mc_pathtrace_params* p, uint8_t* out_rgba8);

/* ---- What runs behind a render, for mc_pathtrace_accel scenes: guides, the denoised and noise-guided chains, the list render and the
 *      budgeted chain (no reference counterpart; additions within ABI 3) -------------------------------------
 * ONE DEFINITION for all six: a call returns what its table form returns for the tables the object was made from.  The walk returns the
 * linear loop's (id, t) for every ray, the accelerated render is the plain render bit for bit in MC_PT_MATH_STRICT, and sample ranges
 * compose; so each chain below is its table form's chain with the guides taken from the tree and every render made through the tree.
 *
 * mc_pathtrace_accel_guides, _guides_device_async  (mirror mc_pathtrace_guides, mc_pathtrace_guides_device_async): the two guide planes,
 *   bit for bit — storage order, a miss as (0, 0, 0, 1e20) and (0, 0, 0, -1).  Strict in every math mode (IEEE divide and square root).
 *   The host form needs no device.  The device form reads the object's cached device copy: nothing is uploaded per call, and
 *   mc_pathtrace_accel_stats.device_copies stays at one per context.  Planes aligned to 16 bytes, not overlapping.
 * mc_pathtrace_render_accel_denoised  (mirrors mc_pathtrace_render_denoised), mc_pathtrace_render_accel_denoised_adaptive  (mirrors
 *   mc_pathtrace_render_denoised_adaptive): the same order and scratch layout, less the records' upload.  In MC_PT_MATH_STRICT the output
 *   is the table form's, bit for bit, f32 and RGBA8.  In MC_PT_MATH_FAST and MC_PT_MATH_FAST_CAREFUL the careful BVH tier renders, as
 *   mc_pathtrace_accel_select_kernel reports, and the promise is the table forms' weaker one: the bits of the same chain made from the
 *   separate public accel calls — NOT the table form's bits, which may come from another tier for the same scene.
 * mc_pathtrace_render_accel_list_device_async  (mirrors mc_pathtrace_render_list_device_async): that call's contract word for word — the
 *   entry -> pixel mapping, acc * prescale with the plane not read when sample_begin == 0, samples added in sample order, never the
 *   final encode, unlisted pixels untouched, an entry >= width * height skipped, n_list == 0 is MC_OK with no launch.  S is the plain
 *   render's rule applied to n_list entries and the range's sample count; a ragged count takes the accelerated render's two launches
 *   (the prescale belongs to the first).
 * mc_pathtrace_render_accel_budgeted  (mirrors mc_pathtrace_render_budgeted): its chain and its promise — in MC_PT_MATH_STRICT out[p] is
 *   mc_pathtrace_render_accel at spp = n0 << level[p], bit for bit; mc_context_last_budget and mc_context_last_timing report as there.
 * Refused as the table forms refuse, with the same status and a detail string; and, as the accelerated render: a NULL or destroyed
 *   object, p->flags other than 0 (MC_ERR_INVALID_ARGUMENT), an MC_PT_PRECISION variant (MC_ERR_UNSUPPORTED, named in the detail).  The
 *   arguments are checked before the context is asked for: every such refusal shows on a machine without a device.
 * Not offered: a warm-up form, mc_multi_*. */
int mc_pathtrace_accel_guides(const mc_pathtrace_accel* a, uint32_t width, uint32_t height, float* out_normal_t, float* out_position_id);
int mc_pathtrace_accel_guides_device_async(mc_context* ctx, const mc_pathtrace_accel* a, uint32_t width, uint32_t height, void* d_normal_t,
                                           void* d_position_id, void* stream);
int mc_pathtrace_render_accel_denoised(mc_context* ctx, const mc_pathtrace_accel* a, const mc_pathtrace_params* p,
                                       const mc_pathtrace_denoise_params* d, float* out_rgba_f32, uint8_t* out_rgba8);
int mc_pathtrace_render_accel_denoised_adaptive(mc_context* ctx, const mc_pathtrace_accel* a, const mc_pathtrace_params* p,
                                                const mc_pathtrace_denoise_params* d, float k_noise, uint32_t radius, float* out_rgba_f32,
                                                uint8_t* out_rgba8);
int mc_pathtrace_render_accel_list_device_async(mc_context* ctx, const mc_pathtrace_accel* a, const mc_pathtrace_params* p, const void* d_list,
                                                uint32_t n_list, float prescale, void* d_acc, void* stream);
int mc_pathtrace_render_accel_budgeted(mc_context* ctx, const mc_pathtrace_accel* a, const mc_pathtrace_params* p,
                                       const mc_pathtrace_budget_params* b, float* out_rgba_f32, uint8_t* out_rgba8, uint8_t* out_levels);

/* ---- cold start (no reference counterpart: vkCreateComputePipelines compiles the shader inside preRun, vulkanComputeApp.cpp:589-643,
 *      before anything is timed; here the runtime loads a kernel family's code object on its first launch, 8 - 12 ms, and the first
 *      full-size launch would pay for it) -----------------------------------------------------------------------------------------
 * mc_context_warmup_*: everything the request's first launch would otherwise do once — device scratch for the whole request (and the
 * RGBA8 image when rgba8 != 0), timing events, scene / colour / c tables, and a 16 x 8 (one-tile) launch of the kernel family the
 * request selects, so that the code object is resident.  Blocks the CALLING thread for the load and returns with the tiny launch
 * queued on the context's stream; results are unaffected (the scratch it touches is overwritten by the render).  An application calls
 * it from a helper thread while it does other start-up work (allocating its storage buffer, opening its output), and joins that
 * thread before its next call on the context (a context is not thread-safe).  (Round 6 also tried to move the storage buffer's
 * allocation BEHIND the launch with a two-phase render call: registering host memory while a kernel runs stalls the device — K4's
 * kernel 82 ms instead of 60 — so the buffer is made first, in 4 ms, and the blocking calls stayed as they were.)
 * mc_context_warmup_mandelbrot's `rgba8`: bit 0 as above, bit 1 = mc_mandelbrot_render_banded will follow (its second stream is made now). */
int mc_context_warmup_pathtrace(mc_context* ctx, const mc_pathtrace_params* p, const float* planes, uint32_t n_planes,
                                const float* spheres, uint32_t n_spheres, int rgba8);
int mc_context_warmup_mandelbrot(mc_context* ctx, const mc_mandelbrot_params* p, int rgba8);

/* Host-side analysis the path tracer applies to a scene before choosing a kernel; touches no device, usable without a
 * GPU.  *out_class: bit 0 (MC_PT_SCENE_SLAB) — six axis-aligned planes in index order x,x,y,y,z,z plus one to eight spheres
 * (the reference scene, pathtracerApp.h:14-39, has three): the specialised slab kernels run; bit 1 (MC_PT_SCENE_LIGHTS_INSIDE) —
 * additionally the planes close a box, the camera (pathTracer.comp:352) and every emissive sphere lie inside it with a
 * margin: shadow rays (pathTracer.comp:420) skip the plane tests.  Both specialisations are bit-exact;
 * every other scene takes the generic kernel.  Bit 2 (MC_PT_SCENE_SPHERES_DISJOINT) — slab scenes: the spheres are pairwise
 * disjoint with a margin; the fast sample-pool kernel then decides shadow rays without square roots, ordering the spheres a ray meets
 * by the projections of their centres (overlapping spheres: its root form; strict math does not depend on it).  Bit 3 (MC_PT_SCENE_LIGHT_ENCLOSED) — any scene: an
 * emissive sphere intersects a non-emissive diffuse sphere (or comes within 1.5 of its own radii of it), or is all but enclosed by a
 * mirror sphere.  Next-event estimation at point-blank range through rays grazing the sphere they start on (pathTracer.comp:325-327,
 * 420) makes such an image a collection of near-ties, which fast math decides differently from the reference arithmetic far more
 * often than its tolerance allows: an MC_PT_MATH_FAST request for such a scene is RENDERED WITH THE STRICT KERNELS
 * (bit-identical to the oracle), never silently outside the bound.  Bit 4 (MC_PT_SCENE_MANY_SPHERES) — any scene: four or more spheres.
 * The share of fast-math samples that take another path than the reference's grows with the number of (specular) spheres a path can
 * run through; on random boxes the fast tier holds the bound with three spheres (36 scenes, at most 3.3 of 4.0), misses it on 2 of 44 with
 * four (5.5, 6.3), reads 3.2 with five and 4.4 .. 5.6 from six on (profiles/r05_fork_census_careful.txt, r06_fast_tier_{3,4}_spheres.txt): an
 * MC_PT_MATH_FAST request for such a scene is rendered by the careful tier (MC_PT_MATH_FAST_CAREFUL).  Bit 5 (MC_PT_SCENE_SPECULAR) — any
 * scene with up to three spheres that has more specular surface than the reference scene (pathtracerApp.h:14-39: diffuse walls, one mirror
 * and one glass sphere of r = 0.8): a mirror or glass wall, or mirror spheres (material 2), or glass spheres (material 3), whose squared radii
 * sum to more than 0.65.  A forked sample that a specular chain carries to a light moves its pixel by the light's whole emission: of 276
 * jittered three-sphere rooms eighteen are outside the bound in the fast tier (up to 8.0) — fourteen of the 132 with a specular wall, two of
 * the 38 with larger mirror spheres, TWO of the 106 this bit leaves to the fast tier (4.2; the others at most 3.8; 76 of them drawn after
 * the rule was set: profiles/r06_fast_tolerance_scenes*.txt).  The careful tier renders the 170 others at 0.8 or less. */
#define MC_PT_SCENE_SLAB 1u
#define MC_PT_SCENE_LIGHTS_INSIDE 2u
#define MC_PT_SCENE_SPHERES_DISJOINT 4u   /* slab scenes: the spheres are pairwise disjoint (the fast pool kernel then needs no square roots for shadow rays) */
#define MC_PT_SCENE_LIGHT_ENCLOSED 8u     /* a light intersecting a diffuse sphere / all but enclosed by a mirror: fast math requests are rendered strict */
#define MC_PT_SCENE_MANY_SPHERES 16u      /* any scene with four or more spheres: an MC_PT_MATH_FAST request is rendered by the careful tier            */
#define MC_PT_SCENE_SPECULAR 32u          /* up to three spheres, more specular surface than the reference scene's: likewise the careful tier          */
int mc_pathtrace_scene_class(const float* planes, uint32_t n_planes, const float* spheres, uint32_t n_spheres,
                             uint32_t* out_class);

/* Which kernel mc_pathtrace_render* will run for a request — decided on the host from the parameters and the scene alone (no
 * device, usable without a GPU).  In MC_PT_MATH_FAST different kernels are different instruction sequences (equal within the
 * tolerance, not bit for bit), so an N-GPU or progressive caller that needs tiles / ranges to compose bit-identically asserts
 * that every part reports the same `kernel` and `lanes_per_pixel` as the whole image does.  Validates like the render call. */
enum {
    MC_PT_KERNEL_GENERIC = 0,        /* any scene, records staged into LDS (pathTracer.comp:112-131 as written)              */
    MC_PT_KERNEL_SLAB = 1,           /* 6 axis-aligned planes + 3 spheres, round-synchronous                                 */
    MC_PT_KERNEL_BOX = 3,            /* closed-box scene facts at compile time, round-synchronous (fast math)                */
    MC_PT_KERNEL_POOL = 4,           /* the sample-pool kernel (the default for the reference scene, both math modes)        */
    MC_PT_KERNEL_GENERIC_MEMORY = 5, /* any scene, records read from memory (large scenes)                                   */
    MC_PT_KERNEL_BVH = 6             /* mc_pathtrace_render_accel*: spheres through a BVH, records read from memory; never automatic */
};
typedef struct mc_pathtrace_kernel_info {
    uint32_t kernel;          /* MC_PT_KERNEL_*                                                                             */
    uint32_t lanes_per_pixel; /* sample-parallel width S: lanes of a wave that share a pixel (1, 4 or 16)                    */
    uint32_t math_mode;       /* the mode that RUNS: for a fast request MC_PT_MATH_FAST, MC_PT_MATH_FAST_CAREFUL (MC_PT_SCENE_MANY_SPHERES,  */
                              /* MC_PT_SCENE_SPECULAR) or MC_PT_MATH_STRICT (MC_PT_SCENE_LIGHT_ENCLOSED)                                    */
    uint32_t launches;        /* kernel launches per call (2: a ragged sample count in the round-synchronous kernels)        */
} mc_pathtrace_kernel_info;
int mc_pathtrace_select_kernel(const mc_pathtrace_params* p, const float* planes, uint32_t n_planes, const float* spheres,
                               uint32_t n_spheres, mc_pathtrace_kernel_info* out);
/* The same for mc_pathtrace_render_accel*: kernel = MC_PT_KERNEL_BVH, the width, the tier that runs, the launches.  Validates like them. */
int mc_pathtrace_accel_select_kernel(const mc_pathtrace_accel* a, const mc_pathtrace_params* p, mc_pathtrace_kernel_info* out);

/* ---- stream / tiling helpers ------------------------------------------------------------------ */
int mc_context_synchronize(mc_context* ctx);
/* Rows per interleave block used by every multi-GPU path of this library (mc_multi_*, bench.py's sharding): rank r of n
 * owns the storage rows whose block index (row / mc_row_block()) is congruent to r mod n.  */
uint32_t mc_row_block(void);
/* Number of storage rows in the tile described by (row_begin,row_end,row_block,row_stride). */
uint32_t mc_tile_rows(uint32_t row_begin, uint32_t row_end, uint32_t row_block, uint32_t row_stride);
/* Reassembles the storage buffer from n_tiles interleaved tiles laid out back to back, each padded to
 * tile_rows_padded rows (the layout an RCCL gather of equal-sized tiles leaves on the root): tile t holds
 * the rows t*row_block + k*n_tiles*row_block + j.  bytes_per_pixel is 16 (vec4 fp32) or 4 (iteration counts). */
int mc_deinterleave_rows_device_async(mc_context* ctx, const void* d_tiles, uint32_t width, uint32_t height,
                                      uint32_t n_tiles, uint32_t row_block, uint32_t tile_rows_padded,
                                      uint32_t bytes_per_pixel, void* d_out, void* stream);

/* Path-tracer RGBA8 exchange on the root (4 B/pixel cross xGMI): d_tiles_rgba8 holds n_tiles interleaved tiles of
 * RGBA8 pixels, each converted by its owner with mc_convert_rgba8_device_async(rotate180 = 0), laid out as
 * mc_deinterleave_rows_device_async expects; writes the whole image d_rgba8 (width*height*4 bytes) in storage-row order and, with
 * rotate180 != 0, point-reflected as PathtracerApp::saveRenderedImage leaves it (pathtracerApp.h:236-243, incl. an odd width's
 * untouched middle column) — the same bytes as mc_pathtrace_render_rgba8 of the whole image on one GPU. */
int mc_assemble_rgba8_device_async(mc_context* ctx, const void* d_tiles_rgba8, uint32_t width, uint32_t height, uint32_t n_tiles,
                                   uint32_t row_block, uint32_t tile_rows_padded, int rotate180, void* d_rgba8, void* stream);

/* Mandelbrot exchange on the root: d_tiles holds n_tiles interleaved tiles of ITERATION COUNTS (iters_bytes = 2: uint16_t,
 * MC_MANDEL_ITERS_U16; 4: uint32_t) laid out as mc_deinterleave_rows_device_async expects; writes the whole image's storage
 * buffer d_rgba_f32 (lut[n] per pixel: exactly what the render kernel writes for that count, mandelbrot.comp:50-59) and/or its
 * uint32 count plane d_iters.  The ranks of a multi-GPU render then exchange 2-4 B/pixel instead of 16. */
int mc_mandelbrot_assemble_device_async(mc_context* ctx, const mc_mandelbrot_params* p, const void* d_tiles, uint32_t iters_bytes,
                                        uint32_t n_tiles, uint32_t row_block, uint32_t tile_rows_padded, void* d_rgba_f32,
                                        void* d_iters, void* stream);

/* ---- single-process multi-GPU render (north_star: row tiles + RCCL gather to rank 0) --------------
 * Renders the whole image on n_devices GPUs of this node (interleaved row blocks), gathers
 * the fp32 tiles to device 0 with RCCL over xGMI and copies the assembled storage buffer to
 * out_rgba_f32 (host, width*height*4 floats).  n_devices = 1 degenerates to the single-GPU path. */
typedef struct mc_multi mc_multi;
int mc_multi_create(int n_devices, mc_multi** out);
int mc_multi_destroy(mc_multi* m);
int mc_multi_mandelbrot_render(mc_multi* m, const mc_mandelbrot_params* p, float* out_rgba_f32, uint32_t* out_iters);
int mc_multi_pathtrace_render(mc_multi* m, const mc_pathtrace_params* p, const float* planes, uint32_t n_planes,
                              const float* spheres, uint32_t n_spheres, float* out_rgba_f32);
/* As mc_*_render_rgba8: only RGBA8 leaves the GPU.  Mandelbrot: device 0 converts the storage buffer it rebuilt from the gathered
 * counts.  Path tracer: every device converts its own tile, the gather moves 4 B/pixel, device 0 de-interleaves and applies the
 * point reflection on bytes (mc_assemble_rgba8_device_async). */
int mc_multi_mandelbrot_render_rgba8(mc_multi* m, const mc_mandelbrot_params* p, uint8_t* out_rgba8);
int mc_multi_pathtrace_render_rgba8(mc_multi* m, const mc_pathtrace_params* p, const float* planes, uint32_t n_planes,
                                    const float* spheres, uint32_t n_spheres, uint8_t* out_rgba8);

#ifdef __cplusplus
}
#endif
#endif /* MC_COMPUTE_H_ */
