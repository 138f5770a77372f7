/* Device self-test hooks of the parity suite: libmc_compute_test.so (vulkan-compute-tests_amd/csrc/test_hooks.hip).
 * TEST INFRASTRUCTURE, not part of the drop-in boundary: a binding of the reference never sees these — they evaluate the
 * device functions the kernels are built from (the explicit fp32 math of the strict mode, the two-float primitives of
 * shaders/emulateDouble.h.glsl:59-139, rand01 of shaders/pathTracer.comp:107-110) over arrays, so that tests/ can compare
 * them with the oracle bit for bit.  Contexts come from libmc_compute.so (mc_context_create). */
#ifndef MC_COMPUTE_TEST_H_
#define MC_COMPUTE_TEST_H_
#include "mc_compute.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- measurement switches: bits of mc_mandelbrot_params.flags / mc_pathtrace_params.flags that libmc_compute.so honours for
 *      this repository's tools (tools/, tests/: A/B timings, forced kernels, the unguarded fast kernels).  They are NOT part of
 *      the boundary a reference maintainer binds (include/mc_compute.h offers precision, math mode, tiling and the sample
 *      range — nothing that can leave a mode's parity contract); MC_PT_NO_FAST_GUARD in particular lets fast math run where it
 *      cannot hold its tolerance.  In MC_PT_MATH_STRICT every accepted combination produces bit-identical buffers; in
 *      MC_PT_MATH_FAST the kernels selected by different flags are different instruction sequences that agree within the
 *      fast-math tolerance. */
enum {
    MC_MANDEL_FMA = 1u << 0,      /* NON-PARITY: allow fp contraction in the fp32 Mandelbrot loop */
    /* bit 1 is MC_MANDEL_ITERS_U16 (include/mc_compute.h) */
    MC_MANDEL_PERTURB_FORCE_DEEP = 1u << 2,/* MC_PRECISION_PERTURB: render any bound orbit with the deep kernel (the rescaled    */
                                           /* loop of include/mc_compute.h) — how the tests check that its plain phase is        */
                                           /* StatePerturb bit for bit.  Shipped code never sets it                               */
    MC_MANDEL_BLA_COUNT_TRIPS = 1u << 3    /* MC_PRECISION_PERTURB_BLA and _BLA_DEEP: each pixel's loop-trip count (skips + exact */
                                           /* iterations, the escaping one included; in [1, M]) is written in place of n, and the  */
                                           /* colour is lut[trips] — how the tests see skipping without a timer                    */
};
enum {
    MC_PT_GENERIC_KERNEL = 1u << 0, /* never use the axis-aligned-slab specialisation of the plane test */
    /* bit 1 is reserved (rounds 2-3: a lane-regrouping experiment, removed) */
    MC_PT_NO_BOX_KERNEL = 1u << 2,  /* fast math: never use the closed-box specialisations (compile-time scene facts, the     */
                                    /* sample-pool kernel); the general fast slab kernel runs instead                         */
    MC_PT_NO_POOL_KERNEL = 1u << 3, /* never use the sample-pool kernel (csrc/pathtrace_pool.h); the round-synchronous        */
                                    /* kernels run instead                                                                   */
    MC_PT_SCENE_IN_LDS = 1u << 4,   /* generic scenes: every block stages the object records into LDS (the automatic choice   */
    MC_PT_SCENE_IN_MEMORY = 1u << 5,/* for small scenes) / the kernel reads them where they lie (large scenes); strict math:  */
                                    /* bit-identical either way                                                             */
    MC_PT_NO_FAST_GUARD = 1u << 6   /* run the fast TIER (tier 1) of MC_PT_MATH_FAST whatever the host's scene class says: neither     */
                                    /* the promotion to strict (MC_PT_SCENE_LIGHT_ENCLOSED) nor the promotion to the careful tier      */
                                    /* (MC_PT_SCENE_MANY_SPHERES, MC_PT_SCENE_SPECULAR) is applied — this is how tools force "tier 1"     */
};
#define MC_PT_FORCE_S(s) ((uint32_t)(s) << 8) /* force the sample-parallel width: 1, 4 or 16 (0 = automatic) */

/* fn: 0 mc_sin, 1 mc_cos, 2 mc_log2, 3 mc_exp2, 4 pow(x,0.45), 5 inversesqrt, 6 sqrt, 7 1/x,
 * 8/9 sin/cos via the fused mc_sincos; fast=1 evaluates the MC_PT_MATH_FAST variants instead, fast=2 the careful tier's
 * unguarded short forms (fn 5, 6, 7 only; any other fn is MC_ERR_INVALID_ARGUMENT). */
int mc_test_math(mc_context* ctx, int fn, int fast, const float* in, float* out, size_t n);
/* Strict (a[3i], a[3i+1], a[3i+2]) / s[i] as the path tracer divides a colour by a probability, by pi, by the sample count (short
 * division inside its window, IEEE expansion outside); with_y != 0: the reciprocal RN(1/s) is supplied instead of computed. */
int mc_test_div3(mc_context* ctx, int with_y, const float* a, const float* s, float* out, size_t n);
/* Strict fn 5 / 6 / 7 (and the guarded short reciprocal) over EVERY fp32 bit pattern first_bits .. first_bits+count-1, compared on
 * the device with the compiler's IEEE expansion: *mismatches (NaN == NaN), *checksum = sum of (result_bits ^ (bits * 0x9E3779B1))
 * mod 2^64 for a host-side comparison, *first_mismatch = lowest offending pattern (0xffffffff if none). */
int mc_test_math_sweep(mc_context* ctx, int fn, uint32_t first_bits, uint64_t count, uint64_t* mismatches, uint64_t* checksum,
                       uint32_t* first_mismatch);
/* rand01 (pathTracer.comp:107-110) over n keys (x,y,z) -> 3 floats each. */
int mc_test_rand01(mc_context* ctx, const uint32_t* xyz, float* out, size_t n);
/* two-float primitives (emulateDouble.h.glsl): op 0 ds_add, 1 ds_sub, 2 ds_mul, 3 ds_compare, 4 ds_sqrt(a), 5 df64_add,
 * 6 df64_mult, 7 df64_sqrt(a), 8 ds_twoProd(a.hi,b.hi), 9 ds_div, 10 twoDiff(a.hi,b.hi), 11 (df64_eq, df64_neq) as 0/1,
 * 12 ds_mul with the one-fma error term (the two-float Mandelbrot's fast block; equals op 2 for |hi| in [2^-50, 2^60));
 * n pairs of (hi,lo). */
int mc_test_ds_op(mc_context* ctx, int op, const float* a, const float* b, float* out, size_t n);
/* The refine list of MC_MANDEL_SUPERSAMPLE_ADAPTIVE (include/mc_compute.h) on a caller's DEVICE plane of W x H counts (iters_bytes 2:
 * uint16_t, 4: uint32_t): the indices y * W + x of the refined pixels are written to d_list (device, room for W * H uint32_t) in no
 * particular order, their number to *d_count (device; zeroed by the call).  Asynchronous on `stream` (NULL = the context's stream).
 * (Named mc_hook_*, not mc_test_*: the five mc_test_* functions above are the device-function evaluators tests/test_abi.py counts; this
 * one runs a kernel of the product library on a caller's plane.) */
int mc_hook_mandel_refine(mc_context* ctx, const void* d_plane, uint32_t iters_bytes, uint32_t width, uint32_t height, uint32_t* d_list,
                          uint32_t* d_count, void* stream);
/* The per-lane audit of the Mandelbrot escape loop's fast block (csrc/mandel_block_audit.h).  Every state of the
 * loop promises, per lane: when its needs_exact test of a block is false, no iteration of the block escaped and the state after the
 * block's fast iterations equals the state after as many exact steps, bit for bit.  The audit runs each pixel (lane) alone: every block
 * is stepped exactly, and every block after the first is also run fast from the saved state.  Four uint32_t per lane: n (the count the
 * render gives), accepted_blocks (needs_exact false), raised_blocks, first_bad (i of the first accepted block in which a step escaped
 * or the states differ; 0xffffffff if none).  sabotage != 0: needs_exact is taken as false for every block — only what counts as
 * accepted changes, the lane still continues from the exact state — so first_bad then shows what the test is there to catch.  Blocking.
 * mc_hook_mandel_block_audit: MC_PRECISION_F32 (MC_MANDEL_FMA honoured), _DS, _F64 on p's whole image or contiguous rows
 *   [row_begin, row_end) with the c table of the render; out: (row_end - row_begin) x width x 4.  Any other precision or flag, or an
 *   interleaved tile, is MC_ERR_INVALID_ARGUMENT.
 * mc_hook_mandel_perturb_block_audit: the perturbation states on a caller's orbit table orbit_xy (Z_0 .. Z_L as L + 1 (re, im) pairs;
 *   any values, not only a real centre's) and n_lanes lanes of offsets (ux[k], uy[k]).  deep == 0: the plain loop, offsets are dc.
 *   deep != 0: the rescaled loop with E = exp2, offsets u * 2^exp2.  out: n_lanes x 4.  L == 0, n_lanes == 0 (or > 2^24), max_iter == 0
 *   or a NULL pointer is MC_ERR_INVALID_ARGUMENT. */
int mc_hook_mandel_block_audit(mc_context* ctx, const mc_mandelbrot_params* p, int sabotage, uint32_t* out);
int mc_hook_mandel_perturb_block_audit(mc_context* ctx, const double* orbit_xy, uint32_t L, int deep, int32_t exp2, const double* ux,
                                       const double* uy, size_t n_lanes, uint32_t max_iter, int sabotage, uint32_t* out);
/* The arithmetic of mc_mandelbrot_orbit_create_device (csrc/mandel_orbit_fix.h), piece by piece.  Numbers are k + 1 uint64_t limbs, least
 * significant first: k fractional limbs and the integer limb, 1 <= k <= 130 (MC_ERR_INVALID_ARGUMENT otherwise).
 * mc_hook_orbit_mul_host: out = (a * b + 2^(64k - 1)) >> 64k, its low k + 1 limbs, by the shared header's columns and carry resolution run
 *   as lane loops on the CPU (no device).  mc_hook_orbit_mul_device: the same phases as the kernel runs them, one workgroup on ctx's device.
 * mc_hook_orbit_to_double_host: the shared to_double (top-bit search, 53 bits, half bit, sticky bit; the subnormal floor) of the magnitude
 *   `limbs` with sign `neg`, on the CPU.
 * mc_hook_orbit_create_lanes_host: mc_mandelbrot_orbit_create_deep with the iteration loop replaced by the kernel's phases as lane loops
 *   on the CPU (no device): the whole device algorithm, checkable on a box without a GPU. */
/* The BLA tables built on the device (mc_context_bind_mandelbrot_orbit_tables, csrc/mandel_bla_table.hip): a workgroup carries this many
 * adjacent entries of a level up through the levels above them, so a level of at most this many entries, and every level above it, is
 * built by a single workgroup, and a launch builds log2(this) + 1 levels.  A power of two.  The tests read it here, to place their table
 * shapes on either side of it. */
#define MC_BLA_TABLE_GROUP_ENTRIES 1024u
int mc_hook_orbit_mul_host(int k, const uint64_t* a_limbs, const uint64_t* b_limbs, uint64_t* out_limbs);
int mc_hook_orbit_mul_device(mc_context* ctx, int k, const uint64_t* a_limbs, const uint64_t* b_limbs, uint64_t* out_limbs);
int mc_hook_orbit_to_double_host(int k, const uint64_t* limbs, int neg, double* out);
int mc_hook_orbit_create_lanes_host(const char* centre_x, const char* centre_y, double scale_x, double scale_y, int32_t scale_exp2,
                                    uint32_t max_iter, mc_mandelbrot_orbit** out);

#ifdef __cplusplus
}
#endif
#endif /* MC_COMPUTE_TEST_H_ */
