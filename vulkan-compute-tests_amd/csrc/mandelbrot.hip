// Mandelbrot escape-time kernels for gfx950 (MI355X).
//
// Replaces shaders/mandelbrot.comp:21-60 (fp32) and adds the two-float deep-zoom variant composed
// from the reference's ds_* primitives (shaders/emulateDouble.h.glsl:59-139), and the
// native fp64 variant the reference's USE_NATIVE_FP64 switch stands for (emulateDouble.h.glsl:13).  The
// perturbation variant (MC_PRECISION_PERTURB) lives in mandel_perturb.hip; both run the escape-time loop of mandel_escape.h.
//
// Design (MI355X-first, not a translation of the 32x32 Vulkan workgroup):
//  * one work-item per pixel; a wave64 owns an 8x8 pixel tile (coherent trip counts, and every
//    128-B output segment of a row is written whole); one wave per workgroup.
//  * the escape test is a wave ballot (`v_cmp_* sgpr-pair`), not an exec-mask update: the loop body
//    is straight-line VALU for U iterations and all bookkeeping (OR of the U ballots, "every lane
//    done" early-out, iteration counter) runs on the scalar unit.  Per-lane iteration counts are
//    reconstructed from the saved ballots only in the (rare) blocks where some lane escapes.
//  * v_cmp_*_f32 costs 4 issue cycles on gfx950 but v_or_b32 only 2 (tools/valu_microbench.hip): the fp32
//    fast path ORs the bit patterns of the block's |z|^2 values (bit 30 set <=> value >= 2) and compares
//    once per block; the exact ballots are recomputed from the block's saved state only when an unfinished
//    lane may have escaped.  Interior tiles issue 8 fp32 ops + 1 v_or per pixel-iteration (18 cycles).
//  * unfused IEEE fp32 in GLSL source order: this TU is built with -ffp-contract=off.
//    zx*zx and zy*zy are computed once per iteration and reused by the magnitude test and the next
//    update — identical values, so identical results to the literal `dot(z,z)` (mandelbrot.comp:43-44).
//  * the colour is a host-built (max_iter+1)-entry vec4 LUT: only max_iter+1 distinct
//    colours exist and GLSL cos() precision is implementation-defined.
#include <cmath>
#include <cstring>

#include "ds_arith.h"
#include "mandel_kernels.h"
#include "mandel_smooth_host.h"
#include "mc_internal.h"

namespace mc {

namespace {

struct MandelArgs {
    uint32_t W, H, max_iter;
    uint32_t row_begin, row_end, row_block, row_stride;
    float cx_hi, cx_lo, cy_hi, cy_lo;
    float sx_hi, sx_lo, sy_hi, sy_lo;
    float4* __restrict__ out_rgba;      // tile-local, may be null
    uint32_t* __restrict__ out_iters;   // tile-local, may be null
    uint16_t* __restrict__ out_iters16; // the same plane as 16-bit counts (MC_MANDEL_ITERS_U16, max_iter <= 65535), may be null
    const float4* __restrict__ lut;     // max_iter+1 entries (null when out_rgba is null)
    // c = centre + (uv - 0.5) * scale per column / per row, evaluated once on the host with the shader's fp32
    // operation sequence (mandelbrot.comp:30-31,38): fp32 [cx[W] | cy[H]], two-float [cx(hi,lo)[W] | cy(hi,lo)[H]],
    // fp64 double [cx[W] | cy[H]] (read through a double pointer).
    // Replaces two IEEE divisions (~50 instructions) per pixel; exterior tiles only run a handful of iterations.
    const float* __restrict__ c_tab;
};
// MandelArgs keeps its own layout: it is its own target block (mandel_kernels.h)
__host__ __device__ __forceinline__ const MandelArgs& target_of(const MandelArgs& a) { return a; }

// ---- per-pixel state machines: step() advances one iteration and reports "escaped now" ----------
template <bool FMA>
struct StateF32 {
    using Args = MandelArgs;
    static constexpr int kBlock = 8;                   // the escape-time block length U
    static constexpr bool kEscapeCBeforeLoop = true;   // c sits in registers: the smooth kernels convert it before the loop
    float cx, cy, zx, zy, sx, sy;   // sx = zx*zx, sy = zy*zy of the current z
    __device__ __forceinline__ void init(uint32_t gx, uint32_t gy, const MandelArgs& a) {
        cx = a.c_tab[gx];                          // mandelbrot.comp:30,38 (host-evaluated, see build_c_table)
        cy = a.c_tab[a.W + gy];                    // :31,38
        zx = zy = sx = sy = 0.0f;
    }
    // One iteration (:43), returns |z|^2 = dot(z,z) of the new z (:44).
    __device__ __forceinline__ float advance() {
        float nzx, nzy;
        if (FMA) {   // NON-PARITY diagnostic variant (MC_MANDEL_FMA)
            nzx = __builtin_fmaf(zx, zx, -sy) + cx;
            nzy = __builtin_fmaf(2.0f * zx, zy, cy);
        } else {
            nzx = (sx - sy) + cx;
            nzy = ((2.0f * zx) * zy) + cy;
        }
        zx = nzx; zy = nzy;
        sx = zx * zx; sy = zy * zy;
        return sx + sy;
    }
    __device__ __forceinline__ bool step() { return advance() > 2.0f; }   // :44
    // z is the orbit's complete state (sx, sy are functions of it): equal z => equal future (see escape_time)
    __device__ __forceinline__ bool same_z(const StateF32& o) const { return zx == o.zx && zy == o.zy; }
    // MC_MANDEL_COLOUR_SMOOTH: the z the last step() tested and the lane's c, as doubles (exact conversions)
    __device__ __forceinline__ void escape_z(double& x, double& y) const { x = (double)zx; y = (double)zy; }
    __device__ __forceinline__ void escape_c(double& x, double& y) const { x = (double)cx; y = (double)cy; }
    static constexpr uint32_t kCycleCheckBlocks = 1;   // compare with the reference state after every block (8 iterations)
    // Conservative escape filter on the bit pattern of |z|^2 (>= 0, or NaN after an overflow): every value
    // > 2.0f has bit 30 set or is 0x40000001..., every value < 2.0f has bit 30 clear, so the bitwise OR of a
    // block's magnitudes exceeds 0x40000000 whenever any of them exceeded 2.0f (no false negatives; the only
    // false positives involve a magnitude of exactly 2.0f).  v_or_b32 issues in 2 cycles, v_cmp_*_f32 in 4.
    static constexpr bool kHasFastBlock = true;
    using Acc = uint32_t;
    __device__ __forceinline__ Acc acc_init() const { return 0u; }
    __device__ __forceinline__ void advance_fast(Acc& acc) { acc |= __float_as_uint(advance()); }
    static __device__ __forceinline__ bool needs_exact(Acc or_of_bits) { return or_of_bits > 0x40000000u; }
    // every word the state iterates on, by bit pattern (mandel_block_audit.h)
    __device__ __forceinline__ bool bits_equal(const StateF32& o) const {
        return same_bits(cx, o.cx) && same_bits(cy, o.cy) && same_bits(zx, o.zx) && same_bits(zy, o.zy) && same_bits(sx, o.sx) &&
               same_bits(sy, o.sy);
    }
};

struct StateDS {
    using Args = MandelArgs;
    static constexpr int kBlock = 4;                   // the escape-time block length U
    static constexpr bool kEscapeCBeforeLoop = true;   // c sits in registers: the smooth kernels convert it before the loop
    ds2 cx, cy, zx, zy, sx, sy;
    __device__ __forceinline__ void init(uint32_t gx, uint32_t gy, const MandelArgs& a) {
        const float2* tab = reinterpret_cast<const float2*>(a.c_tab);
        float2 tx = tab[gx], ty = tab[a.W + gy];
        cx = ds2{tx.x, tx.y};
        cy = ds2{ty.x, ty.y};
        zx = zy = sx = sy = ds_set(0.0f);
    }
    // Fast block: the same iteration with
    //  (1) the Dekker error term of each product replaced by ONE fma — bit-identical whenever the error term is
    //      representable (tools/dekker_vs_fma.c; error-free transformation), which holds for |operand| >= 2^-50;
    //      `mn` tracks the smallest square seen, a block containing a smaller operand (or an exact zero) is redone
    //      with the literal sequence;
    //  (2) the 11-flop ds_add + 3-way compare of the escape test replaced by t = sx.hi + sy.hi and an integer
    //      max: ds_add(sx, sy).hi differs from t by < 4 ulp (|t2| <= 1/2 ulp(t) + |sx.lo| + |sy.lo|), so
    //      t < 2 - 16 ulp proves "not escaped"; a block that gets closer is redone exactly.
    // Both substitutions leave the state words of every unfinished lane bit-identical to step()'s.
    static constexpr bool kHasFastBlock = true;
    struct Acc {
        uint32_t mx;   // max over the block of bits(t), unsigned: a negative or NaN t reads as "large"
        int32_t mn;    // min over the block of bits(square.hi), signed: a negative square reads as "small"
    };
    __device__ __forceinline__ Acc acc_init() const {
        int32_t a = __float_as_int(sx.hi), b = __float_as_int(sy.hi);
        return Acc{0u, a < b ? a : b};   // the incoming z is an operand of this block's first zx*zy
    }
    __device__ __forceinline__ void advance_fast(Acc& acc) {
        ds2 zxy = ds_mul_fma(zx, zy);
        ds2 twoxy = ds2{2.0f * zxy.hi, 2.0f * zxy.lo};
        ds2 nzx = ds_add(ds_sub(sx, sy), cx);
        ds2 nzy = ds_add(twoxy, cy);
        zx = nzx; zy = nzy;
        sx = ds_mul_fma(zx, zx); sy = ds_mul_fma(zy, zy);
        int32_t bx = __float_as_int(sx.hi), by = __float_as_int(sy.hi);
        uint32_t bt = __float_as_uint(sx.hi + sy.hi);
        acc.mx = acc.mx > bt ? acc.mx : bt;
        int32_t m = bx < by ? bx : by;
        acc.mn = acc.mn < m ? acc.mn : m;
    }
    static __device__ __forceinline__ bool needs_exact(Acc acc) {
        // 0x3ffffff0 = 2 - 16 ulp; 0x0e800000 = 2^-98 > (2^-50)^2 (sx.hi is within an ulp of zx.hi^2)
        return acc.mx >= 0x3ffffff0u || acc.mn < 0x0e800000;
    }
    __device__ __forceinline__ bool same_z(const StateDS& o) const {
        return zx.hi == o.zx.hi && zx.lo == o.zx.lo && zy.hi == o.zy.hi && zy.lo == o.zy.lo;
    }
    // MC_MANDEL_COLOUR_SMOOTH: (double)hi + (double)lo of z and c
    __device__ __forceinline__ void escape_z(double& x, double& y) const { x = (double)zx.hi + (double)zx.lo; y = (double)zy.hi + (double)zy.lo; }
    __device__ __forceinline__ void escape_c(double& x, double& y) const { x = (double)cx.hi + (double)cx.lo; y = (double)cy.hi + (double)cy.lo; }
    static constexpr uint32_t kCycleCheckBlocks = 4;   // every 4 blocks (16 iterations): deep-zoom views have few cycling pixels
    __device__ __forceinline__ bool step() {
        ds2 zxy = ds_mul(zx, zy);
        ds2 twoxy = ds2{2.0f * zxy.hi, 2.0f * zxy.lo};   // exact
        ds2 nzx = ds_add(ds_sub(sx, sy), cx);
        ds2 nzy = ds_add(twoxy, cy);
        zx = nzx; zy = nzy;
        sx = ds_sqr(zx); sy = ds_sqr(zy);
        return ds_greater(ds_add(sx, sy), ds_set(2.0f));
    }
    __device__ __forceinline__ bool bits_equal(const StateDS& o) const {   // (mandel_block_audit.h)
        auto eq = [](ds2 a, ds2 b) { return same_bits(a.hi, b.hi) && same_bits(a.lo, b.lo); };
        return eq(cx, o.cx) && eq(cy, o.cy) && eq(zx, o.zx) && eq(zy, o.zy) && eq(sx, o.sx) && eq(sy, o.sy);
    }
};

// Native IEEE double (MC_PRECISION_F64; the exact contract is in include/mc_compute.h).  The loop of StateF32<false> in
// double: 5 v_add_f64 (2*zx is an add) + 3 v_mul_f64 per iteration, no contraction (-ffp-contract=off).  fp64 denormals
// stay enabled (the gfx9 default; the kernel descriptor's FLOAT_DENORM_MODE_16_64 is 3), so orbits that pass near 0
// round as IEEE does.
struct StateF64 {
    using Args = MandelArgs;
    static constexpr int kBlock = 8;                   // the escape-time block length U
    static constexpr bool kEscapeCBeforeLoop = true;   // c sits in registers: the smooth kernels convert it before the loop
    double cx, cy, zx, zy, sx, sy;   // sx = zx*zx, sy = zy*zy of the current z
    __device__ __forceinline__ void init(uint32_t gx, uint32_t gy, const MandelArgs& a) {
        const double* tab = reinterpret_cast<const double*>(a.c_tab);
        cx = tab[gx];
        cy = tab[a.W + gy];
        zx = zy = sx = sy = 0.0;
    }
    __device__ __forceinline__ double advance() {
        double nzx = (sx - sy) + cx;
        double nzy = ((2.0 * zx) * zy) + cy;
        zx = nzx; zy = nzy;
        sx = zx * zx; sy = zy * zy;
        return sx + sy;
    }
    __device__ __forceinline__ bool step() { return advance() > 2.0; }
    __device__ __forceinline__ bool same_z(const StateF64& o) const { return zx == o.zx && zy == o.zy; }
    __device__ __forceinline__ void escape_z(double& x, double& y) const { x = zx; y = zy; }   // MC_MANDEL_COLOUR_SMOOTH
    __device__ __forceinline__ void escape_c(double& x, double& y) const { x = cx; y = cy; }
    static constexpr uint32_t kCycleCheckBlocks = 1;   // every block (8 iterations), as fp32: 2 v_cmp_f64 against ~66 VALU ops
    // StateF32's filter on the HIGH word of |z|^2 (>= 0, or NaN): every value >= 2.0 (and inf, and any NaN) has a high word
    // >= 0x40000000, every value < 2.0 one <= 0x3fffffff.  So the OR of a block's high words exceeds 0x3fffffff whenever one of
    // them escaped (no false negatives); the only false positives are magnitudes of exactly 2.0.  The compiler ORs the whole
    // 64-bit words (6 v_or3_b32 / v_or_b32 per 8 iterations) and compares once.
    static constexpr bool kHasFastBlock = true;
    using Acc = uint32_t;
    __device__ __forceinline__ Acc acc_init() const { return 0u; }
    __device__ __forceinline__ void advance_fast(Acc& acc) { acc |= (uint32_t)((uint64_t)__double_as_longlong(advance()) >> 32); }
    static __device__ __forceinline__ bool needs_exact(Acc or_of_high_words) { return or_of_high_words > 0x3fffffffu; }
    __device__ __forceinline__ bool bits_equal(const StateF64& o) const {   // (mandel_block_audit.h)
        return same_bits(cx, o.cx) && same_bits(cy, o.cy) && same_bits(zx, o.zx) && same_bits(zy, o.zy) && same_bits(sx, o.sx) &&
               same_bits(sy, o.sy);
    }
};

}  // namespace

// colour(n) = d + e*cos(6.28318*(f*t+g)), t = n/M — mandelbrot.comp:50-56, evaluated in fp32 in source
// order on the host (d = kColor.rgb, mandelbrotApp.h:139-141).  alpha = 1.0.
void mandelbrot_build_lut(uint32_t max_iter, const float k_color[4], float* lut) {
    const float e[3] = {-0.2f, -0.3f, -0.5f};
    const float f[3] = {2.1f, 2.0f, 3.0f};
    const float g[3] = {0.0f, 0.1f, 0.0f};
    for (uint32_t n = 0; n <= max_iter; n++) {
        float t = (float)n / (float)max_iter;
        for (int c = 0; c < 3; c++) {
            float arg = 6.28318f * (f[c] * t + g[c]);
            lut[4 * (size_t)n + c] = k_color[c] + e[c] * cosf(arg);
        }
        lut[4 * (size_t)n + 3] = 1.0f;
    }
}

static int ensure_lut(mc_context* ctx, const mc_mandelbrot_params* p, hipStream_t s) {
    if (ctx->lut_max_iter == p->max_iter && std::memcmp(ctx->lut_kcolor, p->k_color, sizeof(float) * 4) == 0 && ctx->lut.ptr)
        return MC_OK;
    size_t bytes = ((size_t)p->max_iter + 1) * 4 * sizeof(float);
    std::vector<float> host(((size_t)p->max_iter + 1) * 4);
    mandelbrot_build_lut(p->max_iter, p->k_color, host.data());
    // a previous launch of this context may still be reading the old table (possibly on another stream): wait for
    // the streams this context has launched on — not the whole device — before replacing it
    int rc = ctx->drain_launch_streams();
    if (rc) return rc;
    if ((rc = ctx->lut.reserve(bytes))) return rc;
    MC_HIP_TRY(hipMemcpyAsync(ctx->lut.ptr, host.data(), bytes, hipMemcpyHostToDevice, s));
    MC_HIP_TRY(hipStreamSynchronize(s));   // host vector goes out of scope
    ctx->lut_max_iter = p->max_iter;
    std::memcpy(ctx->lut_kcolor, p->k_color, sizeof(float) * 4);
    return MC_OK;
}

// Per-column / per-row c tables.  x = float(gx)/float(W) (mandelbrot.comp:30), c.x = centre.x + (x - 0.5)*scale.x (:38) in
// fp32 source order; the two-float variant composes ds_add(centre, ds_mul(ds_set(x - 0.5), scale)); the fp64
// variant computes x = double(gx)/double(W), c.x = (hi + lo) + (x - 0.5)*(scale hi + lo) in double (include/mc_compute.h).
// Host and device execute the same IEEE operations (no contraction), so the tables hold exactly the values the
// kernel used to compute per pixel.  Cached in the context, keyed by (W, H, precision, view).
static int ensure_c_table(mc_context* ctx, const mc_mandelbrot_params* p, hipStream_t s) {
    std::vector<float> key = {(float)p->width, (float)p->height, (float)p->precision, p->centre_x_hi, p->centre_x_lo,
                              p->centre_y_hi, p->centre_y_lo, p->scale_x_hi, p->scale_x_lo, p->scale_y_hi, p->scale_y_lo};
    if (ctx->ctab.ptr && ctx->ctab_key.size() == key.size() &&
        std::memcmp(ctx->ctab_key.data(), key.data(), key.size() * sizeof(float)) == 0)
        return MC_OK;
    const uint32_t W = p->width, H = p->height;
    const bool ds = p->precision == MC_PRECISION_DS, f64 = p->precision == MC_PRECISION_F64;
    std::vector<float> tab(((size_t)W + H) * (ds || f64 ? 2 : 1));
    for (uint32_t g = 0; g < W + H; g++) {
        if (f64) {
            const bool is_x = g < W;
            const double u = is_x ? (double)g / (double)W : (double)(g - W) / (double)H;
            const double c = is_x ? (double)p->centre_x_hi + (double)p->centre_x_lo : (double)p->centre_y_hi + (double)p->centre_y_lo;
            const double sc = is_x ? (double)p->scale_x_hi + (double)p->scale_x_lo : (double)p->scale_y_hi + (double)p->scale_y_lo;
            const double v = c + (u - 0.5) * sc;
            std::memcpy(&tab[2 * (size_t)g], &v, sizeof v);
            continue;
        }
        const bool is_x = g < W;
        const float u = is_x ? (float)g / (float)W : (float)(g - W) / (float)H;
        const float c_hi = is_x ? p->centre_x_hi : p->centre_y_hi, c_lo = is_x ? p->centre_x_lo : p->centre_y_lo;
        const float s_hi = is_x ? p->scale_x_hi : p->scale_y_hi, s_lo = is_x ? p->scale_x_lo : p->scale_y_lo;
        if (ds) {
            ds2 c = ds_add(ds2{c_hi, c_lo}, ds_mul(ds_set(u - 0.5f), ds2{s_hi, s_lo}));
            tab[2 * (size_t)g] = c.hi;
            tab[2 * (size_t)g + 1] = c.lo;
        } else {
            tab[g] = c_hi + (u - 0.5f) * s_hi;
        }
    }
    int rc = ctx->drain_launch_streams();   // an earlier launch of this context may still read the old table
    if (rc) return rc;
    if ((rc = ctx->ctab.reserve(tab.size() * sizeof(float)))) return rc;
    MC_HIP_TRY(hipMemcpyAsync(ctx->ctab.ptr, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice, s));
    MC_HIP_TRY(hipStreamSynchronize(s));
    ctx->ctab_key = key;
    return MC_OK;
}

// The device colour table of (max_iter, k_color), uploaded on first use (mandelbrot_assemble_launch, postprocess.hip).
int mandelbrot_lut_device(mc_context* ctx, const mc_mandelbrot_params* p, hipStream_t s, const void** d_lut) {
    int rc = ensure_lut(ctx, p, s);
    if (rc) return rc;
    *d_lut = ctx->lut.ptr;
    return MC_OK;
}

// The state of a request: (precision, MC_MANDEL_FMA) chosen in this one place, for the render and for the audit.  f is called with a
// StateTag of the state; smooth says whether the state has the smooth kernels (StateF32<true> has none: MC_MANDEL_FMA with
// MC_MANDEL_COLOUR_SMOOTH is refused before any launch).
template <class State, bool Smooth = true>
struct StateTag {
    using type = State;
    static constexpr bool smooth = Smooth;
};
template <class F>
static int with_state(const mc_mandelbrot_params* p, F&& f) {
    if (p->precision == MC_PRECISION_DS) return f(StateTag<StateDS>{});
    if (p->precision == MC_PRECISION_F64) return f(StateTag<StateF64>{});
    if (p->flags & MC_MANDEL_FMA) return f(StateTag<StateF32<true>, false>{});
    return f(StateTag<StateF32<false>>{});
}

// warm = the cold-start warm-up (mc_context_warmup_mandelbrot): the tables of the REAL request are built and uploaded, then ONE 8 x 8
// tile is run for at most 32 iterations into d_iters — enough for the runtime to load this code object and create the kernel.
// list = the list render of mandel_adaptive.h (p is the sample grid, d_rgba the image the list's pixels are written to, d_iters unused).
// d_smooth: the q plane of MC_MANDEL_COLOUR_SMOOTH (null: not wanted); the flag selects the smooth instantiation of every tile kernel.
// slist = the smooth list render of mandel_adaptive_smooth.h (p is the sample grid and carries MC_MANDEL_COLOUR_SMOOTH; list is null).
static int launch_impl(mc_context* ctx, const mc_mandelbrot_params* p, void* d_rgba, void* d_iters, hipStream_t s, bool warm,
                       const SampleList* list = nullptr, void* d_smooth = nullptr, const SmoothSampleList* slist = nullptr) {
    if (!ctx || !p || (!d_rgba && !d_iters && !d_smooth)) return MC_ERR_INVALID_ARGUMENT;
    const bool smooth = (p->flags & MC_MANDEL_COLOUR_SMOOTH) != 0u;
    if (d_smooth && !smooth) return MC_ERR_INVALID_ARGUMENT;
    if (smooth && list) return MC_ERR_INVALID_ARGUMENT;   // (the integer list kernels colour counts: the entry points refuse the pair)
    if (slist && (!smooth || list || d_smooth || (p->flags & MC_MANDEL_FMA))) return MC_ERR_INVALID_ARGUMENT;
    if (int rc = smooth_refuse_combination(p, "MC_MANDEL_COLOUR_SMOOTH")) return rc;
    if (!p->width || !p->height || !p->max_iter || p->row_end > p->height || p->row_begin >= p->row_end)
        return MC_ERR_INVALID_ARGUMENT;
    if (p->precision != MC_PRECISION_F32 && p->precision != MC_PRECISION_DS && p->precision != MC_PRECISION_F64 &&
        p->precision != MC_PRECISION_PERTURB && p->precision != MC_PRECISION_PERTURB_BLA &&
        p->precision != MC_PRECISION_PERTURB_BLA_DEEP)
        return MC_ERR_INVALID_ARGUMENT;
    if (p->row_stride && (!p->row_block || p->row_block > p->row_stride)) return MC_ERR_INVALID_ARGUMENT;
    if (p->precision == MC_PRECISION_PERTURB || p->precision == MC_PRECISION_PERTURB_BLA ||
        p->precision == MC_PRECISION_PERTURB_BLA_DEEP)
        return perturb_launch(ctx, p, d_rgba, d_iters, s, warm, list, d_smooth, slist);   // mandel_perturb.hip
    if (d_rgba || warm) {
        int rc = ensure_lut(ctx, p, s);
        if (rc) return rc;
    }
    {
        int rc = ensure_c_table(ctx, p, s);
        if (rc) return rc;
    }
    MandelArgs a;
    dim3 grid;
    SampleList l{};
    if (int rc = launch_geometry(p, d_rgba, d_iters, warm, slist ? &slist->l : list, &a, &grid, &l)) return rc;   // mandel_target.h
    a.c_tab = (const float*)ctx->ctab.ptr;
    a.cx_hi = p->centre_x_hi; a.cx_lo = p->centre_x_lo; a.cy_hi = p->centre_y_hi; a.cy_lo = p->centre_y_lo;
    a.sx_hi = p->scale_x_hi; a.sx_lo = p->scale_x_lo; a.sy_hi = p->scale_y_hi; a.sy_lo = p->scale_y_lo;
    a.lut = a.out_rgba ? (const float4*)ctx->lut.ptr : nullptr;
    const SmoothSampleList sl = {l, slist ? slist->pairs : nullptr};
    const int rc = with_state(p, [&](auto tag) {
        using Tag = decltype(tag);
        return launch_state<typename Tag::type, Tag::smooth>(a, grid, s, list ? &l : nullptr, {smooth, (uint32_t*)d_smooth}, slist ? &sl : nullptr);
    });
    if (rc) return rc;
    return ctx->note_launch(s);
}

int mandelbrot_launch(mc_context* ctx, const mc_mandelbrot_params* p, void* d_rgba, void* d_iters, hipStream_t s) {
    return launch_impl(ctx, p, d_rgba, d_iters, s, false);
}

int mandelbrot_smooth_launch(mc_context* ctx, const mc_mandelbrot_params* p, void* d_rgba, void* d_iters, void* d_smooth, hipStream_t s) {
    if (!p || !(p->flags & MC_MANDEL_COLOUR_SMOOTH)) return MC_ERR_INVALID_ARGUMENT;
    return launch_impl(ctx, p, d_rgba, d_iters, s, false, nullptr, d_smooth);
}

int mandelbrot_list_launch(mc_context* ctx, const mc_mandelbrot_params* grid, const SampleList& l, hipStream_t s, bool warm) {
    if (!l.list || !l.count || !l.img_w || !l.table || !l.out_rgba || l.log2s < 1u || l.log2s > 3u) return MC_ERR_INVALID_ARGUMENT;
    return launch_impl(ctx, grid, l.out_rgba, nullptr, s, warm, &l);
}

int mandelbrot_list_smooth_launch(mc_context* ctx, const mc_mandelbrot_params* grid, const SmoothSampleList& sl, hipStream_t s, bool warm) {
    const SampleList& l = sl.l;
    if (!l.list || !l.count || !l.img_w || !l.table || !l.out_rgba || l.log2s < 1u || l.log2s > 3u) return MC_ERR_INVALID_ARGUMENT;
    return launch_impl(ctx, grid, l.out_rgba, nullptr, s, warm, nullptr, nullptr, &sl);
}

int mandelbrot_warmup(mc_context* ctx, const mc_mandelbrot_params* p, void* d_iters_scratch, hipStream_t s) {
    return launch_impl(ctx, p, nullptr, d_iters_scratch, s, true);
}

// mc_hook_mandel_block_audit: F32 (MC_MANDEL_FMA honoured), DS and F64 with the block lengths the render launches, the c table built
// as the render builds it; a whole image or a contiguous row range, no other flag.  d_out: tile rows x W x 4 uint32_t.
int mandelbrot_block_audit_launch(mc_context* ctx, const mc_mandelbrot_params* p, bool sabotage, uint32_t* d_out, hipStream_t s) {
    if (!ctx || !p || !d_out) return MC_ERR_INVALID_ARGUMENT;
    if (!p->width || !p->height || !p->max_iter || p->row_end > p->height || p->row_begin >= p->row_end) return MC_ERR_INVALID_ARGUMENT;
    if (p->precision != MC_PRECISION_F32 && p->precision != MC_PRECISION_DS && p->precision != MC_PRECISION_F64) return MC_ERR_INVALID_ARGUMENT;
    if (p->row_stride || p->row_block) return MC_ERR_INVALID_ARGUMENT;
    const bool fma = (p->flags & MC_MANDEL_FMA) != 0u;
    if ((p->flags & ~(uint32_t)MC_MANDEL_FMA) || (fma && p->precision != MC_PRECISION_F32)) return MC_ERR_INVALID_ARGUMENT;
    if (int rc = ensure_c_table(ctx, p, s)) return rc;
    MandelArgs a;
    dim3 grid;
    SampleList l{};
    if (int rc = launch_geometry(p, nullptr, nullptr, false, nullptr, &a, &grid, &l)) return rc;
    a.c_tab = (const float*)ctx->ctab.ptr;
    a.cx_hi = p->centre_x_hi; a.cx_lo = p->centre_x_lo; a.cy_hi = p->centre_y_hi; a.cy_lo = p->centre_y_lo;
    a.sx_hi = p->scale_x_hi; a.sx_lo = p->scale_x_lo; a.sy_hi = p->scale_y_hi; a.sy_lo = p->scale_y_lo;
    a.lut = nullptr;
    const int rc = with_state(p, [&](auto tag) { return launch_block_audit<typename decltype(tag)::type, false>(a, grid, s, sabotage, d_out); });
    if (rc) return rc;
    return ctx->note_launch(s);
}

// mc_mandelbrot_render_atom / _device_async (include/mc_compute.h: "atom domains").  The refusals in the header's order; F32 and F64 launch
// here with the render's own c table, PERTURB in mandel_perturb.hip.
int mandelbrot_atom_launch(mc_context* ctx, const mc_mandelbrot_params* p, void* d_iters, void* d_period, void* d_amin, hipStream_t s) {
    const std::string fn = "mc_mandelbrot_render_atom";
    auto refuse = [&](const std::string& why, int status) {
        set_error_detail(fn + ": " + why);
        return status;
    };
    if (!ctx || !p) return MC_ERR_INVALID_ARGUMENT;
    if (!d_iters && !d_period && !d_amin) return refuse("all three outputs are NULL", MC_ERR_INVALID_ARGUMENT);
    if (p->flags) return refuse("flags must be 0 (the period plane is built from entry points, not flag bits)", MC_ERR_INVALID_ARGUMENT);
    if (!p->width || !p->height || !p->max_iter) return refuse("width, height and max_iter must be nonzero", MC_ERR_INVALID_ARGUMENT);
    if (!whole_image(p) || p->row_block) return refuse("the whole image only (row_begin = 0, row_end = height, no interleave)", MC_ERR_INVALID_ARGUMENT);
    if (p->precision == MC_PRECISION_DS) return refuse("MC_PRECISION_DS is not supported (F32, F64 and PERTURB are)", MC_ERR_UNSUPPORTED);
    if (p->precision == MC_PRECISION_PERTURB_BLA)
        return refuse("MC_PRECISION_PERTURB_BLA is not supported: a skip does not visit its iterations", MC_ERR_UNSUPPORTED);
    if (p->precision == MC_PRECISION_PERTURB_BLA_DEEP)
        return refuse("MC_PRECISION_PERTURB_BLA_DEEP is not supported: a skip does not visit its iterations", MC_ERR_UNSUPPORTED);
    const AtomOut o = {(uint32_t*)d_period, (double*)d_amin};
    if (p->precision == MC_PRECISION_PERTURB) return perturb_atom_launch(ctx, p, d_iters, o, s);
    if (p->precision != MC_PRECISION_F32 && p->precision != MC_PRECISION_F64) return refuse("unknown precision", MC_ERR_INVALID_ARGUMENT);
    if (int rc = ensure_c_table(ctx, p, s)) return rc;
    MandelArgs a;
    dim3 grid;
    SampleList l{};
    if (int rc = launch_geometry(p, nullptr, d_iters, false, nullptr, &a, &grid, &l)) return rc;
    a.c_tab = (const float*)ctx->ctab.ptr;
    a.cx_hi = p->centre_x_hi; a.cx_lo = p->centre_x_lo; a.cy_hi = p->centre_y_hi; a.cy_lo = p->centre_y_lo;
    a.sx_hi = p->scale_x_hi; a.sx_lo = p->scale_x_lo; a.sy_hi = p->scale_y_hi; a.sy_lo = p->scale_y_lo;
    a.lut = nullptr;
    const int rc = p->precision == MC_PRECISION_F64 ? launch_atom<StateF64>(a, grid, s, o) : launch_atom<StateF32<false>>(a, grid, s, o);
    if (rc) return rc;
    return ctx->note_launch(s);
}

}  // namespace mc
