// MC_PRECISION_PERTURB: Mandelbrot deep zooms past fp64 by perturbation (include/mc_compute.h states the contract).
//
//  * the reference orbit Z_0 .. Z_L is the host's (mandel_orbit.cpp); here it is bound to a context as a double2 table.
//  * device: StatePerturb inside the escape-time loop of mandel_escape.h.  Each pixel iterates its offset d from the orbit in IEEE
//    double, rebasing onto Z_0 when |z| < |d| or the orbit ends (Zhuoran's rebasing: no glitch detection, no second reference).
//    The orbit is read from HBM (L2-resident: 800 KB at M = 50 000); the fast block fetches the block's U entries at its start, so
//    no load sits on the iteration's dependency chain, and a block in which an unfinished lane rebases is replayed exactly.
//  * IEEE double in source order: this TU is built with -ffp-contract=off like every other; fp64 denormals stay enabled.
#include <atomic>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "mandel_bla_table.h"
#include "mandel_kernels.h"
#include "mandel_perturb.h"
#include "mandel_side_record.h"
#include "mc_internal.h"

namespace mc {

namespace {

// The orbit bound to each context (a side record: mandel_side_record.h).
struct Binding {
    DeviceBuffer orbit;                // Z_0 .. Z_L, double2
    uint32_t length = 0, max_iter = 0;
    double scale_x = 0.0, scale_y = 0.0;   // a deep orbit: the mantissas
    int32_t scale_exp2 = 0;
    bool deep = false;                 // rendered by the deep kernel (mandel_perturb_deep.hip)
    bool has_zero = false;             // some Z_j = 0 exactly, 1 <= j < L
    uint32_t generation = 0;           // a new value per bind, part of the dc table's cache key
    // MC_PRECISION_PERTURB_BLA: the orbit's BLA table when it had one at the bind (mc_mandelbrot_orbit_bla), or the one the bind built
    // on the device (mc_context_bind_mandelbrot_orbit_tables).  The per-level offsets
    // follow from L (mandel_perturb.h); levels / entries are its shape.  An orbit without a table leaves bla unallocated.
    DeviceBuffer bla;
    uint32_t bla_levels = 0;
    uint64_t bla_entries = 0;
    bool has_bla = false;
    // MC_PRECISION_PERTURB_BLA_DEEP: the orbit's floatexp table when it had one at the bind (mc_mandelbrot_orbit_bla_deep), likewise
    DeviceBuffer bla_deep;
    uint32_t bla_deep_levels = 0;
    uint64_t bla_deep_entries = 0;
    bool has_bla_deep = false;
};
SideRecords<Binding> g_bindings;
std::atomic<uint32_t> g_generation{0};

struct PerturbArgs {
    MandelTarget t;   // t.table: [dcx[W] | dcy[H]], the pixel's offset from c_ref per column / per row
};

// One pixel's offset from the reference orbit (the loop of include/mc_compute.h, MC_PRECISION_PERTURB).  Per iteration 20 fp64 ops
// (2 + 2 for a, 4 + 4 for the new offset, 2 for z, 3 for |z|^2, 3 for |d|^2) against F64's 8.
struct StatePerturb {
    using Args = PerturbArgs;
    static constexpr int kBlock = 8;        // the escape-time block length U: the fast block prefetches this many orbit entries
    static constexpr bool kEscapeCBeforeLoop = false;   // c needs a load of Z_1: the smooth kernels form it after the loop
    const double2* __restrict__ Z;
    uint32_t L;
    double dcx, dcy, dx, dy, zmx, zmy;      // zm = Z[m]
    uint32_t m;
    __device__ __forceinline__ void init(uint32_t gx, uint32_t gy, const PerturbArgs& a) {
        Z = a.t.orbit;
        L = a.t.L;
        dcx = a.t.table[gx];
        dcy = a.t.table[a.t.W + gy];
        dx = dy = zmx = zmy = 0.0;
        m = 0;
    }
    // the iteration up to the new z; returns r = |z|^2, leaves the new offset in ndx, ndy and z in zx, zy
    __device__ __forceinline__ double advance(double2 z1, double& ndx, double& ndy, double& zx, double& zy) const {
        const double ax = (zmx + zmx) + dx, ay = (zmy + zmy) + dy;
        ndx = ((ax * dx) - (ay * dy)) + dcx;
        ndy = ((ax * dy) + (ay * dx)) + dcy;
        zx = z1.x + ndx;
        zy = z1.y + ndy;
        return (zx * zx) + (zy * zy);
    }
    // Exact iteration.  A lane that has escaped keeps iterating until its wave is done (its state no longer matters), and a lane past
    // a fast block it took as finished may hold m > L: the load index is clamped so that no lane reads beyond Z_L.
    __device__ __forceinline__ bool step() {
        m = m + 1u;
        const double2 z1 = Z[m < L ? m : L];
        double ndx, ndy, zx, zy;
        const double r = advance(z1, ndx, ndy, zx, zy);
        if (m == L || r < ((ndx * ndx) + (ndy * ndy))) { dx = zx; dy = zy; m = 0; zmx = zmy = 0.0; }   // rebase: Z_0 = 0
        else { dx = ndx; dy = ndy; zmx = z1.x; zmy = z1.y; }
        return r > 2.0;
    }
    // MC_MANDEL_COLOUR_SMOOTH: the z the last step() tested.  After a rebase it is d itself (Z_0 = 0 is not added: a -0 stays -0); otherwise
    // Z[m] + d, the very addition step() made.  c = Z_1 + dc (Z_1 is c_ref correctly rounded).
    __device__ __forceinline__ void escape_z(double& x, double& y) const {
        x = m == 0u ? dx : zmx + dx;
        y = m == 0u ? dy : zmy + dy;
    }
    __device__ __forceinline__ void escape_c(double& x, double& y) const {
        const double2 z1 = Z[1];
        x = z1.x + dcx;
        y = z1.y + dcy;
    }
    // Fast block: Z[m+1 .. m+U] are loaded at the block's start (acc_init), off the dependency chain; the block assumes m advances by
    // one per iteration.  needs_exact = F64's high-word escape filter OR "this lane rebased, or reached m == L, in the block": any
    // unfinished lane raising it replays the block exactly from the saved state (step(), one load per iteration).
    static constexpr bool kHasFastBlock = true;
    static constexpr uint32_t kCycleCheckBlocks = 0;   // no cycle exit: the state includes m and never repeats
    struct Acc {
        uint32_t hi;        // OR of the high words of |z|^2
        bool rebase;        // some iteration rebased or reached the orbit's end
        double2 z[kBlock];  // Z[m+1 ..], consumed one per iteration
    };
    __device__ __forceinline__ Acc acc_init() const {
        Acc acc;
        acc.hi = 0u;
        acc.rebase = L - m <= (uint32_t)kBlock;   // m + k == L for some k in [1, U]  (m <= L)
#pragma unroll
        for (int k = 0; k < kBlock; k++) {
            const uint32_t j = m + 1u + (uint32_t)k;
            acc.z[k] = Z[j < L ? j : L];
        }
        return acc;
    }
    __device__ __forceinline__ void advance_fast(Acc& acc) {
        const double2 z1 = acc.z[0];
#pragma unroll
        for (int k = 0; k + 1 < kBlock; k++) acc.z[k] = acc.z[k + 1];   // register renaming once unrolled
        double ndx, ndy, zx, zy;
        const double r = advance(z1, ndx, ndy, zx, zy);
        acc.hi |= (uint32_t)((uint64_t)__double_as_longlong(r) >> 32);
        acc.rebase |= r < ((ndx * ndx) + (ndy * ndy));
        dx = ndx; dy = ndy; zmx = z1.x; zmy = z1.y;
        m = m + 1u;
    }
    static __device__ __forceinline__ bool needs_exact(const Acc& acc) { return acc.hi > 0x3fffffffu || acc.rebase; }
    // every word the state iterates on, by bit pattern (mandel_block_audit.h)
    __device__ __forceinline__ bool bits_equal(const StatePerturb& o) const {
        return Z == o.Z && L == o.L && m == o.m && same_bits(dcx, o.dcx) && same_bits(dcy, o.dcy) && same_bits(dx, o.dx) &&
               same_bits(dy, o.dy) && same_bits(zmx, o.zmx) && same_bits(zmy, o.zmy);
    }
};

// dcx[g] = ((double)g / (double)W - 0.5) * sx, dcy likewise: F64's c table without the centre.  In the context's c-table slot, keyed
// by (W, H, precision, the bind generation): the params' view words are all zero for this precision.
int ensure_dc_table(mc_context* ctx, const mc_mandelbrot_params* p, const Binding& b, hipStream_t s) {
    float gen;
    std::memcpy(&gen, &b.generation, sizeof gen);   // compared bytewise
    std::vector<float> key = {(float)p->width, (float)p->height, (float)p->precision, gen};
    if (ctx->ctab.ptr && ctx->ctab_key.size() == key.size() &&
        std::memcmp(ctx->ctab_key.data(), key.data(), key.size() * sizeof(float)) == 0)
        return MC_OK;
    const uint32_t W = p->width, H = p->height;
    std::vector<double> tab((size_t)W + H);
    for (uint32_t g = 0; g < W; g++) tab[g] = ((double)g / (double)W - 0.5) * b.scale_x;
    for (uint32_t g = 0; g < H; g++) tab[W + g] = ((double)g / (double)H - 0.5) * b.scale_y;
    int rc = ctx->drain_launch_streams();   // an earlier launch of this context may still read the old table
    if (rc) return rc;
    if ((rc = ctx->ctab.reserve(tab.size() * sizeof(double)))) return rc;
    MC_HIP_TRY(hipMemcpyAsync(ctx->ctab.ptr, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, s));
    MC_HIP_TRY(hipStreamSynchronize(s));
    ctx->ctab_key = key;
    return MC_OK;
}

}  // namespace

int perturb_launch(mc_context* ctx, const mc_mandelbrot_params* p, void* d_rgba, void* d_iters, hipStream_t s, bool warm,
                   const SampleList* list, void* d_smooth, const SmoothSampleList* slist) {
    const SmoothOut smooth = {(p->flags & MC_MANDEL_COLOUR_SMOOTH) != 0u && !list && !slist, (uint32_t*)d_smooth};
    const bool bla = p->precision == MC_PRECISION_PERTURB_BLA;
    const bool bla_deep = p->precision == MC_PRECISION_PERTURB_BLA_DEEP;
    const std::string name = bla ? "MC_PRECISION_PERTURB_BLA" : bla_deep ? "MC_PRECISION_PERTURB_BLA_DEEP" : "MC_PRECISION_PERTURB";
    const Binding* b = g_bindings.find(ctx);
    if (!b || !b->orbit.ptr || !b->length) {
        set_error_detail(name + ": no orbit bound to the context (mc_context_bind_mandelbrot_orbit)");
        return MC_ERR_INVALID_ARGUMENT;
    }
    const float words[8] = {p->centre_x_hi, p->centre_x_lo, p->centre_y_hi, p->centre_y_lo,
                            p->scale_x_hi, p->scale_x_lo, p->scale_y_hi, p->scale_y_lo};
    for (float w : words)
        if (w != 0.0f) {
            set_error_detail(name + ": the view is the bound orbit's; the params' eight view words must be zero");
            return MC_ERR_INVALID_ARGUMENT;
        }
    if (p->max_iter > b->max_iter) {
        set_error_detail(name + ": max_iter above the bound orbit's");
        return MC_ERR_INVALID_ARGUMENT;
    }
    MandelTarget t;
    dim3 grid;
    SampleList l{};
    if (int rc = launch_geometry(p, d_rgba, d_iters, warm, slist ? &slist->l : list, &t, &grid, &l)) return rc;   // mandel_target.h
    if (list) list = &l;
    const SmoothSampleList sl = {l, slist ? slist->pairs : nullptr};
    if (slist) slist = &sl;
    if (bla && b->deep) {
        set_error_detail(name + ": the bound orbit is deep (min |scale| < 2^-960); BLA covers the plain loop only");
        return MC_ERR_UNSUPPORTED;
    }
    if (bla && !b->has_bla) {
        set_error_detail(name + ": the bound orbit has no BLA table (mc_mandelbrot_orbit_bla before mc_context_bind_mandelbrot_orbit)");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (bla_deep && !b->has_bla_deep) {
        set_error_detail(name + ": the bound orbit has no deep BLA table (mc_mandelbrot_orbit_bla_deep before "
                                "mc_context_bind_mandelbrot_orbit)");
        return MC_ERR_INVALID_ARGUMENT;
    }
    const void* lut = nullptr;
    int rc;
    if ((d_rgba || warm) && (rc = mandelbrot_lut_device(ctx, p, s, &lut))) return rc;
    if ((rc = ensure_dc_table(ctx, p, *b, s))) return rc;
    t.L = b->length;
    t.lut = t.out_rgba ? (const float4*)lut : nullptr;
    t.table = (const double*)ctx->ctab.ptr;
    t.orbit = (const double2*)b->orbit.ptr;
    if (bla) {   // mandel_perturb_bla.hip
        const PerturbBlaArgs d = {t, b->bla_entries ? (const double*)b->bla.ptr : nullptr,
                                  (p->flags & MC_MANDEL_BLA_COUNT_TRIPS) ? 1u : 0u};
        if ((rc = perturb_bla_launch(d, grid, s, list, smooth, slist))) return rc;
        return ctx->note_launch(s);
    }
    if (bla_deep) {   // mandel_perturb_bla_deep.hip
        const PerturbBlaDeepArgs d = {t, b->bla_deep_entries ? (const BlaDeepRec*)b->bla_deep.ptr : nullptr, b->scale_exp2,
                                      (p->flags & MC_MANDEL_BLA_COUNT_TRIPS) ? 1u : 0u};
        if ((rc = perturb_bla_deep_launch(d, grid, s, list, smooth, slist))) return rc;
        return ctx->note_launch(s);
    }
    if (b->deep || (p->flags & MC_MANDEL_PERTURB_FORCE_DEEP)) {   // below 2^-960 (or forced by a test): mandel_perturb_deep.hip
        const PerturbDeepArgs d = {t, b->scale_exp2, b->has_zero ? 1u : 0u};
        if ((rc = perturb_deep_launch(d, grid, s, list, smooth, slist))) return rc;
        return ctx->note_launch(s);
    }
    const PerturbArgs a = {t};
    if ((rc = launch_state<StatePerturb>(a, grid, s, list, smooth, slist))) return rc;
    return ctx->note_launch(s);
}

// mc_hook_mandel_perturb_block_audit: a caller's orbit table and per-lane offsets, both already on the device.
int perturb_block_audit_launch(const double2* d_orbit, uint32_t L, bool deep, int32_t exp2, bool has_zero, const double* d_table,
                               uint32_t n_lanes, uint32_t max_iter, bool sabotage, uint32_t* d_out, hipStream_t s) {
    if (!d_orbit || !d_table || !d_out || !L || !n_lanes || !max_iter) return MC_ERR_INVALID_ARGUMENT;
    MandelTarget t{};
    t.W = n_lanes; t.H = n_lanes; t.max_iter = max_iter; t.L = L;
    t.row_begin = 0u; t.row_end = n_lanes;
    t.table = d_table;
    t.orbit = d_orbit;
    const dim3 grid((n_lanes + 63u) / 64u);
    if (deep) return perturb_deep_block_audit_launch({t, exp2, has_zero ? 1u : 0u}, grid, sabotage, d_out, s);   // mandel_perturb_deep.hip
    return launch_block_audit<StatePerturb, true>({t}, grid, s, sabotage, d_out);
}

void perturb_release(mc_context* ctx) {
    g_bindings.erase(ctx, [](Binding& b) {
        b.orbit.release();
        b.bla.release();
        b.bla_deep.release();
    });
}

// mc_mandelbrot_render_atom, MC_PRECISION_PERTURB (mandel_atom.h): perturb_launch's checks of the binding and the view, the refusal of a
// deep orbit (its z leaves the double range), the dc table, the launch.  p is a whole image with no flag (mandelbrot_atom_launch).
int perturb_atom_launch(mc_context* ctx, const mc_mandelbrot_params* p, void* d_iters, const AtomOut& o, hipStream_t s) {
    const std::string name = "mc_mandelbrot_render_atom: MC_PRECISION_PERTURB";
    const Binding* b = g_bindings.find(ctx);
    if (!b || !b->orbit.ptr || !b->length) {
        set_error_detail(name + ": no orbit bound to the context (mc_context_bind_mandelbrot_orbit)");
        return MC_ERR_INVALID_ARGUMENT;
    }
    const float words[8] = {p->centre_x_hi, p->centre_x_lo, p->centre_y_hi, p->centre_y_lo,
                            p->scale_x_hi, p->scale_x_lo, p->scale_y_hi, p->scale_y_lo};
    for (float w : words)
        if (w != 0.0f) {
            set_error_detail(name + ": the view is the bound orbit's; the params' eight view words must be zero");
            return MC_ERR_INVALID_ARGUMENT;
        }
    if (p->max_iter > b->max_iter) {
        set_error_detail(name + ": max_iter above the bound orbit's");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (b->deep) {
        set_error_detail(name + ": the bound orbit is deep (min |scale| < 2^-960): its z leaves the double range, a floatexp amin is not built");
        return MC_ERR_UNSUPPORTED;
    }
    MandelTarget t;
    dim3 grid;
    SampleList l{};
    if (int rc = launch_geometry(p, nullptr, d_iters, false, nullptr, &t, &grid, &l)) return rc;
    if (int rc = ensure_dc_table(ctx, p, *b, s)) return rc;
    t.L = b->length;
    t.lut = nullptr;
    t.table = (const double*)ctx->ctab.ptr;
    t.orbit = (const double2*)b->orbit.ptr;
    const PerturbArgs a = {t};
    if (int rc = launch_atom<StatePerturb>(a, grid, s, o)) return rc;
    return ctx->note_launch(s);
}

bool perturb_bound_scale(mc_context* ctx, double* scale_x, double* scale_y, int32_t* scale_exp2) {
    const Binding* b = g_bindings.find(ctx);
    if (!b || !b->length) return false;
    *scale_x = b->scale_x;
    *scale_y = b->scale_y;
    *scale_exp2 = b->scale_exp2;
    return true;
}

}  // namespace mc

namespace mc {
namespace {

// mc_context_bind_mandelbrot_orbit (device_tables = 0) and mc_context_bind_mandelbrot_orbit_tables.  A table named in device_tables is
// built on the device from the Z uploaded here; any other is uploaded when the orbit holds it and released otherwise.
int bind_orbit(const char* fn, mc_context* ctx, const mc_mandelbrot_orbit* o, uint32_t device_tables) {
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    if (device_tables & ~(uint32_t)(MC_ORBIT_TABLE_BLA | MC_ORBIT_TABLE_BLA_DEEP)) {
        set_error_detail(std::string(fn) + ": unknown bits in device_tables");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (o && o->deep && (device_tables & MC_ORBIT_TABLE_BLA)) {
        set_error_detail(std::string(fn) + ": a deep orbit (min |scale| < 2^-960) renders by the rescaled loop, which has no BLA");
        return MC_ERR_UNSUPPORTED;
    }
    MC_HIP_TRY(hipSetDevice(ctx->device));
    // a running launch of this context may read the current table (or the dc table keyed by its generation): wait for the context's
    // launch streams — not the whole device — before replacing it, as the colour table does
    int rc = ctx->drain_launch_streams();
    if (rc) return rc;
    if (!o) {
        perturb_release(ctx);
        return MC_OK;
    }
    const bool dev_bla = (device_tables & MC_ORBIT_TABLE_BLA) != 0u, dev_deep = (device_tables & MC_ORBIT_TABLE_BLA_DEEP) != 0u;
    const blatab::Shape sh = blatab::shape(o->length);
    Binding* b = g_bindings.get(ctx);
    b->generation = ++g_generation;
    b->length = 0;                   // unusable until the copy below has completed
    b->has_bla = false;
    b->has_bla_deep = false;
    const size_t bytes = o->z.size() * sizeof(double);
    if ((rc = b->orbit.reserve(bytes))) return rc;
    MC_HIP_TRY(hipMemcpyAsync(b->orbit.ptr, o->z.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
    if (dev_bla && sh.total) {   // built below, in place
        if ((rc = b->bla.reserve(bla_table_bytes(MC_ORBIT_TABLE_BLA, o->length)))) return rc;
    } else if (!dev_bla && o->has_bla && !o->bla.empty()) {   // MC_PRECISION_PERTURB_BLA's table; an orbit without one binds exactly as before
        const size_t tbytes = o->bla.size() * sizeof(double);
        if ((rc = b->bla.reserve(tbytes))) return rc;
        MC_HIP_TRY(hipMemcpyAsync(b->bla.ptr, o->bla.data(), tbytes, hipMemcpyHostToDevice, ctx->stream));
    } else {
        b->bla.release();   // (a table left by an earlier bind)
    }
    if (dev_deep && sh.total) {
        if ((rc = b->bla_deep.reserve(bla_table_bytes(MC_ORBIT_TABLE_BLA_DEEP, o->length)))) return rc;
    } else if (!dev_deep && o->has_bla_deep && !o->bla_deep.empty()) {   // MC_PRECISION_PERTURB_BLA_DEEP's table, likewise
        const size_t tbytes = o->bla_deep.size() * sizeof(BlaDeepRec);
        if ((rc = b->bla_deep.reserve(tbytes))) return rc;
        MC_HIP_TRY(hipMemcpyAsync(b->bla_deep.ptr, o->bla_deep.data(), tbytes, hipMemcpyHostToDevice, ctx->stream));
    } else {
        b->bla_deep.release();
    }
    if (device_tables &&
        (rc = bla_table_build(ctx, device_tables, b->orbit.ptr, o->length, o->scale_x, o->scale_y, o->deep, o->scale_exp2, b->bla.ptr,
                              b->bla_deep.ptr, ctx->stream)))
        return rc;
    MC_HIP_TRY(hipStreamSynchronize(ctx->stream));
    b->has_bla = dev_bla || o->has_bla;
    b->bla_levels = dev_bla ? sh.levels : o->bla_levels;
    b->bla_entries = dev_bla ? sh.total : o->bla_entries;
    b->has_bla_deep = dev_deep || o->has_bla_deep;
    b->bla_deep_levels = dev_deep ? sh.levels : o->bla_deep_levels;
    b->bla_deep_entries = dev_deep ? sh.total : o->bla_deep_entries;
    b->length = o->length;
    b->max_iter = o->max_iter;
    b->scale_x = o->scale_x;
    b->scale_y = o->scale_y;
    b->scale_exp2 = o->scale_exp2;
    b->deep = o->deep;
    b->has_zero = false;
    for (uint32_t j = 1; j < o->length; j++)
        if (o->z[2 * j] == 0.0 && o->z[2 * j + 1] == 0.0) { b->has_zero = true; break; }
    return MC_OK;
}

// The binding whose table of one kind is to be read back; a refusal when nothing of the kind is bound.
int bound_table(const char* fn, mc_context* ctx, bool deep_kind, const Binding** out) {
    *out = nullptr;
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    const Binding* b = g_bindings.find(ctx);
    if (!b || !b->length || !(deep_kind ? b->has_bla_deep : b->has_bla)) {
        set_error_detail(std::string(fn) + ": no such table is bound to the context");
        return MC_ERR_INVALID_ARGUMENT;
    }
    MC_HIP_TRY(hipSetDevice(ctx->device));
    *out = b;
    return MC_OK;
}

}  // namespace
}  // namespace mc

extern "C" int mc_context_bind_mandelbrot_orbit(mc_context* ctx, const mc_mandelbrot_orbit* o) {
    return mc::bind_orbit("mc_context_bind_mandelbrot_orbit", ctx, o, 0u);
}

extern "C" int mc_context_bind_mandelbrot_orbit_tables(mc_context* ctx, const mc_mandelbrot_orbit* o, uint32_t device_tables) {
    return mc::bind_orbit("mc_context_bind_mandelbrot_orbit_tables", ctx, o, device_tables);
}

extern "C" int mc_context_bound_bla_copy(mc_context* ctx, double* out, uint32_t* levels, uint64_t* entries) {
    const mc::Binding* b;
    if (int rc = mc::bound_table("mc_context_bound_bla_copy", ctx, false, &b)) return rc;
    if (out && b->bla_entries) {
        MC_HIP_TRY(hipMemcpyAsync(out, b->bla.ptr, (size_t)b->bla_entries * mc::blatab::kPlainDoubles * sizeof(double),
                                  hipMemcpyDeviceToHost, ctx->stream));
        MC_HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    if (levels) *levels = b->bla_levels;
    if (entries) *entries = b->bla_entries;
    return MC_OK;
}

extern "C" int mc_context_bound_bla_deep_copy(mc_context* ctx, double* mant, int32_t* exps, uint32_t* levels, uint64_t* entries) {
    const mc::Binding* b;
    if (int rc = mc::bound_table("mc_context_bound_bla_deep_copy", ctx, true, &b)) return rc;
    if ((mant || exps) && b->bla_deep_entries) {
        std::vector<mc::BlaDeepRec> t;
        try {
            t.resize((size_t)b->bla_deep_entries);
        } catch (const std::bad_alloc&) {
            return MC_ERR_OUT_OF_MEMORY;
        }
        MC_HIP_TRY(hipMemcpyAsync(t.data(), b->bla_deep.ptr, t.size() * sizeof(mc::BlaDeepRec), hipMemcpyDeviceToHost, ctx->stream));
        MC_HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (size_t j = 0; j < t.size(); j++) {
            const mc::BlaDeepRec& r = t[j];
            if (mant) { mant[5 * j] = r.ax; mant[5 * j + 1] = r.ay; mant[5 * j + 2] = r.bx; mant[5 * j + 3] = r.by; mant[5 * j + 4] = r.r; }
            if (exps) { exps[3 * j] = r.ea; exps[3 * j + 1] = r.eb; exps[3 * j + 2] = r.er; }
        }
    }
    if (levels) *levels = b->bla_deep_levels;
    if (entries) *entries = b->bla_deep_entries;
    return MC_OK;
}
