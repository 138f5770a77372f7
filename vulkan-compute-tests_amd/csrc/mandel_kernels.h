// The lane mappings of the Mandelbrot render kernels, written once for every per-pixel state machine: StateF32<FMA>,
// StateDS, StateF64 (mandelbrot.hip), StatePerturb (mandel_perturb.hip) and StateDeep (mandel_perturb_deep.hip), and the host dispatch
// that picks a mapping from a request — also for the two BLA units, whose loops are not states: each is one kernel body over the mapping
// policies below, and hands the dispatch its four instantiations.
//
// A state names its kernel arguments (Args), its block length (kBlock: the U its kernels are instantiated with) and where the smooth
// kernels read its c (kEscapeCBeforeLoop).  target_of(args) is the target block the mappings address: the struct itself for MandelArgs
// (mandelbrot.hip's overload), the member t of the perturbation argument structs.
//
// A NEW MAPPING is one kernel template, one policy and one line of MappingKernels / launch_mapping here (and one more instantiation in
// each BLA unit's table);
// a NEW ENGINE is a state with these three members in its own translation unit and one launch_state<State> call.
#pragma once
#include "mandel_adaptive.h"
#include "mandel_adaptive_smooth.h"
#include "mandel_atom.h"
#include "mandel_block_audit.h"
#include "mandel_escape.h"
#include "mandel_perturb.h"
#include "mandel_smooth.h"
#include "mandel_target.h"
#include "mc_internal.h"

namespace mc {

#ifdef __HIPCC__
template <class Args>
__host__ __device__ __forceinline__ const MandelTarget& target_of(const Args& a) { return a.t; }

// The q plane as a kernel parameter.  The qualifier is part of the listings: without it the smooth tile kernels allocate other registers.
using SmoothPlane = uint32_t* __restrict__;

// (An unnamed namespace in a header, on purpose: every instantiation is over a state that is private to the including unit, and the
// kernels and their launchers are as private as the per-unit kernels they replace.)
namespace {

// The prefetching states (StatePerturb, StateDeep) fetch exactly kBlock orbit entries per fast block; every state is launched with its own.
template <class State, int U>
__device__ __forceinline__ constexpr void require_block_length() {
    static_assert(U == State::kBlock, "a state's kernels run blocks of its own length kBlock");
}

// tile: workgroup = one wave = one 8x8 pixel tile, lane = (lx, ly) inside the tile.  Tiles finish anywhere between 1 and max_iter
// iterations apart, so the unit the hardware schedules is the tile itself: a 4-wave block would keep its place on the CU until its
// slowest tile is through (K1: 0.208 -> 0.200 ms).
template <class State, int U>
__global__ void __launch_bounds__(64) mandelbrot_kernel(typename State::Args a) {
    require_block_length<State, U>();
    const auto& t = target_of(a);
    const TileLane ln = tile_lane(t);
    State st;
    st.init(ln.valid ? ln.gx : 0u, ln.valid ? ln.gy : 0u, a);
    tile_store(t, ln, escape_time<State, U>(st, t.max_iter, ln.valid));
}

// list: the list mapping of mandel_adaptive.h.  `a` describes the sample grid, a lane is one sample of a refined pixel, and the pixel's
// colour is resolved between the lanes (no count leaves the kernel).
template <class State, int U>
__global__ void __launch_bounds__(64) mandelbrot_list_kernel(typename State::Args a, SampleList l) {
    require_block_length<State, U>();
    const auto& t = target_of(a);
    const SampleLane ln = sample_lane(l);
    State st;
    st.init(ln.valid ? ln.gx : 0u, ln.valid ? ln.gy : 0u, a);
    const uint32_t n = escape_time<State, U>(st, t.max_iter, ln.valid);
    sample_resolve(l, ln, n, t.max_iter);
}

// smooth tile (MC_MANDEL_COLOUR_SMOOTH, mandel_smooth.h): the tile kernel's loop with the z of each lane's first escape latched, then the
// shared epilogue — c as the state holds it, the fp64 continuation to radius 256, q and the interpolated colour.
// ORDER: a state whose c sits in registers all along (kEscapeCBeforeLoop) converts it before the loop, whose registers are free again
// after it; StatePerturb and StateDeep load Z_1 for it and do so after the loop.  Moving the call, or only the declaration of cx and cy,
// to the other side of the loop moves instructions: hence two ordered blocks, not one body with two conditional calls.
template <class State, int U>
__global__ void __launch_bounds__(64) mandelbrot_smooth_kernel(typename State::Args a, SmoothPlane out_smooth) {
    require_block_length<State, U>();
    const auto& t = target_of(a);
    const TileLane ln = tile_lane(t);
    State st;
    st.init(ln.valid ? ln.gx : 0u, ln.valid ? ln.gy : 0u, a);
    if constexpr (State::kEscapeCBeforeLoop) {
        double cx, cy;
        st.escape_c(cx, cy);
        EscapeCapture cap;
        const uint32_t n = escape_time<State, U, EscapeCapture>(st, t.max_iter, ln.valid, &cap);
        smooth_tile_store(t, ln, out_smooth, n, n, cap.zx, cap.zy, cx, cy);
    } else {
        EscapeCapture cap;
        const uint32_t n = escape_time<State, U, EscapeCapture>(st, t.max_iter, ln.valid, &cap);
        double cx, cy;
        st.escape_c(cx, cy);
        smooth_tile_store(t, ln, out_smooth, n, n, cap.zx, cap.zy, cx, cy);
    }
}

// smooth list (MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE, mandel_adaptive_smooth.h): the smooth kernel's lane under the list mapping.  A lane
// is one smooth sample of a refined pixel; its q never leaves the kernel, the pixel's colour is resolved between the lanes.
template <class State, int U>
__global__ void __launch_bounds__(64) mandelbrot_list_smooth_kernel(typename State::Args a, SmoothSampleList l) {
    require_block_length<State, U>();
    const auto& t = target_of(a);
    const SampleLane ln = sample_lane(l.l);
    State st;
    st.init(ln.valid ? ln.gx : 0u, ln.valid ? ln.gy : 0u, a);
    if constexpr (State::kEscapeCBeforeLoop) {
        double cx, cy;
        st.escape_c(cx, cy);
        EscapeCapture cap;
        const uint32_t n = escape_time<State, U, EscapeCapture>(st, t.max_iter, ln.valid, &cap);
        smooth_sample_resolve(l, ln, smooth::smooth_count(n, t.max_iter, cap.zx, cap.zy, cx, cy), t.max_iter);
    } else {
        EscapeCapture cap;
        const uint32_t n = escape_time<State, U, EscapeCapture>(st, t.max_iter, ln.valid, &cap);
        double cx, cy;
        st.escape_c(cx, cy);
        smooth_sample_resolve(l, ln, smooth::smooth_count(n, t.max_iter, cap.zx, cap.zy, cx, cy), t.max_iter);
    }
}

// The per-lane audit of the fast block (mandel_block_audit.h) under the tile mapping: one thread per pixel and nothing shared between
// them; four words per pixel, tile-local.
template <class State, int U, bool Sabotage>
__global__ void __launch_bounds__(64) mandelbrot_block_audit_kernel(typename State::Args a, uint32_t* __restrict__ out) {
    require_block_length<State, U>();
    const auto& t = target_of(a);
    const TileLane ln = tile_lane(t);
    if (!ln.valid) return;
    State st;
    st.init(ln.gx, ln.gy, a);
    block_audit<State, U, Sabotage>(st, t.max_iter, out + 4u * ((size_t)ln.ty * t.W + ln.gx));
}

// The same audit over a caller's lanes: lane k reads table[k] and table[W + k] (W = the number of lanes), four words per lane.
template <class State, int U, bool Sabotage>
__global__ void __launch_bounds__(64) mandelbrot_lane_audit_kernel(typename State::Args a, uint32_t* __restrict__ out) {
    require_block_length<State, U>();
    const auto& t = target_of(a);
    const uint32_t k = blockIdx.x * 64u + threadIdx.x;
    if (k >= t.W) return;
    State st;
    st.init(k, k, a);
    block_audit<State, U, Sabotage>(st, t.max_iter, out + 4u * (size_t)k);
}

// ---- the four mappings as policies, for a kernel that is ONE body over its mapping (the BLA units) ---------------------------------
// lane(t, extra...) is the lane's sample, store(t, ln, extra..., n, shown[, ezx, ezy, cx, cy]) its result: shown is the count the planes
// get (n, or the trip count under MC_MANDEL_BLA_COUNT_TRIPS), the smooth count is always of n.
struct MapTile {
    static constexpr bool kSmooth = false;
    static __device__ __forceinline__ TileLane lane(const MandelTarget& t) { return tile_lane(t); }
    static __device__ __forceinline__ void store(const MandelTarget& t, const TileLane& ln, uint32_t, uint32_t shown) { tile_store(t, ln, shown); }
};
struct MapList {
    static constexpr bool kSmooth = false;
    static __device__ __forceinline__ SampleLane lane(const MandelTarget&, const SampleList& l) { return sample_lane(l); }
    static __device__ __forceinline__ void store(const MandelTarget& t, const SampleLane& ln, const SampleList& l, uint32_t, uint32_t shown) {
        sample_resolve(l, ln, shown, t.max_iter);
    }
};
struct MapSmoothTile {
    static constexpr bool kSmooth = true;
    static __device__ __forceinline__ TileLane lane(const MandelTarget& t, SmoothPlane) { return tile_lane(t); }
    static __device__ __forceinline__ void store(const MandelTarget& t, const TileLane& ln, SmoothPlane q, uint32_t n, uint32_t shown,
                                                 double ezx, double ezy, double cx, double cy) {
        smooth_tile_store(t, ln, q, n, shown, ezx, ezy, cx, cy);
    }
};
struct MapSmoothList {
    static constexpr bool kSmooth = true;
    static __device__ __forceinline__ SampleLane lane(const MandelTarget&, const SmoothSampleList& l) { return sample_lane(l.l); }
    static __device__ __forceinline__ void store(const MandelTarget& t, const SampleLane& ln, const SmoothSampleList& l, uint32_t n, uint32_t,
                                                 double ezx, double ezy, double cx, double cy) {
        smooth_sample_resolve(l, ln, smooth::smooth_count(n, t.max_iter, ezx, ezy, cx, cy), t.max_iter);
    }
};

// ---- host: from a request to its mapping --------------------------------------------------------------------------------------------
// The four render kernels of one engine.  A null smooth pair is an engine without smooth colouring (StateF32<true>: the callers refuse
// the request before it gets here).
template <class Args>
struct MappingKernels {
    void (*tile)(Args);
    void (*list)(Args, SampleList);
    void (*smooth)(Args, uint32_t*);
    void (*list_smooth)(Args, SmoothSampleList);
};

// slist: the smooth list render; list: the list render; smooth.on: the smooth tile render into smooth.q; none: the tile render.
template <class Args>
int launch_mapping(const MappingKernels<Args>& k, const Args& a, dim3 grid, hipStream_t s, const SampleList* list, SmoothOut smooth,
                   const SmoothSampleList* slist) {
    const dim3 block(64);
    if ((slist && !k.list_smooth) || (!slist && !list && smooth.on && !k.smooth)) return MC_ERR_INVALID_ARGUMENT;
    if (slist) hipLaunchKernelGGL(k.list_smooth, grid, block, 0, s, a, *slist);
    else if (list) hipLaunchKernelGGL(k.list, grid, block, 0, s, a, *list);
    else if (smooth.on) hipLaunchKernelGGL(k.smooth, grid, block, 0, s, a, smooth.q);
    else hipLaunchKernelGGL(k.tile, grid, block, 0, s, a);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

template <class State, bool Smooth = true>
int launch_state(const typename State::Args& a, dim3 grid, hipStream_t s, const SampleList* list, SmoothOut smooth,
                 const SmoothSampleList* slist) {
    constexpr int U = State::kBlock;
    MappingKernels<typename State::Args> k = {mandelbrot_kernel<State, U>, mandelbrot_list_kernel<State, U>, nullptr, nullptr};
    if constexpr (Smooth) {
        k.smooth = mandelbrot_smooth_kernel<State, U>;
        k.list_smooth = mandelbrot_list_smooth_kernel<State, U>;
    }
    return launch_mapping(k, a, grid, s, list, smooth, slist);
}

// The two audits (LaneMapped: over a caller's lanes); sabotage: the instantiation that takes needs_exact as false (mandel_block_audit.h).
template <class State, bool LaneMapped>
int launch_block_audit(const typename State::Args& a, dim3 grid, hipStream_t s, bool sabotage, uint32_t* d_out) {
    constexpr int U = State::kBlock;
    void (*k)(typename State::Args, uint32_t*);
    if constexpr (LaneMapped) k = sabotage ? mandelbrot_lane_audit_kernel<State, U, true> : mandelbrot_lane_audit_kernel<State, U, false>;
    else k = sabotage ? mandelbrot_block_audit_kernel<State, U, true> : mandelbrot_block_audit_kernel<State, U, false>;
    hipLaunchKernelGGL(k, grid, dim3(64), 0, s, a, d_out);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

// atom (mc_mandelbrot_render_atom, mandel_atom.h): the tile kernel's lane with the state's exact steps only and the (period, amin) capture
// latched after each; n goes where the tile kernel puts it (out_iters alone: no flag is accepted), period and amin into their own planes.
// Whole images only, so the tile-local row is the storage row.  Vector stores, no atomics.
template <class State, int U>
__global__ void __launch_bounds__(64) mandelbrot_atom_kernel(typename State::Args a, AtomOut o) {
    require_block_length<State, U>();
    const auto& t = target_of(a);
    const TileLane ln = tile_lane(t);
    ExactSteps<State> st;
    st.init(ln.valid ? ln.gx : 0u, ln.valid ? ln.gy : 0u, a);
    AtomCapture cap;
    const uint32_t n = escape_time<ExactSteps<State>, U, AtomCapture>(st, t.max_iter, ln.valid, &cap);
    tile_store(t, ln, n);
    if (ln.valid) {
        const size_t idx = (size_t)ln.ty * t.W + ln.gx;
        if (o.period) o.period[idx] = cap.period;
        if (o.amin) o.amin[idx] = cap.best;
    }
}

template <class State>
int launch_atom(const typename State::Args& a, dim3 grid, hipStream_t s, const AtomOut& o) {
    hipLaunchKernelGGL((mandelbrot_atom_kernel<State, State::kBlock>), grid, dim3(64), 0, s, a, o);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

}  // namespace
#endif

}  // namespace mc
