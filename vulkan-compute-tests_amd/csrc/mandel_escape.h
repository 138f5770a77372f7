// The escape-time loop shared by the Mandelbrot kernels of mandelbrot.hip (F32, DS, F64) and mandel_perturb.hip (PERTURB):
// per-lane state machines run in blocks of U iterations, escapes are wave ballots.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mc {

// Runs the escape-time loop for the 64 pixels of a wave.  Returns n in [0,max_iter] per lane:
// the number of iterations that did not escape (mandelbrot.comp:40-46).
//
// CONVERGED TILES (north_star: "wavefront ballot/any for early-out on converged Mandelbrot tiles").  The iteration is a
// deterministic map of the state z (c is fixed per lane; sx, sy are functions of z), so an orbit that returns to a value it
// has held before repeats that stretch for ever.  If lane L has not escaped up to iteration i and z_i == z_j for an earlier
// j (compared as VALUES: +0 and -0 are interchangeable operands of +, -, x and of the comparison, and a NaN never compares
// equal), no iteration of the cycle j..i escaped, so none ever will: the shader's loop would run to max_iter and leave
// n = max_iter — exactly what this lane returns.  Brent's scheme at block granularity: a reference state is kept per lane,
// compared with the state at the end of a block of U iterations (fp32: 2 compares per 8 iterations) and replaced when the
// number of comparisons made reaches 1, 2, 4, 8, ...  A wave leaves as soon as every lane has escaped or is known to cycle:
// at K1 that is 91 % of the interior pixels (median: iteration 88 of 1000), 2.44x fewer issued instructions and
// 0.38 -> 0.21 ms; the iteration plane is bit-identical (tests, fuzz).  fp32 orbits inside the set collapse
// onto a short exact cycle near their attractor; the two-float orbits of a deep zoom rarely do (checked every 16 iterations).
// A State with kCycleCheckBlocks == 0 has no cycle exit: its lanes run until they escape or max_iter is reached.
//
// The State interface: init (per kernel), step() = one exact iteration, reporting "escaped now"; kHasFastBlock, Acc, acc_init(),
// advance_fast(acc) and needs_exact(acc) = the block of U iterations without per-iteration ballots, replayed exactly from the saved
// state when some unfinished lane raises needs_exact; same_z() and kCycleCheckBlocks = the cycle exit.
//
// Cap: NoCapture, or a type whose latch(escaped, st) is called after every EXACT step (EscapeCapture of mandel_smooth.h keeps the z of
// the lane's first escape).  An unfinished lane's escape is only ever detected in an exact step: a fast block in which one may have
// escaped is replayed.  With NoCapture the loop is the one it was.
struct NoCapture {};
template <class State, int U, class Cap = NoCapture>
__device__ __forceinline__ uint32_t escape_time(State& st, uint32_t max_iter, bool valid, [[maybe_unused]] Cap* cap = nullptr) {
    constexpr bool kCapture = !__is_same(Cap, NoCapture);
    const uint32_t lane = __lane_id();
    const uint64_t lanebit = 1ull << lane;
    uint64_t done = ~__ballot(valid);   // lanes outside the image never hold the wave
    uint32_t n = max_iter;
    uint32_t i = 0;
    [[maybe_unused]] State ref = st;    // Brent reference state (z_0 = 0: a cycle through the origin is caught too)
    [[maybe_unused]] uint32_t checks = 0;   // comparisons made so far (wave-uniform)
    for (; i + U <= max_iter; i += U) {
        if constexpr (State::kCycleCheckBlocks != 0u) {   // 0: no cycle exit (a state that never repeats: StatePerturb)
            if (i != 0 && (i / (uint32_t)U) % State::kCycleCheckBlocks == 0u) {
                // cycling lanes are finished with n = max_iter (their state stays on the cycle: harmless to keep iterating)
                done |= __ballot(st.same_z(ref));
                if (done == ~0ull) return n;
                checks++;
                if ((checks & (checks - 1u)) == 0u) ref = st;   // wave-uniform: at 1, 2, 4, 8, ... comparisons
            }
        }
        if (State::kHasFastBlock && i != 0) {   // the first block is evaluated exactly: most tiles escape right there
            // fast path: U iterations without per-iteration compares/ballots, ONE test per block; the exact
            // per-iteration ballots below are evaluated (from the saved state) only if some unfinished lane may
            // have escaped (or, two-float state, may have left the fast arithmetic's precondition)
            State probe = st;
            typename State::Acc acc = st.acc_init();
#pragma unroll
            for (int k = 0; k < U; k++) probe.advance_fast(acc);
            if ((__ballot(State::needs_exact(acc)) & ~done) == 0ull) {
                st = probe;
                continue;
            }
        }
        uint64_t b[U];
        uint64_t any = 0;
#pragma unroll
        for (int k = 0; k < U; k++) {
            if constexpr (kCapture) {
                const bool e = st.step();
                cap->latch(e, st);
                b[k] = __ballot(e);
            } else {
                b[k] = __ballot(st.step());
            }
            any |= b[k];
        }
        uint64_t newly = any & ~done;
        if (newly) {   // wave-uniform: some lane escaped for the first time in this block
#pragma unroll
            for (int k = U - 1; k >= 0; k--)
                if (b[k] & ~done & lanebit) n = i + k;
            done |= any;
            if (done == ~0ull) return n;
        }
    }
    for (; i < max_iter; i++) {   // tail: max_iter % U iterations
        uint64_t b;
        if constexpr (kCapture) {
            const bool e = st.step();
            cap->latch(e, st);
            b = __ballot(e);
        } else {
            b = __ballot(st.step());
        }
        uint64_t newly = b & ~done;
        if (newly) {
            if (newly & lanebit) n = i;
            done |= b;
            if (done == ~0ull) return n;
        }
    }
    return n;
}

}  // namespace mc
