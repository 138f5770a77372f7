// The per-lane audit of the escape-time loop's fast block (mandel_escape.h): test infrastructure, reached only through
// libmc_compute_test.so (mc_hook_mandel_block_audit, mc_hook_mandel_perturb_block_audit).
//
// escape_time accepts a fast block's result when no unfinished lane of the wave raises needs_exact.  Each State promises, PER LANE:
// needs_exact(acc) false => no iteration of the block escaped, and the state words after U advance_fast() calls equal the words after
// U step() calls, bit for bit.  A wave hides a lane that breaks the promise whenever a neighbour raises the flag in the same block (both
// are then replayed exactly).  block_audit runs ONE lane with no ballot and no cross-lane operation: every block is stepped exactly, and
// every block the kernel could run fast (i != 0) is also run fast from the saved state and compared.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mc {

constexpr uint32_t kAuditNoBadBlock = 0xffffffffu;

// bit-pattern equality: +0 / -0 and NaN payloads count as different
__device__ __forceinline__ bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }
__device__ __forceinline__ bool same_bits(double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b); }

// st: the lane's state after init().  out[0] = n as escape_time returns it; out[1] = the blocks whose fast result would be accepted
// (needs_exact false), out[2] = the blocks that raised it; out[3] = i of the first accepted block that broke the promise (a step of
// it escaped, or the state words differ), kAuditNoBadBlock if none.  Sabotage: needs_exact is taken as false for every block — nothing
// else changes (the lane always continues from the exactly stepped state), so out[3] then shows what the filter is there to catch.
template <class State, int U, bool Sabotage>
__device__ __forceinline__ void block_audit(State& st, uint32_t max_iter, uint32_t* __restrict__ out) {
    uint32_t n = max_iter, accepted = 0u, raised = 0u, first_bad = kAuditNoBadBlock;
    uint32_t i = 0;
    bool escaped = false;
    for (; i + U <= max_iter; i += U) {
        const State saved = st;
        int first = -1;   // the first step of this block that escaped
#pragma unroll
        for (int k = 0; k < U; k++) {
            const bool e = st.step();
            if (e && first < 0) first = k;
        }
        if (State::kHasFastBlock && i != 0) {   // the kernel never runs a fast block at i == 0
            State probe = saved;
            typename State::Acc acc = saved.acc_init();
#pragma unroll
            for (int k = 0; k < U; k++) probe.advance_fast(acc);
            const bool raise = Sabotage ? false : State::needs_exact(acc);
            if (raise) {
                raised++;
            } else {
                accepted++;
                if ((first >= 0 || !probe.bits_equal(st)) && first_bad == kAuditNoBadBlock) first_bad = i;
            }
        }
        if (first >= 0) {
            n = i + (uint32_t)first;
            escaped = true;
            break;
        }
    }
    if (!escaped) {
        for (; i < max_iter; i++) {   // tail: max_iter % U iterations, exact steps only
            if (st.step()) {
                n = i;
                break;
            }
        }
    }
    out[0] = n;
    out[1] = accepted;
    out[2] = raised;
    out[3] = first_bad;
}

}  // namespace mc
