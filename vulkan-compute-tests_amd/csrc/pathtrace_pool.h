// The sample-pool path tracer kernels for gfx950 — closed-box scenes (SceneArgs::box_ok); fast math (included by pathtrace_fast.hip),
// its careful tier (pathtrace_careful.hip; `Fast` is the math tier: 0 strict, 1 fast, 2 careful) and strict math (pathtrace_strict.hip).
//
// Why: the round-synchronous kernels (pathtrace_kernel.h) step all 64 lanes of a wave through the depths of ONE sample each;
// Russian roulette (pathTracer.comp:395-397) thins the wave from depth 6 on and the round still costs its longest path, so the
// intersection + prologue code runs with 52 of 64 lanes and `VALUUtilization` sits at 59 % (profiles/r02_pt_fast_pmc_summary.json).
// gfx950 issues every VALU instruction in ~2.4 cycles whatever its class or EXEC mask (profiles/r03_valu_microbench3.txt), so
// what is left is the number of lanes an issued instruction serves.
//
// What: a wave owns 64/S pixels; the S lanes of a pixel share ALL its samples as a pool.  Camera rays and their first
// intersection (:357-362, :316-341) are produced one batch — S consecutive samples of every pixel, 64 rays — at a time at full
// width into a stash in LDS (two batches deep); a lane whose path ended takes its pixel's next stash entry at the top of the
// next iteration, so lanes sit at different depths of different samples and the wave stays full until the pool runs dry.
// No path state ever moves between lanes, there are no queues between waves, no reorder ring: a lane adds the radiance it
// gathers (:391, :422) to its own register accumulator, and at the end the S partial sums of a pixel are added in lane order,
// scaled by 1/spp and :453 is applied.
// (First version: any lane took any pixel's sample and added its radiance to the pixel's accumulator in LDS with ds_add_f32.
// gfx950 executes an LDS float atomic at ~2 cycles per LANE — 131 LDS cycles per wave instruction, conflict or not — and the
// kernel became LDS-bound: 33.6 ms.  profiles/r03_pool_v1_lds_atomics_pmc.txt.)
//
// STRICT variant (Fast = 0; bit-identical to the oracle like every strict kernel): the per-pixel sum must be the reference's —
// samples added in sample order (:451-:452).  A lane therefore keeps a per-PATH accrad, writes accrad / spp into its sample's slot
// of a result ring in LDS (three batches per pixel for the reference scene, four beyond three spheres) when the path ends, and the pixel's 16 lanes add a batch's 16 results in sample
// order — the fold of the round-synchronous kernels, fed from LDS — once every sample of the batch has ended (oldest live sample
// of the pixel by a 4-step butterfly, only when a new batch is wanted).  Same decisions, same operations, same order: exact.
//
// Parity (fast): a sample follows the fast closed-box round-synchronous kernel's arithmetic (the same inlined functions) except for
// the cheaper equivalent forms this kernel alone uses — the bounce off a wall as a signed permutation (the same values), shadow rays
// decided by comparing squares and centre projections (disjoint spheres: the host's premise for selecting it), |c - x|^2 - r^2 and
// colour / p formed once — DESIGN.md §3.3; beyond that what differs is the ORDER in which a pixel's fp32 contributions are added — the
// reference adds accrad/spp sample by sample (:451-:452), here every lane sums the contributions of the samples it happened to trace and the S partial sums are added at
// the end — a reassociation, relative 1e-6 of the pixel value, far inside the fast-math tolerance; the strict variant
// above keeps the reference's order.  It is deterministic: a wave's schedule depends on nothing outside the wave, and
// the pixels a wave owns are the same for every tiling the host selects it for (pathtrace.hip).
//
// Transcendentals as prioritised groups (fast tier only).  4.9 % of the kernel's VALU instructions are hardware transcendentals and
// take a quarter of its time: among other instructions one costs a SIMD 11 - 13 cycles, directly behind another one 8.3 - 9, and with
// seven waves of equal priority interleaving none ever is behind another.  The two places of a diffuse bounce where several are
// independent of each other and of everything computed there — the light sample's 1 / |xc| with sin and cos of its angle
// (light_sample_direction<1, true>), the cosine bounce's sqrt(r2), sin, cos, sqrt(1 - r2) (bounce_trans_grouped) — issue them as ONE
// block between s_setprio 3 and s_setprio 0 (mc_math.h): seven of a bounce's fourteen.  Same opcodes, same operands, same bits
// (tests/test_gpu_pool_trans_groups.py renders with and without the groups: equal bit for bit); 71 VGPRs and 7 waves per SIMD as before.
// Measured (profiles/valu_microbench_prio.txt, trans_groups_k2_ab.txt): a grouped transcendental costs 8.3 - 9.1 cycles in a group of
// four, 8.6 - 9.8 in a pair; K2 14.01 -> 13.74 ms, 2.689 -> 2.643 cycles per VALU instruction on the same 1.2739e10 VALU instructions.
// One light: the same instructions per iteration as before.  Every further light repeats the sine and cosine in its own group (the
// compiler shared one pair between the unrolled light blocks before; a block cannot share out of another's).
// -DMC_PT_TRANS_UNGROUPED (make exp; the shipped build never sets it) compiles the instruction order before the groups.
//
// Loop predicates from lane masks the wave already holds (all tiers).  `__ballot(p)` of a bool that was merged across control flow is
// compiled as v_cndmask_b32 v, 0, 1, s[..] + v_cmp_ne_u32 vcc, 0, v: a mask that lies in scalar registers is written into a vector
// register and read back — two VALU instructions that compute nothing, in a kernel bound by VALU issue.  So: the termination test asks
// the scalar `batch >= n_batches` first and takes its ballots only while the pool drains; "no diffuse lane is on a sphere" is read off
// the mask the prologue's own compare `id >= 6` wrote; the emission of a path the roulette ends is added under the lanes' own condition.
// Seven VALU instructions an iteration less, every bit kept (tests/test_gpu_pool_valu_diet.py; profiles/valu_diet_k2_ab.txt).
// -DMC_PT_POOL_PARENT_FORMS (make exp) compiles the forms before.
//
// Lane state in wave masks (profiles/valu_diet2_k2_ab.txt).  A lane's two one-bit facts were per-lane values: `alive`, whose ballot at the
// top of the loop — its mask is data, the dead lanes of a pixel are counted — cost the same pair, and `emissive`, a 0.0f / 1.0f factor
// set by a v_mov in the stash pick-up, after the specular merge and after the diffuse bounce of (nearly) every iteration.
//   alive_m (fast, careful): a wave-uniform 64-bit mask in scalar registers.  It stays scalar only while no assignment to it stands under
//     a lanes' branch, and a ballot is free only of a COMPARE.  So the bounce block ends after the material, and the depth limit, the
//     intersection, the next bounce's random numbers and the roulette follow where all lanes pass: each compare's mask is and-ed into
//     alive_m by the scalar unit, the blocks between are entered through the inverse ballot (a bare s_and_saveexec_b64).  The same
//     instructions on the same operands in the live lanes; what a dead lane computes of them (key, rx, ry) the pick-up overwrites.
//   emis (all tiers): a per-lane condition, only ever tested — the compiler keeps it as a mask by itself.  The three emission sites add
//     accmat * e in the lanes where it holds (add_emission), leaving out multiplications by 1 and additions of +-0: the argument is beside
//     the first of them.
//   key is incremented in place (it went through a temporary and two copies), alpha = 1 of the mirror / glass bounce is one v_mov.
// Fast <1, 16, 3, true>: 8.5 VALU instructions an iteration less (SQ_INSTS_VALU), 71 VGPRs, 7 waves, K2 13.51 -> 13.27 ms; every bit kept in
// all tiers (tests/test_gpu_pool_lane_masks.py).  Where a form cost registers it is not taken (pool_lane_masks, pool_emis_cond): the strict
// kernels keep `alive` per lane (the mask form spilled), fast with two spheres keeps the parent's forms (8 -> 7 waves).
// -DMC_PT_POOL_FLOAT_STATE (make exp; implied by MC_PT_POOL_PARENT_FORMS) compiles the per-lane values: the parent's listing.
//
// Third diet (profiles/valu_diet3_listing.txt): what an iteration still computed although the wave had it, or held in a costlier place.
//   1  `key > krr` of the prologue's row select is the roulette's own mask of the iteration before: deep_m & ~end_m stays in scalar
//      registers over the loop edge (deep_row_m).
//   2  nl = +-n is read once per light, in max(dot(l, nl), 0): dot(l, n) with the flip applied to the sum by one v_bitop3
//      (dm::flip_where_sign_clear); the vector is formed only where a lane bounces off a diffuse sphere (nl_of).  The argument for the
//      one case that differs — an exactly cancelling sum, -0 for +0 — stands where nl was formed.
//   3  the three -w_neg of the slab intersection in vector registers (HotSlabN::load: a v_cndmask reads one scalar, and that is its mask).
//      The registers are the ones the staged record wasted: its "emits" flag shared a word with the material code, whose byte-selecting
//      compares need their constants in VGPRs.  The flag has slot 3 now (fast, careful), the code is the whole word (pool_flag_apart).
//   4  the roulette compares the unscaled draw with p * 2^32 from the record (rand01_zraw).
//   5  `id >= 0` of the stash entries taken is asked only while a wave can take an empty one: a pixel outside the image or the tile,
//      the ragged last batch.  (`lane & 48` of the refill stays re-derived: held it costs a register.)
// Fast <1, 16, 3, true>: 6.1 VALU instructions an iteration less by the listing, 71 VGPRs, 7 waves.  Taken per instantiation (pool_diet3):
// fast and careful with eight spheres keep the parent's loop (scratch); the strict kernels take nothing (item 4 measured no gain there).
// -DMC_PT_POOL_DIET3_PARENT (make exp; implied by the two older switches) compiles the forms before: the parent's listing
// (tests/test_gpu_pool_diet3.py renders with both: equal bit for bit).
#pragma once
#include <type_traits>
#include "pathtrace_kernel.h"

namespace mc {
namespace pt {

#ifdef MC_PT_POOL_PARENT_FORMS   // diagnostic build only (tests/test_gpu_pool_valu_diet.py): the loop predicates as ballots of carried bools
constexpr bool kPoolParentForms = true;
#else
constexpr bool kPoolParentForms = false;
#endif
// diagnostic builds only (tests/test_gpu_pool_lane_masks.py; the parent forms are older still): `alive` and `emissive` as per-lane values
#if defined(MC_PT_POOL_FLOAT_STATE) || defined(MC_PT_POOL_PARENT_FORMS)
constexpr bool kPoolFloatState = true;
#else
constexpr bool kPoolFloatState = false;
#endif
// A lane mask from a compare, and a mask as a per-lane condition.  (__ballot takes an int: a bool that was merged across control flow
// reaches it as v_cndmask_b32 v, 0, 1 + v_cmp_ne_u32 — and so does the builtin's argument when it is anything but a compare.  Of a
// compare it is the compare's own result in scalar registers; the inverse enters a branch with a bare s_and_saveexec_b64.)
__device__ __forceinline__ unsigned long long lanes_where(bool cmp) { return __builtin_amdgcn_ballot_w64(cmp); }
__device__ __forceinline__ bool lane_in(unsigned long long m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
// rad + accmat * e with the product rounded before the sum in every tier — what rad + (accmat * e) * 1.0f computes, contracted
// (fma(p, 1, rad) rounds p + rad once) or not (p * 1 = p).  Written out under contract(off): the fast tier would otherwise fuse
// accmat * e into the sum and round once where the form with the factor rounds twice.
__device__ __forceinline__ v3 add_emission(v3 rad, v3 accmat, v3 e) {
#pragma clang fp contract(off)
    const float px = accmat.x * e.x, py = accmat.y * e.y, pz = accmat.z * e.z;
    return v3{rad.x + px, rad.y + py, rad.z + pz};
}
// nl = dot(n, rd) < 0 ? n : -n (:390) in the fast tiers' form: the sign bit of the dot product, inverted, flips n
__device__ __forceinline__ v3 nl_of(v3 n, float dot_n_rd) {
    return v3{dm::flip_where_sign_clear(n.x, dot_n_rd), dm::flip_where_sign_clear(n.y, dot_n_rd), dm::flip_where_sign_clear(n.z, dot_n_rd)};
}
constexpr uint32_t kPoolEntryFloats = 8;     // {rd.x, rd.y, rd.z, t | id (-1: nothing to trace), key0 = samp * maxDepth, rnd.x, rnd.y of key0}
// floats per staged record, four rows of four (the packing at the top of the kernel is the definition):
//   row 0   geo.xyz | strict: p.  fast, careful: 1 / p — or, where pool_flag_apart holds, the "emits" flag (256 or 0, integer bits)
//   row 1   colour.rgb | the material code as integer bits, + 256 * emits unless pool_flag_apart (then the bare code)
//   row 2   emission.xyz | strict: RN(1 / p).  fast, careful: p — or, where pool_rr_unscaled holds, p * 2^32
//   row 3   fast, careful: colour.rgb / p | the same word as row 1's.  strict: unused
constexpr uint32_t kPoolRecordStride = 16;
template <int NS> constexpr uint32_t pool_record_floats() { return (6u + (uint32_t)NS) * kPoolRecordStride; }   // 6 planes + NS spheres
constexpr uint32_t kPoolStashFloats = 128u * kPoolEntryFloats;     // per wave: 64/S pixels x 2 batches x S entries
// Strict: the result ring holds this many batches per pixel (3 planes x, y, z).  Three for the reference's scene: with the 23 + 3 KB of a
// block six blocks fit a CU's 160 KB, and 6 waves per SIMD with a 3-batch ring beat 5 waves with a 4-batch ring (32.7 against 33.1 ms at K2;
// 2 batches stall the production: 34.3; profiles/r04_strict_occupancy.txt).  Scenes with more spheres run at 4 waves per SIMD: 4 batches.
template <int NS> constexpr uint32_t pool_result_batches() { return NS <= 3 ? 3u : 4u; }
template <int NS> constexpr uint32_t pool_result_floats() { return 64u * pool_result_batches<NS>() * 3u; }   // per wave: 64/S pixels x batches x S samples x 3
template <int Fast, int NS> constexpr uint32_t pool_wave_lds_floats() { return kPoolStashFloats + (Fast ? 0u : pool_result_floats<NS>()); }
template <int Fast, int NS> constexpr size_t pool_block_lds_bytes() { return (pool_record_floats<NS>() + 4u * pool_wave_lds_floats<Fast, NS>()) * sizeof(float); }
// Waves per SIMD the register budget is set for: 7 / 6 for the reference's three spheres (72 / 80 VGPRs); every further sphere
// keeps five more values live across a bounce (c_i - x, |c_i - x|^2 and its r^2-reduced form), so the budget widens with the count.
template <int Fast, int NS> constexpr int pool_waves() {
    constexpr int kFast3 = 7;     // 72 VGPRs (6: 18.29 ms, 7: 18.11, 8: 18.68 at K2)
    constexpr int kStrict3 = 6;   // 80 VGPRs (three values spilled, none reloaded inside an iteration), 6 blocks of 26 KB per CU
    return Fast ? (NS <= 3 ? kFast3 : NS <= 5 ? 6 : NS <= 6 ? 5 : 4) : (NS <= 3 ? kStrict3 : NS <= 6 ? 4 : 3);
}

// Which instantiations take the lane-mask forms (see the header): all would compute the same bits; these keep their occupancy and
// add no scratch with them.
template <int Fast, int NS> constexpr bool pool_parent_state() { return kPoolFloatState || (Fast == 1 && NS == 2); }   // (fast, two spheres: 8 -> 7 waves with any of them)
template <int Fast, int NS> constexpr bool pool_lane_masks() { return !pool_parent_state<Fast, NS>() && Fast != 0 && !(Fast == 2 && NS == 7); }
template <int Fast, int NS> constexpr bool pool_emis_cond() { return !pool_parent_state<Fast, NS>(); }

// The third diet (see the header), item by item and per instantiation as above: what an instantiation takes costs it neither a wave of
// occupancy nor a scratch instruction.  -DMC_PT_POOL_DIET3_PARENT (make exp; implied by the two older switches) compiles the forms before.
#if defined(MC_PT_POOL_DIET3_PARENT) || defined(MC_PT_POOL_FLOAT_STATE) || defined(MC_PT_POOL_PARENT_FORMS)
constexpr bool kPoolDiet3Parent = true;
#else
constexpr bool kPoolDiet3Parent = false;
#endif
// (fast and careful with eight spheres, at four and five waves: 16 B more scratch with items 1, 4 and 5 alone — they keep the parent's loop)
template <int Fast, int NS> constexpr bool pool_diet3() { return !kPoolDiet3Parent && !pool_parent_state<Fast, NS>() && !(Fast != 0 && NS == 8); }
// 1: the depth-over-5 mask carried over the loop edge (a lane mask: the kernels that hold alive_m)
template <int Fast, int NS> constexpr bool pool_deep_carry() { return pool_diet3<Fast, NS>() && pool_lane_masks<Fast, NS>(); }
// 2: dot(l, nl) as dot(l, n) with its sign flipped (the fast and careful tiers' flip; the strict kernel selects n or -n)
template <int Fast, int NS> constexpr bool pool_nl_dot() { return pool_diet3<Fast, NS>() && Fast != 0; }
// 3: how many of the three -w_neg the intersection holds in vector registers — all three wherever the flag below made the room
template <int Fast, int NS> constexpr int pool_wneg_vgprs() { return pool_diet3<Fast, NS>() && Fast != 0 ? 3 : 0; }
// 4: the roulette compares the unscaled draw with p * 2^32 from the record (strict: measured, 32.47 -> 32.52 ms at K2, inside the spread
// of 0.10 — not taken, the strict kernels are the parent's: profiles/valu_diet3_k2_ab.txt)
template <int Fast, int NS> constexpr bool pool_rr_unscaled() { return pool_diet3<Fast, NS>() && Fast != 0; }
// 5: no `id >= 0` of the entries taken while every entry the wave can take holds a path (the closed-box tiers' lane-mask kernels)
template <int Fast, int NS> constexpr bool pool_live_entries() { return pool_diet3<Fast, NS>() && pool_lane_masks<Fast, NS>(); }
// what makes the room for 3: a record's "emits" flag in a word of its own, the material code a whole word (fast, careful: slot 3 is free)
template <int Fast, int NS> constexpr bool pool_flag_apart() { return pool_diet3<Fast, NS>() && Fast != 0; }

// Disjoint (fast math): the host proved the spheres pairwise disjoint — shadow rays are decided without square roots
// (shadow_visible_disjoint); false: overlapping spheres, the root form (shadow_reaches_sphere).  The strict kernel has one form.
template <int Fast, int S, int NS, bool Disjoint = true>
__global__ void __launch_bounds__(256, (pool_waves<Fast, NS>())) pathtrace_pool_kernel(PTArgs a) {
    constexpr uint32_t kPoolRecordFloats = pool_record_floats<NS>();
    extern __shared__ float lds_dyn[];
    float* lds_obj = lds_dyn;
    // The 9 records, re-packed for two 16-byte reads per bounce at address id << 6: the plane normal / sphere centre with the
    // roulette probability max(max(c.x, c.y), c.z) (:394), the colour with the material code int(floor(m + 0.5)) (:378/:384)
    // and an "emits" flag as integer bits — the same fp32 operations on the same operands as evaluating them at every bounce.
    // Fast math: slot 3 holds v_rcp_f32(p), the factor :397's division multiplies by — formed once per block instead of once
    // per bounce and lane (a transcendental blocks the SIMD for 8 cycles); p itself, which :396 compares with, is in slot 11.
    // Strict: slot 3 holds p and slot 11 the correctly rounded 1 / p that the short division of :397 starts from (dm::div3).
    if (threadIdx.x < 6u + (uint32_t)NS) {
        const float* o = a.scene.obj + 12u * threadIdx.x;
        float* r = lds_obj + kPoolRecordStride * threadIdx.x;
        const float p = dm::gmax(dm::gmax(o[8], o[9]), o[10]);
        const float r3 = Fast ? dm::fdiv<Fast>(1.0f, p) : p;
        r[0] = o[0]; r[1] = o[1]; r[2] = o[2]; r[3] = r3;
        r[4] = o[8]; r[5] = o[9]; r[6] = o[10];
        const uint32_t emits = (o[4] != 0.0f || o[5] != 0.0f || o[6] != 0.0f) ? 256u : 0u;
        // (pool_flag_apart: the flag in slot 3, which 1 / p leaves free once the colour rows below are formed — the material code then is
        // the whole word: no byte select, and no vector registers that hold the constants a byte-selecting compare needs)
        constexpr bool kFlagApart = pool_flag_apart<Fast, NS>();
        const uint32_t mcode = (uint32_t)(int)__builtin_floorf(o[11] + 0.5f);
        r[7] = dm::as_float(kFlagApart ? mcode : (mcode | emits));
        // (pool_rr_unscaled: p * 2^32, what the roulette compares the unscaled draw with — rand01_zraw; p has no other reader)
        r[8] = o[4]; r[9] = o[5]; r[10] = o[6]; r[11] = Fast ? (pool_rr_unscaled<Fast, NS>() ? p * 4294967296.0f : p) : dm::rcp_short(p);
        // fast math: the colour already divided by p (:392 and :397 as ONE multiplication past depth 5), with the same integer bits
        if constexpr (Fast) { r[12] = o[8] * r3; r[13] = o[9] * r3; r[14] = o[10] * r3; r[15] = r[7]; }
        if constexpr (kFlagApart) r[3] = dm::as_float(emits);
    }
    __syncthreads();
    // fast math: the sphere tests of a bounce (three of the shadow ray, three of the next ray, all from the hit point x) read
    // |c_i - x|^2 - r_i^2, formed once, instead of each adding r_i^2 to its b^2 - |c_i - x|^2
    // (fast tier only.  The careful tier keeps the reference's order (b^2 - |c - x|^2) + r^2: of the identities of exact arithmetic fast
    // math does not execute, this one and the un-normalised directions are the two whose forked samples do not balance — more of them
    // lose radiance than gain it; with both in the reference's form gains and losses cancel: profiles/r05_fork_bias_identities.txt)
    constexpr bool kOccR2 = Fast == 1;
    // what of the lane-mask forms this instantiation takes (pool_lane_masks)
    constexpr bool kLaneMasks = pool_lane_masks<Fast, NS>(), kEmisCond = pool_emis_cond<Fast, NS>(), kOneAlpha = kEmisCond;
    // fast tier: the bounce's transcendentals whose operands are known early are issued as prioritised groups (mc_math.h, "groups")
    constexpr bool kGrouped = Fast == 1 && dm::kTransGroups;
    // what of the third diet it takes (pool_deep_carry ...)
    constexpr bool kDeepCarry = pool_deep_carry<Fast, NS>(), kNlDot = pool_nl_dot<Fast, NS>(), kRrUnscaled = pool_rr_unscaled<Fast, NS>(),
                   kLiveEntries = pool_live_entries<Fast, NS>(), kFlagApart = pool_flag_apart<Fast, NS>();
    constexpr uint32_t TW = WaveTile<S>::w, TH = WaveTile<S>::h, Ring = 2u * (uint32_t)S, RRing = pool_result_batches<NS>() * (uint32_t)S;
    HotSlabN<NS> hot;
    // (uniform operands but W_pos — and as many of W_negm as pool_wneg_vgprs finds room for: this kernel has no vector registers to spare for copies)
    hot.template load<false, true, pool_wneg_vgprs<Fast, NS>()>(a.scene);
    // A lane's pixel (pix = lane / S of the wave tile) and slot of a batch (sub = lane % S) never change.  What derives from them
    // and is needed only now and then — the stash base, the tile row, the validity — is derived afresh from an opaque copy of
    // the thread id where it is used, so that it does not occupy registers across the bounce loop (80 VGPRs = 6 waves per SIMD).
    struct Lane { uint32_t lane, pix, sub, ty; bool valid; };
    auto my_lane = [&](bool with_row) {
        uint32_t tid = threadIdx.x;
        // (The refill's lane and sub stay in registers — two instructions an iteration less; the fast and careful kernels have the room.
        //  The strict kernel at its 80-register budget has not: kept "in registers" they were spilled, and the lanes-below-me mask was
        //  reloaded from scratch in the stash pick-up of nearly every iteration; there they are re-derived from the thread index.)
        if (Fast == 0 || with_row) asm volatile("" : "+v"(tid));
        Lane q;
        q.lane = tid & 63u; q.pix = q.lane / (uint32_t)S; q.sub = q.lane % (uint32_t)S;
        const uint32_t wave = tid >> 6;
        q.ty = 0u; q.valid = false;
        if (with_row) {   // pathTracer.comp:348
            q.ty = blockIdx.y * (2u * TH) + (wave >> 1) * TH + q.pix / TW;
            const uint32_t gxx = blockIdx.x * (2u * TW) + (wave & 1u) * TW + q.pix % TW;
            q.valid = gxx < a.W && tile_row_to_storage(q.ty, a.row_begin, a.row_block, a.row_stride) < a.row_end;
        }
        return q;
    };
    // my pixel's coordinates (:349) stay: the RNG key of every bounce needs them; so does the base of its stash
    uint32_t gx, gy;
    bool pixel_valid;         // my pixel lies in the image and in the tile (:348); kept as a lane mask, not re-derived per batch
    float* const gstash = lds_dyn + kPoolRecordFloats + (threadIdx.x >> 6) * pool_wave_lds_floats<Fast, NS>() +
                          ((threadIdx.x & 63u) / (uint32_t)S) * (Ring * kPoolEntryFloats);
    // strict: my pixel's result ring [3][RRing] (x, y, z planes) behind the wave's stash
    float* const gres = lds_dyn + kPoolRecordFloats + (threadIdx.x >> 6) * pool_wave_lds_floats<Fast, NS>() + kPoolStashFloats +
                        ((threadIdx.x & 63u) / (uint32_t)S) * (3u * RRing);
    // (re-deriving THIS address where it is used — path ends, commits — instead of keeping it was measured: + 1.1 ms at K2 strict)
    {
        const uint32_t tid = threadIdx.x, wave = tid >> 6, pix = (tid & 63u) / (uint32_t)S;
        gx = blockIdx.x * (2u * TW) + (wave & 1u) * TW + pix % TW;
        const uint32_t ty = blockIdx.y * (2u * TH) + (wave >> 1) * TH + pix / TW;
        const uint32_t srow = tile_row_to_storage(ty, a.row_begin, a.row_block, a.row_stride);
        pixel_valid = gx < a.W && srow < a.row_end;
        gy = a.H - 1u - (pixel_valid ? srow : 0u);
    }
    const uint32_t n_batches = (a.sample_end - a.sample_begin + (uint32_t)S - 1u) / (uint32_t)S;
    uint32_t batch = 0u;      // wave-uniform: batches produced; every pixel's stash has received batch * S entries
    uint32_t ghead = 0u;      // entries my pixel's lanes have taken (the same value in all S lanes)
    // ---- the state of a lane's path, and the radiance its paths have gathered
    v3 ro{0, 0, 0}, rd{0, 0, 1}, accmat{1, 1, 1}, acc{0, 0, 0};   // acc: fast = this lane's partial sum; strict = the pixel's ordered sum
    v3 accrad{0, 0, 0};       // strict: the radiance of the current path (:391, :422)
    if constexpr (!Fast) {
        // strict: a later sample range continues the ordered sum the caller passes back in (the samps.x protocol, :451-:452) —
        // every lane of the pixel starts from the stored value and adds the range's samples in order, as one launch would have
        if (a.sample_begin > 0u) {
            const Lane me = my_lane(true);
            if (me.valid) { const float4 prev = a.out[(size_t)me.ty * a.W + gx]; acc = v3{prev.x, prev.y, prev.z}; }
        }
    }
    uint32_t cur = 0u;        // strict: index (within my pixel) of the sample this lane traces; its result slot is cur % RRing
    uint32_t committed = 0u;  // strict: samples of my pixel already added to acc (the same value in all S lanes)
    // (wave-uniform: held in a scalar register — as a vector value the strict kernel spilled it and reloaded it at every path end)
    const float fspp = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int((float)a.spp)));
    float emissive = 1.0f, t = 0.0f, occ[NS];
#pragma unroll
    for (int i = 0; i < NS; i++) occ[i] = 0.0f;
    int id = 0;
    uint32_t key = 0u, kend = 0u, krr = 0u;   // key0 + depth; key0 + maxDepth; key0 + 5 (:395: roulette while key > krr)
    // rand01 of the bounce about to be traced (:393).  It is drawn at the END of the previous bounce, together with the Russian
    // roulette decision of :396 (the hit — hence p — is known there: the loop is rotated), so that a path the roulette ends
    // frees its lane at the end of an iteration, not a third of the way into the next one.
    float rx = 0.0f, ry = 0.0f;
    bool alive = false;
    // The two facts as lane masks (kLaneMasks, kEmisCond: which of them this instantiation takes).  `alive_m`, the lanes that trace a path, is a
    // wave-uniform 64-bit value in scalar registers: the refill needs it as DATA (the dead lanes of a pixel, counted), and every change
    // of it is a scalar and / or of compares' masks taken where all lanes pass.  `emis` (:365: no diffuse surface met since the camera or
    // the last specular bounce) is only ever tested, so it is a per-lane condition the compiler keeps as a mask by itself.
    unsigned long long alive_m = 0ull;
    bool emis = true;
    // kDeepCarry: the lanes that go on past depth 5 — the roulette's own mask less the paths it ended, kept in scalar registers over the
    // loop edge.  The next prologue picks the colour row by it instead of comparing key with krr again: for a lane that goes on it is that
    // compare on the same two values, and a lane that takes a stash entry in between was not in alive_m, so its bit is clear — as its
    // compare would be (key = key0 <= krr).
    unsigned long long deep_row_m = 0ull;
    // kLiveEntries: every stash entry this wave's lanes can take holds a path (closed box: every camera ray hits) — all four pixels lie in
    // the image and the tile, and no batch produced so far is a ragged last one.  Wave-uniform; while it holds, `id >= 0` of the entries
    // taken is not asked.
    bool pixels_live = false;
    uint32_t full_batches = 0u;   // (batches before a ragged last one: every batch when the sample range is a multiple of S)
    if constexpr (kLiveEntries) {
        pixels_live = __ballot(!pixel_valid) == 0ull;
        full_batches = (a.sample_end - a.sample_begin) % (uint32_t)S == 0u ? n_batches : n_batches - 1u;
    }
    // every iteration either traces a bounce of a live lane, or consumes stash entries, or produces a batch: bounded
    unsigned long long max_iters = (unsigned long long)n_batches * S * (a.max_depth + 2ull) + 64ull;
#ifdef MC_PT_POOL_TEST_BOUND   // diagnostic build only (tests/test_gpu_pool.py): a bound the loop must trip
    max_iters = MC_PT_POOL_TEST_BOUND;
#endif
    bool finished = false;
    for (unsigned long long it = 0; it < max_iters; it++) {
        // ---- lanes whose path ended take their pixel's next camera rays
        // (MC_REGION: diagnostic build only — make stats, tools/pool_region_stats.py — executions and active lanes per block)
        MC_REGION(0);    // an iteration
        const unsigned long long deadm = kLaneMasks ? ~alive_m & lanes_where(true) : __ballot(!alive);
        if (deadm != 0ull) {
            MC_REGION(1);    // refill bookkeeping
            const Lane me = my_lane(false);
            // the dead lanes of my pixel: S bits of the ballot starting at my pixel's first lane
            const uint32_t gbits = (uint32_t)(deadm >> (me.lane - me.sub)) & (S == 32 ? ~0u : ((1u << (S & 31)) - 1u));
            const uint32_t need = (uint32_t)__builtin_popcount(gbits);
            uint32_t avail = batch * (uint32_t)S - ghead;
            bool want = batch < n_batches && __ballot(need > avail) != 0ull && __ballot(avail > (uint32_t)S) == 0ull;
            if constexpr (!Fast) {
                if (want) {   // (uniform) add the batches whose samples have all ended, in order; then: is the result ring free?
                    uint32_t oldest = alive ? cur : 0xffffffffu;                      // oldest sample a lane of my pixel still traces
                    if constexpr (S == 16) {
                        // The minimum over the pixel's 16 lanes = one DPP row: four rotations within the row (row_ror 8, 4, 2, 1), each
                        // folded into its v_min_u32 — no LDS round trip and no address registers.  (The butterfly through ds_bpermute kept
                        // four lane-address VGPRs live across the whole kernel; at the strict kernel's 80-register budget they were
                        // spilled and RELOADED FROM SCRATCH here, inside the loop, each load waited for.)  Integer minimum: same value.
                        auto rot_min = [](uint32_t v, auto ctrl) {
                            const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, decltype(ctrl)::value, 0xf, 0xf, false);
                            return o < v ? o : v;
                        };
                        oldest = rot_min(oldest, std::integral_constant<int, 0x128>{});   // row_ror:8
                        oldest = rot_min(oldest, std::integral_constant<int, 0x124>{});   // row_ror:4
                        oldest = rot_min(oldest, std::integral_constant<int, 0x122>{});   // row_ror:2
                        oldest = rot_min(oldest, std::integral_constant<int, 0x121>{});   // row_ror:1
                    } else {
#pragma unroll
                        for (uint32_t o = 1; o < (uint32_t)S; o <<= 1) {
                            const uint32_t other = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((me.lane ^ o) << 2), (int)oldest);
                            oldest = other < oldest ? other : oldest;
                        }
                    }
                    const uint32_t fin = oldest < ghead ? oldest : ghead;             // samples [0, fin) are taken and ended
                    while (committed + (uint32_t)S <= fin) {
                        for (uint32_t k = 0; k < (uint32_t)S; k++) {                  // :452 acc += accrad / spp, in sample order
                            const uint32_t slot = (committed + k) % RRing;
                            acc.x += gres[slot]; acc.y += gres[RRing + slot]; acc.z += gres[2u * RRing + slot];
                        }
                        committed += (uint32_t)S;
                    }
                    want = __ballot((batch + 1u) * (uint32_t)S - committed > RRing) == 0ull;   // every pixel's ring has room
                }
            }
            // one more batch when a pixel wants more rays than it has — and every pixel's ring has room for S more
            if (want) {
                MC_REGION(2);    // a batch of camera rays
                const Lane g = my_lane(false);
                const uint32_t samp = a.sample_begin + batch * (uint32_t)S + g.sub;
                // (strict: the pixel coordinates as fresh values — otherwise float(gy) of :359 is hoisted out of the loop, and at this
                //  kernel's register budget "out of the loop" meant spilled and reloaded from scratch at the end of every iteration)
                uint32_t cgx = gx, cgy = gy;
                if constexpr (!Fast) asm volatile("" : "+v"(cgx), "+v"(cgy));
                const v3 crd = camera_ray<Fast>(a, cgx, cgy, samp);
                v3 oc0[NS];
                float occ0[NS], ct;
#pragma unroll
                for (int i = 0; i < NS; i++) {
                    oc0[i] = v3{a.cam_oc[i][0], a.cam_oc[i][1], a.cam_oc[i][2]};
                    occ0[i] = kOccR2 ? a.cam_occ[i] - hot.r2[i] : a.cam_occ[i];
                }
                int cid = intersect_slab<Fast, (Fast != 0), kOccR2, 22>(hot, a.lc, crd, ct, false, occ0, oc0);
                // nothing to trace: a pixel outside the tile, a sample beyond the range; a camera ray that misses everything (:369)
                // gathers nothing either
                if (!(pixel_valid && samp < a.sample_end)) cid = -1;
                if constexpr (!Fast) {   // such a sample's result is a zero (adding +0 changes no bit of the sum)
                    const uint32_t slot = (batch * (uint32_t)S + g.sub) % RRing;
                    if (cid < 0) { gres[slot] = 0.0f; gres[RRing + slot] = 0.0f; gres[2u * RRing + slot] = 0.0f; }
                }
                float4* e = reinterpret_cast<float4*>(gstash + ((batch * (uint32_t)S + g.sub) & (Ring - 1u)) * kPoolEntryFloats);
                e[0] = make_float4(crd.x, crd.y, crd.z, ct);
                const v3 r0 = rand01(gx, gy, samp * a.max_depth);           // :393 at depth 0 (no roulette there: z unused)
                e[1] = make_float4(dm::as_float((uint32_t)cid), dm::as_float(samp * a.max_depth), r0.x, r0.y);
                batch++;
                avail += (uint32_t)S;
            }
            const uint32_t rank = (uint32_t)__builtin_popcount(gbits & ((1u << me.sub) - 1u));   // dead lanes of my pixel below me
            const unsigned long long take_m = kLaneMasks ? deadm & lanes_where(rank < avail) : 0ull;
            if (kLaneMasks ? lane_in(take_m) : (!alive && rank < avail)) {
                MC_REGION(3);    // lanes taking a stash entry
                const float4* q = reinterpret_cast<const float4*>(gstash + ((ghead + rank) & (Ring - 1u)) * kPoolEntryFloats);
                const float4 q0 = q[0], q1 = q[1];
                rd = v3{q0.x, q0.y, q0.z}; t = q0.w;
                if constexpr (!Fast) { cur = ghead + rank; accrad = v3{0.0f, 0.0f, 0.0f}; }   // :361
                id = (int)dm::as_uint(q1.x);
                key = dm::as_uint(q1.y); kend = key + a.max_depth; krr = key + 5u;
                rx = q1.z; ry = q1.w;
                ro = a.lc;                                                  // :362
                accmat = v3{1.0f, 1.0f, 1.0f};                              // :361
                if constexpr (kEmisCond) emis = true; else emissive = 1.0f;   // :365
                if constexpr (!kLaneMasks) alive = id >= 0;
            }
            // (where all lanes pass: set under the lanes' branch the mask would be a vector value)
            if constexpr (kLiveEntries) {
                if (pixels_live && batch <= full_batches) alive_m |= take_m;   // (uniform)
                else alive_m |= take_m & lanes_where(id >= 0);
            } else if constexpr (kLaneMasks) alive_m |= take_m & lanes_where(id >= 0);
            ghead += need < avail ? need : avail;
        }
        // pool exhausted and every path ended?  (no lane alive but entries left: only empty entries were taken — go round again)
        // (the scalar test first: while batches are left — all but the last ten or so of a wave's ~294 iterations — no ballot is taken)
#ifdef MC_PT_POOL_PARENT_FORMS
        if (__ballot(alive) == 0ull && batch >= n_batches && __ballot(ghead != batch * (uint32_t)S) == 0ull) { finished = true; break; }
#else
        if (batch >= n_batches && (kLaneMasks ? alive_m : __ballot(alive)) == 0ull && __ballot(ghead != batch * (uint32_t)S) == 0ull) { finished = true; break; }
#endif
        // ---- one bounce of every live lane: prologue, material, intersection of the next depth (the rotated loop of trace_sample)
        // (structured ifs, no break / continue: every extra exit edge of this block cost a dozen register copies at its merge)
        // kLaneMasks: the block ends after the material; the depth limit, the intersection, the next bounce's random numbers and the
        // roulette follow where all lanes pass, each compare's mask and-ed into `alive_m` there — the same instructions (what a dead
        // lane computes of them is never read: the pick-up rewrites id, key, rx, ry), and no mask is merged across a lanes' branch.
        v3 xoc[NS];                                                               // c_i - x (:317 at the next depth, :408 now)
        if (kLaneMasks ? lane_in(alive_m) : alive) {
            {
                MC_REGION(4);    // a bounce: prologue
                // the live lanes on a sphere, as the compare's own lane mask (the diffuse branch asks whether any of ITS lanes, a subset
                // of these, is on one)
                unsigned long long sph_m = 0ull;
                if constexpr (!kPoolParentForms) sph_m = __ballot(id >= 6);
                v3 x = ro + rd * t;                                               // :374
#pragma unroll
                for (int i = 0; i < NS; i++) { xoc[i] = v3{hot.c[i][0], hot.c[i][1], hot.c[i][2]} - x; occ[i] = dot(xoc[i], xoc[i]); }
                float xcc[NS];                                                    // |c_i - x|^2 itself (:410 needs it)
#pragma unroll
                for (int i = 0; i < NS; i++) { xcc[i] = occ[i]; if constexpr (kOccR2) occ[i] = occ[i] - hot.r2[i]; }
                const float4* obj = reinterpret_cast<const float4*>(lds_obj + kPoolRecordStride * (uint32_t)id);   // per-lane fetch
                // (fast: past depth 5 the colour row is the one already divided by the roulette probability)
                // (kDeepCarry: the mask the previous iteration's roulette left — see deep_row_m)
                const bool deep_row = kDeepCarry ? lane_in(deep_row_m) : (Fast && key > krr);
                const float4 o0 = obj[0], o1 = obj[deep_row ? 3 : 1];
                // (fast, careful: o0.w is not read and the compiler narrows row 0 to ds_read_b96.  Keeping the word in use for a
                //  ds_read_b128 was measured: 13.220 against 13.223 ms at K2, a tenth of the run-to-run spread — not kept,
                //  profiles/valu_diet2_k2_ab.txt)
                const bool is_sphere = id >= 6;
                v3 geo{o0.x, o0.y, o0.z};
                v3 col{o1.x, o1.y, o1.z};
                const uint32_t mbits = dm::as_uint(o1.w);
                const int mat = kFlagApart ? (int)mbits : (int)(mbits & 255u);    // :378/:384
                const bool hit_emits = kFlagApart ? dm::as_uint(o0.w) != 0u : mbits >= 256u;
#ifdef MC_PT_REGION_STATS
                if (is_sphere) MC_REGION(5);    // sphere normal
#endif
                v3 n = is_sphere ? normalize<Fast>(x - geo) : geo;                // :381/:387
                const float dot_n_rd = dot(n, rd);
                v3 nl;                                                            // :390 nl = dot(n, rd) < 0 ? n : -n
                // kNlDot: the vector nl is formed only where a lane bounces off a diffuse sphere (the general basis); the light's cosine is
                // dot(l, n) with the flip applied to the sum.  Negating every component of n negates every product and every partial sum
                // of the dot product exactly (rounding to nearest is symmetric, contracted or not), so the flipped sum IS dot(l, -n) —
                // but for a sum that cancels exactly: +0 in either order, hence -0 once flipped where dot(l, -n) gives +0.  max(., 0) and
                // the multiplication by the solid angle's finite factor make that a scale of +-0, and (accmat * le) * (+-0) is a zero
                // added to a sum that is never -0 (the argument beside add_emission's first use): every bit of rad is kept.
                // (dm::flip_where_sign_clear: one v_bitop3 of dot_n_rd, the value and the sign mask at each use — no flip word is held)
                if constexpr (kNlDot) {
                    // (nl is not read: the light's cosine flips its sum, the general bounce forms nl_of(n, dot_n_rd) — in the fast tiers.
                    //  The strict kernel hands nl to specular_bounce_general and must never get here with an unflipped normal.)
                    static_assert(!kNlDot || Fast != 0, "the flipped dot product is the fast and careful tiers' form: strict reads nl");
                    nl = n;
                } else if constexpr (Fast) {   // (the sign bit of the dot product, inverted, flips n — trace_sample)
                    const uint32_t flip = ~dm::as_uint(dot_n_rd) & 0x80000000u;
                    nl = v3{dm::as_float(dm::as_uint(n.x) ^ flip), dm::as_float(dm::as_uint(n.y) ^ flip), dm::as_float(dm::as_uint(n.z) ^ flip)};
                } else {
                    nl = dot_n_rd < 0.0f ? n : -n;
                }
                v3& rad = Fast ? acc : accrad;                                    // where gathered radiance goes (see the header)
                if constexpr (!kEmisCond) {
                if (__ballot(mbits >= 256u) != 0ull) {                            // :391 (non-emitters add a zero: box_ok)
                    MC_REGION(12);   // emission of a hit
                    const float4 o2 = obj[2];
                    rad = rad + (accmat * v3{o2.x, o2.y, o2.z}) * emissive;
                }
                } else if (hit_emits && emis) {                                      // :391
                    // Only the emitters' lanes whose condition holds add, and they add accmat * e without a factor.  Every bit is kept:
                    // the factor `emissive` was 1.0f or 0.0f and nothing else.  1: (accmat * e) * 1 = accmat * e, and contracted,
                    // fma(accmat * e, 1, rad), is the product's rounded value plus rad, rounded once — add_emission's sum.  0:
                    // (accmat * e) * 0 is a zero of either sign for the finite accmat of a closed box (colours in [0, 1] divided by their
                    // own maximum, finite glass factors) and finite e, and rad + (+-0) = rad for every rad but -0, which rad never is
                    // (it starts at +0 and only receives sums; a sum is -0 only when both operands are).  A lane that did not hit an
                    // emitter read e = +0: a zero again.  (The argument of the roulette's emission below, applied to the factor too.)
                    MC_REGION(12);   // emission of a hit
                    const float4 o2 = obj[2];
                    rad = add_emission(rad, accmat, v3{o2.x, o2.y, o2.z});
                }
                accmat = accmat * col;                                            // :392
                const v3 rnd{rx, ry, 0.0f};                                       // :393 (drawn at the end of the previous bounce)
                // :395, :397 (:396 was decided there too).  Strict: accmat / p, p = o0.w (:394).  Fast: o1 is the colour row divided by p
                if constexpr (!Fast) { if (key > krr) accmat = divs_recip<Fast>(accmat, o0.w, obj[2].w); }
                bool go = true;
                {
                ro = x;                                                           // :429, :434, :447
                if (mat == 1) {                                                   // :400 diffuse
                    MC_REGION(13);   // diffuse: light sample + shadow test
                    v3 accmat_over_pi{0.0f, 0.0f, 0.0f};                          // strict: :422's accmat / pi, once per bounce
                    if constexpr (!Fast) accmat_over_pi = divs_recip<Fast>(accmat, kPi, kInvPi);
#pragma unroll
                    for (int i = 0; i < NS; i++) {                                // :403
                        if (!((a.scene.emissive_mask >> i) & 1u)) continue;       // :407 (uniform)
                        const float* ls = a.scene.obj + 12 * (6 + i);
                        v3 le{ls[4], ls[5], ls[6]};
                        float cos_a_max;
                        v3 l = light_sample_direction<Fast, kGrouped>(xoc[i], xcc[i], hot.r2[i], rnd, cos_a_max);   // :408-:413
                        bool lit;                                                                          // :420
                        if constexpr (Fast && Disjoint) lit = shadow_visible_disjoint<kOccR2>(hot, l, i, xoc, occ);
                        else lit = shadow_reaches_sphere<Fast, kOccR2>(hot, x, l, i, xoc[i], occ);
                        if (lit) {
                            MC_REGION(8);    // light contribution
                            if constexpr (Fast) {
                                const float l_nl = kNlDot ? dm::flip_where_sign_clear(dot(l, n), dot_n_rd) : dot(l, nl);
                                // (kNlDot: the same v_max_f32 v, 0, v, written out — fmaxf of a value that comes out of a bit operation gets
                                //  a v_max_f32 v, v, v in front of it, which quiets a signalling NaN that no flipped sum can be)
                                const float cosine = kNlDot ? dm::max_zero_as_is(l_nl) : __builtin_fmaxf(l_nl, 0.0f);
                                const float scale = cosine * (2.0f - (cos_a_max + cos_a_max));   // :421-:422
                                rad = rad + (accmat * le) * scale;
                            } else {
                                const float omega = (2.0f * kPi) * (1.0f - cos_a_max);                     // :421
                                rad = rad + ((accmat_over_pi * dm::gmax(dot(l, nl), 0.0f)) * le) * omega;  // :422
                            }
                        }
                    }
                    // :426-:428 (uniform: no lane of the wave bounces off a diffuse SPHERE — the light — in almost every iteration)
                    auto walls_only = [&]() {
                        if constexpr (kPoolParentForms) return __ballot(is_sphere) == 0ull;
                        else return (sph_m & __ballot(true)) == 0ull;
                    };
                    if constexpr (kGrouped) {   // (the four transcendentals both forms share: one group in front of them)
                        const BounceTrans bt = bounce_trans_grouped(rnd);
                        if (walls_only()) { MC_REGION(9); rd = cosine_bounce_wall_grouped(id, bt); }
                        else { MC_REGION(10); rd = cosine_bounce_grouped<true>(kNlDot ? nl_of(n, dot_n_rd) : nl, bt); }
                    } else if (walls_only()) { MC_REGION(9); rd = cosine_bounce_wall<Fast>(id, rnd); }
                    else { MC_REGION(10); rd = cosine_bounce<Fast, true>(kNlDot ? nl_of(n, dot_n_rd) : nl, rnd); }
                    if constexpr (kEmisCond) emis = false; else emissive = 0.0f;  // :429
                } else {                                                          // :432 mirror, :437 glass (box_ok: 2 or 3)
                    MC_REGION(11);   // mirror / glass
                    if constexpr (Fast) rd = specular_bounce_fast<Fast, kOneAlpha>(mat, rd, n, dot_n_rd, rnd.x, accmat);
                    else rd = specular_bounce_general<false, true>(mat, rd, n, nl, dot_n_rd, rnd.x, accmat);
                    if constexpr (kEmisCond) emis = true; else emissive = 1.0f;   // :447
                }
                if constexpr (!kLaneMasks) {
                key++;
                go = key != kend;                                                 // :367 depth limit
                if (go) {
                    MC_REGION(14);   // intersection of the next depth
                    id = intersect_slab<Fast, (Fast != 0), kOccR2, 16>(hot, ro, rd, t, false, occ, xoc);
                    go = id >= 0;                                                 // :369
                }
                if (go) {                                                         // the next bounce's random numbers and roulette
                    // (kRrUnscaled: z as the converted integer, compared with p * 2^32 — rand01_zraw)
                    const v3 rn = kRrUnscaled ? rand01_zraw(gx, gy, key) : rand01(gx, gy, key);   // :393 (key = samp * maxDepth + depth)
                    rx = rn.x; ry = rn.y;
                    if (key > krr) {                                              // :395 depth > 5
                        MC_REGION(15);   // roulette
                        const float4* nobj = reinterpret_cast<const float4*>(lds_obj + kPoolRecordStride * (uint32_t)id);
                        go = !(rn.z >= nobj[Fast ? 2 : 0].w);                     // :396
                        // a path the roulette ends has still gathered the emission of this hit (:391 precedes :396)
                        if constexpr (kPoolParentForms) {
                            if (__ballot(!go && dm::as_uint(nobj[1].w) >= 256u) != 0ull) {
                                const float4 o2 = nobj[2];
                                if (!go) rad = rad + (accmat * v3{o2.x, o2.y, o2.z}) * emissive;
                            }
                        } else if constexpr (kEmisCond) {
                            // (as below, and without the factor: see the emission of a hit)
                            if (!go && (kFlagApart ? dm::as_uint(nobj[0].w) != 0u : dm::as_uint(nobj[1].w) >= 256u) && emis) {
                                const float4 o2 = nobj[2];
                                rad = add_emission(rad, accmat, v3{o2.x, o2.y, o2.z});
                            }
                        } else if (!go && dm::as_uint(nobj[1].w) >= 256u) {
                            // Only the emitters add.  The wave-wide form let every ended lane add whenever one of them had hit an
                            // emitter: accmat * e * emissive with e = +-0, the emission of a record whose flag is clear.  accmat is finite
                            // (box_ok: colours in [0, 1], divided by their own maximum; the glass factors are finite), so that product is a
                            // zero of either sign, and rad + (+-0) = rad for every rad but -0 — which rad never is: it starts at +0 and
                            // only ever receives sums, and a sum is -0 only when both operands are.  Leaving the addition out keeps every bit.
                            const float4 o2 = nobj[2];
                            rad = rad + (accmat * v3{o2.x, o2.y, o2.z}) * emissive;
                        }
                    }
                }
                }
                }
                if constexpr (!Fast && !kLaneMasks) {
                    if (!go) {   // the path has ended: :452's accrad / samps.y into the sample's slot of the result ring
                        const v3 q = divs_recip<Fast>(accrad, fspp, a.inv_spp);
                        const uint32_t slot = cur % RRing;
                        gres[slot] = q.x; gres[RRing + slot] = q.y; gres[2u * RRing + slot] = q.z;
                    }
                }
                if constexpr (!kLaneMasks) alive = go;
            }
        }
        if constexpr (kLaneMasks) {
            static_assert(Fast != 0 || !kLaneMasks, "the strict kernels keep `alive` per lane: the mask form spilled (pool_lane_masks)");
            v3& rad = acc;
            // (key of a dead lane is never read again: incremented in every lane, in place — the increment under the lanes' branch went
            //  through a temporary, a copy of kend for the lanes at the depth limit and a copy of the temporary for the others)
            key++;
            alive_m &= lanes_where(key != kend);                                  // :367 depth limit
            if (lane_in(alive_m)) {
                MC_REGION(14);   // intersection of the next depth
                id = intersect_slab<Fast, (Fast != 0), kOccR2, 16>(hot, ro, rd, t, false, occ, xoc);
            }
            // (:369: a closed box — every ray hits)
            // the next bounce's random numbers and roulette
            // (kRrUnscaled: z as the converted integer, compared with p * 2^32 — rand01_zraw)
            const v3 rn = kRrUnscaled ? rand01_zraw(gx, gy, key) : rand01(gx, gy, key);   // :393 (key = samp * maxDepth + depth)
            rx = rn.x; ry = rn.y;
            const unsigned long long deep_m = alive_m & lanes_where(key > krr);   // :395 depth > 5
            const float4* nobj = reinterpret_cast<const float4*>(lds_obj + kPoolRecordStride * (uint32_t)id);   // (formed once, read under the masks)
            float pn;                                                             // the hit's roulette probability, read by the deep lanes
            asm volatile("" : "=v"(pn));                                          // (any value elsewhere, and no instruction: deep_m masks the compare)
            if (lane_in(deep_m)) {
                MC_REGION(15);   // roulette
                pn = nobj[2].w;   // (kRrUnscaled: p * 2^32)
            }
            const unsigned long long end_m = deep_m & lanes_where(rn.z >= pn);    // :396
            alive_m &= ~end_m;
            if constexpr (kDeepCarry) deep_row_m = deep_m & ~end_m;
            if (lane_in(end_m)) {
                // a path the roulette ends has still gathered the emission of this hit (:391 precedes :396) — the emitters' lanes alone,
                // and without the factor, as at the emission of a hit above
                if ((kFlagApart ? dm::as_uint(nobj[0].w) != 0u : dm::as_uint(nobj[1].w) >= 256u) && emis) {
                    const float4 o2 = nobj[2];
                    rad = add_emission(rad, accmat, v3{o2.x, o2.y, o2.z});
                }
            }
        }
    }
    // the bound tripped (a scheduling defect): say so — the image is incomplete (mc_context::check_status -> MC_ERR_HIP)
    if (!finished && a.status && (threadIdx.x & 63u) == 0u) atomicOr(a.status, 2u);
    float4 sum = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const Lane fin = my_lane(true);
    if constexpr (Fast) {
        // ---- :452-:453: the S partial sums of a pixel, added in lane order by each of its lanes (all S copies identical)
        auto from_lane = [](float v, uint32_t src) {
            return __int_as_float(__builtin_amdgcn_ds_bpermute((int)(src << 2), __float_as_int(v)));
        };
        for (uint32_t k = 0; k < (uint32_t)S; k++) {
            const uint32_t src = fin.lane - fin.sub + k;
            sum.x += from_lane(acc.x, src); sum.y += from_lane(acc.y, src); sum.z += from_lane(acc.z, src);
        }
        sum.x *= a.inv_spp; sum.y *= a.inv_spp; sum.z *= a.inv_spp;
        // a later sample range of a progressive render (the samps.x protocol, :451-:452): the range's share is added to the stored
        // accumulator.  (Fast math has no ordered-sum contract: 5 ranges and one launch agree within the tolerance, not bit for bit;
        // the SAME split composes identically on every tiling.)
        if (a.sample_begin > 0u && fin.valid) {
            const float4 prev = a.out[(size_t)fin.ty * a.W + gx];
            sum.x += prev.x; sum.y += prev.y; sum.z += prev.z;
        }
    } else {
        // ---- every sample of the pool has ended: the batches not yet added, in sample order (entries beyond the sample range hold zeros)
        while (committed < n_batches * (uint32_t)S) {
            for (uint32_t k = 0; k < (uint32_t)S; k++) {
                const uint32_t slot = (committed + k) % RRing;
                acc.x += gres[slot]; acc.y += gres[RRing + slot]; acc.z += gres[2u * RRing + slot];
            }
            committed += (uint32_t)S;
        }
        sum = make_float4(acc.x, acc.y, acc.z, 0.0f);
    }
    if (a.sample_end == a.spp) {                                                // :453 after sample spp-1
        sum.x = dm::fpow<Fast>(dm::gmin(dm::gmax(sum.x, 0.0f), 1.0f), 0.45f) * 255.0f + 0.5f;
        sum.y = dm::fpow<Fast>(dm::gmin(dm::gmax(sum.y, 0.0f), 1.0f), 0.45f) * 255.0f + 0.5f;
        sum.z = dm::fpow<Fast>(dm::gmin(dm::gmax(sum.z, 0.0f), 1.0f), 0.45f) * 255.0f + 0.5f;
    }
    if (fin.valid && fin.sub == 0u) a.out[(size_t)fin.ty * a.W + gx] = sum;
}

template <int Fast, int S, int NS> inline int launch_pool_one(const PTArgs& a, uint32_t tile_rows, hipStream_t s) {
    dim3 grid((a.W + block_w<S>() - 1u) / block_w<S>(), (tile_rows + block_h<S>() - 1u) / block_h<S>());
    constexpr size_t lds = pool_block_lds_bytes<Fast, NS>();
    if (Fast && !a.scene.spheres_disjoint) hipLaunchKernelGGL((pathtrace_pool_kernel<Fast, S, NS, false>), grid, dim3(256), lds, s, a);
    else hipLaunchKernelGGL((pathtrace_pool_kernel<Fast, S, NS, true>), grid, dim3(256), lds, s, a);
    return MC_OK;
}
// MC_PT_KERNEL_POOL: 16 lanes per pixel and batch (the host never passes anything else); one instantiation per sphere count
template <int Fast> inline int launch_pool(const PTArgs& a, int S, uint32_t tile_rows, hipStream_t s) {
    if (S != 16) return MC_ERR_INVALID_ARGUMENT;
    return dispatch_spheres(a.scene.n_spheres, [&](auto NS) { return launch_pool_one<Fast, 16, NS>(a, tile_rows, s); });
}

// One tier's launcher (declared in pathtrace_kernel.h; instantiated by pathtrace_strict.hip / pathtrace_fast.hip / pathtrace_careful.hip).
template <int Fast> int launch_tier(const PTArgs& a, int kernel, int S, int prec, uint32_t tile_rows, hipStream_t s) {
    if (kernel == MC_PT_KERNEL_POOL) return launch_pool<Fast>(a, S, tile_rows, s);
    if (prec != 0)   // the extended-precision sphere tests: generic kernel, S = 1 or 16
        return dispatch<1, 2, 3>(prec, [&](auto P) {
            return dispatch<1, 16>(S, [&](auto W) { return launch_one<Fast, -1, -1, false, W, P>(a, tile_rows, s); });
        });
    switch (kernel) {
        case MC_PT_KERNEL_BOX:   // (fast math only)
            if constexpr (Fast != 0) return launch_slab<Fast, true>(a, S, tile_rows, s);
            return MC_ERR_INVALID_ARGUMENT;
        case MC_PT_KERNEL_SLAB: return launch_slab<Fast, false>(a, S, tile_rows, s);
        case MC_PT_KERNEL_GENERIC_MEMORY:
            return dispatch<1, 4, 16>(S, [&](auto W) { return launch_one<Fast, -2, -2, false, W, 0>(a, tile_rows, s); });
        default: return dispatch<1, 4, 16>(S, [&](auto W) { return launch_one<Fast, -1, -1, false, W, 0>(a, tile_rows, s); });
    }
}

}  // namespace pt
}  // namespace mc
