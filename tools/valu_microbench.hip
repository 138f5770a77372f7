// VALU issue-cost surveys of gfx950 (MI355X) — ONE program, one mode per survey (rounds 1-4 kept them as four files):
//   valu_microbench classes   every opcode class in isolation (profiles/r01_valu_microbench.txt)
//   valu_microbench mix       how the issue classes combine; instructions under EXEC = 0 (profiles/r03_valu_microbench3.txt)
//   valu_microbench among     a transcendental among other instructions (profiles/r03_valu_microbench7.txt)
//   valu_microbench opcodes   every transcendental opcode, f32 and f16, alone and in a mix (profiles/r04_valu_microbench8.txt)
//   valu_microbench fp64      the fp64 rows of "classes": v_add/mul/fma_f64, v_cmp_gt_f64 — the issue cost and the fp64 peak of the
//                             MC_PRECISION_F64 Mandelbrot kernel (profiles/f64_valu_microbench.txt)
//   valu_microbench prio      a group of transcendentals issued at raised wave priority (s_setprio) against the same group at equal
//                             priority (profiles/valu_microbench_prio.txt)
//   valu_microbench ldsmov    a register filled by ds_read from a wave-uniform address against v_mov_b32 from an SGPR
//                             (profiles/valu_microbench_ldsmov.txt)
// These are the measurements the path tracer's design rests on: add / mul / fmac / mov / logic issue in ~2.3 cycles
// per wave64 instruction per SIMD, compare / select / min / max / convert / three-operand integer in ~4.2 alone but ~2.4 in a mix,
// transcendentals in ~8.2 wherever they stand.  Each mode is the former file's code, unchanged, in a namespace of its own.
// Build: hipcc --offload-arch=gfx950 -O2 -o tools/bin/valu_microbench tools/valu_microbench.hip
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// ======================================================================================================================
// mode "classes" — formerly tools/valu_microbench.hip
// VALU issue-rate microbenchmark for gfx950: measures wave-instructions per cycle per SIMD for the
// instruction classes the Mandelbrot / path-tracer kernels are made of, at several occupancies.
// Used to fix the roofline denominators in DESIGN.md (is v_pk_*_f32 2 flops/lane/issue or half rate?
// what do v_rcp/v_rsq/v_sqrt/v_sin/v_mul_lo_u32/v_cmp cost relative to v_add_f32?).
//
// Build: hipcc --offload-arch=gfx950 -O2 -o valu_microbench tools/valu_microbench.hip
namespace classes {
#define CHECK(x)                                                                     \
    do {                                                                             \
        hipError_t e = (x);                                                          \
        if (e != hipSuccess) {                                                       \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e));                   \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

constexpr int kIters = 4096;   // loop trips
constexpr int kUnroll = 16;    // instructions per trip (8 independent chains x 2)

// 8 independent accumulator chains so dependent-issue latency never limits throughput.
#define BODY1(INS)                                                                                        \
    asm volatile(INS " %0, %0, %8\n\t" INS " %1, %1, %8\n\t" INS " %2, %2, %8\n\t" INS " %3, %3, %8\n\t"  \
                 INS " %4, %4, %8\n\t" INS " %5, %5, %8\n\t" INS " %6, %6, %8\n\t" INS " %7, %7, %8\n\t"  \
                 INS " %0, %0, %8\n\t" INS " %1, %1, %8\n\t" INS " %2, %2, %8\n\t" INS " %3, %3, %8\n\t"  \
                 INS " %4, %4, %8\n\t" INS " %5, %5, %8\n\t" INS " %6, %6, %8\n\t" INS " %7, %7, %8\n\t"  \
                 : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)         \
                 : "v"(b))
#define BODY_UN(INS)                                                                                      \
    asm volatile(INS " %0, %0\n\t" INS " %1, %1\n\t" INS " %2, %2\n\t" INS " %3, %3\n\t"                  \
                 INS " %4, %4\n\t" INS " %5, %5\n\t" INS " %6, %6\n\t" INS " %7, %7\n\t"                  \
                 INS " %0, %0\n\t" INS " %1, %1\n\t" INS " %2, %2\n\t" INS " %3, %3\n\t"                  \
                 INS " %4, %4\n\t" INS " %5, %5\n\t" INS " %6, %6\n\t" INS " %7, %7\n\t"                  \
                 : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7))
#define BODY_FMA(INS)                                                                                                     \
    asm volatile(INS " %0, %0, %8, %8\n\t" INS " %1, %1, %8, %8\n\t" INS " %2, %2, %8, %8\n\t" INS " %3, %3, %8, %8\n\t"  \
                 INS " %4, %4, %8, %8\n\t" INS " %5, %5, %8, %8\n\t" INS " %6, %6, %8, %8\n\t" INS " %7, %7, %8, %8\n\t"  \
                 INS " %0, %0, %8, %8\n\t" INS " %1, %1, %8, %8\n\t" INS " %2, %2, %8, %8\n\t" INS " %3, %3, %8, %8\n\t"  \
                 INS " %4, %4, %8, %8\n\t" INS " %5, %5, %8, %8\n\t" INS " %6, %6, %8, %8\n\t" INS " %7, %7, %8, %8\n\t"  \
                 : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)                         \
                 : "v"(b))
#define BODY_CMP(INS)                                                                                                     \
    asm volatile(INS " vcc, %0, %8\n\t" INS " vcc, %1, %8\n\t" INS " vcc, %2, %8\n\t" INS " vcc, %3, %8\n\t"              \
                 INS " vcc, %4, %8\n\t" INS " vcc, %5, %8\n\t" INS " vcc, %6, %8\n\t" INS " vcc, %7, %8\n\t"              \
                 INS " vcc, %0, %8\n\t" INS " vcc, %1, %8\n\t" INS " vcc, %2, %8\n\t" INS " vcc, %3, %8\n\t"              \
                 INS " vcc, %4, %8\n\t" INS " vcc, %5, %8\n\t" INS " vcc, %6, %8\n\t" INS " vcc, %7, %8\n\t"              \
                 : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)                         \
                 : "v"(b)                                                                                                 \
                 : "vcc")

#define KERNEL32(NAME, BODY)                                                     \
    __global__ void __launch_bounds__(256) NAME(float* out, float seed) {        \
        float a0 = seed, a1 = seed + 1, a2 = seed + 2, a3 = seed + 3;            \
        float a4 = seed + 4, a5 = seed + 5, a6 = seed + 6, a7 = seed + 7;        \
        float b = seed * 0.5f + 1.0f;                                            \
        for (int i = 0; i < kIters; i++) { BODY; }                               \
        out[blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7; \
    }
typedef float float2v __attribute__((ext_vector_type(2)));
#define KERNEL64(NAME, BODY)                                                     \
    __global__ void __launch_bounds__(256) NAME(float* out, float seed) {        \
        float2v a0 = {seed, seed}, a1 = a0 + 1.f, a2 = a0 + 2.f, a3 = a0 + 3.f;  \
        float2v a4 = a0 + 4.f, a5 = a0 + 5.f, a6 = a0 + 6.f, a7 = a0 + 7.f;      \
        float2v b = a0 * 0.5f + 1.0f;                                            \
        for (int i = 0; i < kIters; i++) { BODY; }                               \
        float2v r = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;                       \
        out[blockIdx.x * blockDim.x + threadIdx.x] = r.x + r.y;                  \
    }
#define KERNELU32(NAME, BODY)                                                    \
    __global__ void __launch_bounds__(256) NAME(float* out, float seed) {        \
        unsigned a0 = (unsigned)seed, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3;     \
        unsigned a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7;             \
        unsigned b = a0 * 3u + 12345u;                                           \
        for (int i = 0; i < kIters; i++) { BODY; }                               \
        out[blockIdx.x * blockDim.x + threadIdx.x] = (float)(a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7); \
    }

KERNEL32(k_add, BODY1("v_add_f32"))
KERNEL32(k_mul, BODY1("v_mul_f32"))
KERNEL32(k_fma, BODY_FMA("v_fma_f32"))
KERNEL32(k_max, BODY1("v_max_f32"))
KERNEL32(k_cmp, BODY_CMP("v_cmp_gt_f32"))
KERNEL32(k_rcp, BODY_UN("v_rcp_f32"))
KERNEL32(k_rsq, BODY_UN("v_rsq_f32"))
KERNEL32(k_sqrt, BODY_UN("v_sqrt_f32"))
KERNEL32(k_sin, BODY_UN("v_sin_f32"))
KERNEL32(k_exp, BODY_UN("v_exp_f32"))
KERNEL32(k_log, BODY_UN("v_log_f32"))
KERNEL32(k_cvt, BODY_UN("v_cvt_f32_u32"))
KERNEL32(k_rndne, BODY_UN("v_rndne_f32"))
KERNEL64(k_pk_add, BODY1("v_pk_add_f32"))
KERNEL64(k_pk_mul, BODY1("v_pk_mul_f32"))
KERNEL64(k_pk_fma, BODY_FMA("v_pk_fma_f32"))
KERNELU32(k_mullo, BODY1("v_mul_lo_u32"))
KERNELU32(k_xor, BODY1("v_xor_b32"))
KERNELU32(k_lshr, BODY1("v_lshrrev_b32"))
KERNELU32(k_addu, BODY1("v_add_u32"))
// second series (round 1, after the fast-math contraction result): the "other" class of the issue model
#define BODY_CNDMASK                                                                                       \
    asm volatile("v_cndmask_b32 %0, %0, %8, vcc\n\tv_cndmask_b32 %1, %1, %8, vcc\n\tv_cndmask_b32 %2, %2, %8, vcc\n\t" \
                 "v_cndmask_b32 %3, %3, %8, vcc\n\tv_cndmask_b32 %4, %4, %8, vcc\n\tv_cndmask_b32 %5, %5, %8, vcc\n\t" \
                 "v_cndmask_b32 %6, %6, %8, vcc\n\tv_cndmask_b32 %7, %7, %8, vcc\n\tv_cndmask_b32 %0, %0, %8, vcc\n\t" \
                 "v_cndmask_b32 %1, %1, %8, vcc\n\tv_cndmask_b32 %2, %2, %8, vcc\n\tv_cndmask_b32 %3, %3, %8, vcc\n\t" \
                 "v_cndmask_b32 %4, %4, %8, vcc\n\tv_cndmask_b32 %5, %5, %8, vcc\n\tv_cndmask_b32 %6, %6, %8, vcc\n\t" \
                 "v_cndmask_b32 %7, %7, %8, vcc\n\t"                                                                    \
                 : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)                         \
                 : "v"(b)                                                                                                 \
                 : "vcc")
KERNELU32(k_mov, BODY_UN("v_mov_b32"))
KERNELU32(k_cndmask, BODY_CNDMASK)
KERNELU32(k_and, BODY1("v_and_b32"))
KERNEL32(k_fmac, BODY1("v_fmac_f32"))
KERNEL32(k_sub, BODY1("v_sub_f32"))
// fp64 rows: the same 8 chains x 2 on register pairs (the "v" constraint of a double is a VGPR pair)
#define KERNELF64(NAME, BODY)                                                    \
    __global__ void __launch_bounds__(256) NAME(float* out, float seed) {        \
        double a0 = seed, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3;                 \
        double a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7;               \
        double b = a0 * 0.5 + 1.0;                                               \
        for (int i = 0; i < kIters; i++) { BODY; }                               \
        out[blockIdx.x * blockDim.x + threadIdx.x] = (float)(a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7); \
    }
KERNELF64(k_add64, BODY1("v_add_f64"))
KERNELF64(k_mul64, BODY1("v_mul_f64"))
KERNELF64(k_fma64, BODY_FMA("v_fma_f64"))
KERNELF64(k_cmp64, BODY_CMP("v_cmp_gt_f64"))

struct Entry {
    const char* name;
    void (*fn)(float*, float);
    int flops_per_lane;   // flops per lane per instruction (0 for non-fp): fp32, or fp64 for the *_f64 rows
};

static int run_entries(const std::vector<Entry>& es);

static int run() {
    std::vector<Entry> es = {
        {"v_add_f32", k_add, 1},     {"v_mul_f32", k_mul, 1},       {"v_fma_f32", k_fma, 2},     {"v_max_f32", k_max, 1},
        {"v_cmp_gt_f32", k_cmp, 0},  {"v_pk_add_f32", k_pk_add, 2}, {"v_pk_mul_f32", k_pk_mul, 2}, {"v_pk_fma_f32", k_pk_fma, 4},
        {"v_rcp_f32", k_rcp, 1},     {"v_rsq_f32", k_rsq, 1},       {"v_sqrt_f32", k_sqrt, 1},   {"v_sin_f32", k_sin, 1},
        {"v_exp_f32", k_exp, 1},     {"v_log_f32", k_log, 1},       {"v_cvt_f32_u32", k_cvt, 0}, {"v_rndne_f32", k_rndne, 0},
        {"v_mul_lo_u32", k_mullo, 0}, {"v_xor_b32", k_xor, 0},      {"v_lshrrev_b32", k_lshr, 0}, {"v_add_u32", k_addu, 0},
        {"v_mov_b32", k_mov, 0},     {"v_cndmask_b32", k_cndmask, 0}, {"v_and_b32", k_and, 0},   {"v_fmac_f32", k_fmac, 2},
        {"v_sub_f32", k_sub, 1},
    };
    return run_entries(es);
}

static int run_fp64() {
    return run_entries({{"v_add_f64", k_add64, 1}, {"v_mul_f64", k_mul64, 1}, {"v_fma_f64", k_fma64, 2}, {"v_cmp_gt_f64", k_cmp64, 0},
                        {"v_add_f32", k_add, 1}});   // the fp32 row again, same run, for the ratio
}

static int run_entries(const std::vector<Entry>& es) {
    CHECK(hipSetDevice(0));
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    printf("device %s  CUs %d  clock %d kHz\n", prop.name, cus, prop.clockRate);
    float* out;
    CHECK(hipMalloc(&out, sizeof(float) * 256 * cus * 64));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    printf("%-16s %5s %10s %14s %12s %10s\n", "instr", "w/SIMD", "ms", "Gwaveinst/s", "cyc/inst@2.4", "TFLOP/s");
    for (auto& e : es) {
        for (int wps : {1, 2, 4, 8}) {
            // wps waves per SIMD: blocks of 256 threads = 4 waves = 1 wave per SIMD; launch wps blocks per CU
            int blocks = cus * wps;
            hipLaunchKernelGGL(e.fn, dim3(blocks), dim3(256), 0, 0, out, 1.0f);   // warm-up
            CHECK(hipDeviceSynchronize());
            const int reps = 5;
            CHECK(hipEventRecord(e0));
            for (int r = 0; r < reps; r++) hipLaunchKernelGGL(e.fn, dim3(blocks), dim3(256), 0, 0, out, 1.0f);
            CHECK(hipEventRecord(e1));
            CHECK(hipEventSynchronize(e1));
            float ms;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            ms /= reps;
            double winst = (double)blocks * 4 * kIters * kUnroll;           // wave-instructions
            double rate = winst / (ms * 1e-3);                              // per second, whole chip
            double per_simd_cycle = rate / (cus * 4.0) / 2.4e9;             // wave-inst per SIMD per cycle @2.4GHz
            double tflops = rate * 64.0 * e.flops_per_lane / 1e12;
            printf("%-16s %5d %10.4f %14.2f %12.3f %10.2f\n", e.name, wps, ms, rate / 1e9, 1.0 / per_simd_cycle, tflops);
        }
    }
    CHECK(hipFree(out));
    return 0;
}
}  // namespace classes
#undef CHECK
#undef BODY1
#undef BODY_UN
#undef BODY_FMA
#undef BODY_CMP
#undef KERNEL32
#undef KERNEL64
#undef KERNELU32
#undef KERNELF64
#undef BODY_CNDMASK

// ======================================================================================================================
// mode "mix" — formerly tools/valu_microbench3.hip
// Third VALU survey for gfx950: how the issue classes COMBINE.  valu_microbench{,2}.hip priced each opcode in isolation
// (add/mul/fmac/mov/logic ~2.3 cycles per wave64 instruction per SIMD, compare/select/min/max/convert/3-operand integer ~4.2,
// transcendental ~8.2).  The path tracer's measured time is well under the sum of those prices, and a rewrite that removed
// 4 % of its instructions made it slower — so: do classes overlap when they come from different waves, from one wave, and
// what does an instruction cost whose EXEC mask is empty?
namespace mix {
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)
constexpr int kIters = 2048;
#define OPS : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b), "v"(c), "s"(sm)
#define F(k) "v_add_f32_e32 %" #k ", %" #k ", %8\n\t"
#define S(k) "v_max_f32_e32 %" #k ", %" #k ", %8\n\t"
#define C(k) "v_cndmask_b32_e64 %" #k ", %" #k ", %8, %10\n\t"
#define M(k) "v_cmp_lt_f32_e64 s[20:21], %" #k ", %8\n\t"
#define T(k) "v_rcp_f32_e32 %" #k ", %" #k "\n\t"
#define I(k) "v_min_u32_e32 %" #k ", %" #k ", %8\n\t"
#define A(k) "v_and_or_b32 %" #k ", %" #k ", %8, %9\n\t"
// 16 instructions per trip on 8 independent chains
#define P_FAST   F(0) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(0) F(1) F(2) F(3) F(4) F(5) F(6) F(7)
#define P_SLOW   S(0) S(1) S(2) S(3) S(4) S(5) S(6) S(7) S(0) S(1) S(2) S(3) S(4) S(5) S(6) S(7)
#define P_SEL    C(0) C(1) C(2) C(3) C(4) C(5) C(6) C(7) C(0) C(1) C(2) C(3) C(4) C(5) C(6) C(7)
#define P_TRANS  T(0) T(1) T(2) T(3) T(4) T(5) T(6) T(7) T(0) T(1) T(2) T(3) T(4) T(5) T(6) T(7)
#define P_FS     F(0) S(1) F(2) S(3) F(4) S(5) F(6) S(7) F(1) S(0) F(3) S(2) F(5) S(4) F(7) S(6)
#define P_FC     F(0) C(1) F(2) C(3) F(4) C(5) F(6) C(7) F(1) C(0) F(3) C(2) F(5) C(4) F(7) C(6)
#define P_FM     F(0) M(1) F(2) M(3) F(4) M(5) F(6) M(7) F(1) M(0) F(3) M(2) F(5) M(4) F(7) M(6)
#define P_FFFT   F(0) F(1) F(2) T(3) F(4) F(5) F(6) T(7) F(1) F(2) F(3) T(0) F(5) F(6) F(7) T(4)
#define P_FFS    F(0) F(1) S(2) F(3) F(4) S(5) F(6) F(7) S(0) F(1) F(2) S(3) F(4) F(5) S(6) F(7)
#define P_FIA    F(0) I(1) F(2) A(3) F(4) I(5) F(6) A(7) F(1) I(0) F(3) A(2) F(5) I(4) F(7) A(6)
#define KERNEL(NAME, PAT)                                                                           \
    __global__ void __launch_bounds__(512) NAME(float* out, float seed, int mode) {                  \
        float a0 = seed, a1 = seed + 1, a2 = seed + 2, a3 = seed + 3, a4 = seed + 4, a5 = seed + 5, a6 = seed + 6, a7 = seed + 7; \
        float b = seed * 0.5f + 1.0f, c = seed * 0.25f + 2.0f;                                      \
        unsigned long long sm = 0x5555aaaa3333ccccull;                                               \
        for (int i = 0; i < kIters; i++) asm volatile(PAT OPS : "vcc", "s20", "s21");                \
        out[blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;          \
    }
KERNEL(k_fast, P_FAST) KERNEL(k_slow, P_SLOW) KERNEL(k_sel, P_SEL) KERNEL(k_trans, P_TRANS) KERNEL(k_fs, P_FS) KERNEL(k_fc, P_FC)
KERNEL(k_fm, P_FM) KERNEL(k_ffft, P_FFFT) KERNEL(k_ffs, P_FFS) KERNEL(k_fia, P_FIA)
// two programs on one SIMD: waves 0-3 of a 512-thread block run pattern X, waves 4-7 pattern Y (a block's waves go to the
// SIMDs cyclically, so wave w and wave w + 4 share one)
#define KERNEL2(NAME, PX, PY)                                                                        \
    __global__ void __launch_bounds__(512) NAME(float* out, float seed, int mode) {                   \
        float a0 = seed, a1 = seed + 1, a2 = seed + 2, a3 = seed + 3, a4 = seed + 4, a5 = seed + 5, a6 = seed + 6, a7 = seed + 7; \
        float b = seed * 0.5f + 1.0f, c = seed * 0.25f + 2.0f;                                       \
        unsigned long long sm = 0x5555aaaa3333ccccull;                                                \
        if ((threadIdx.x >> 8) == 0) { for (int i = 0; i < kIters; i++) asm volatile(PX OPS : "vcc", "s20", "s21"); } \
        else { for (int i = 0; i < kIters; i++) asm volatile(PY OPS : "vcc", "s20", "s21"); }        \
        out[blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;           \
    }
KERNEL2(k2_fast_slow, P_FAST, P_SLOW) KERNEL2(k2_fast_trans, P_FAST, P_TRANS) KERNEL2(k2_slow_trans, P_SLOW, P_TRANS)
KERNEL2(k2_fast_sel, P_FAST, P_SEL)
// EXEC = 0: the same streams issued with an empty mask
#define KERNEL0(NAME, PAT)                                                                          \
    __global__ void __launch_bounds__(512) NAME(float* out, float seed, int mode) {                  \
        float a0 = seed, a1 = seed + 1, a2 = seed + 2, a3 = seed + 3, a4 = seed + 4, a5 = seed + 5, a6 = seed + 6, a7 = seed + 7; \
        float b = seed * 0.5f + 1.0f, c = seed * 0.25f + 2.0f;                                      \
        unsigned long long sm = 0x5555aaaa3333ccccull;                                               \
        for (int i = 0; i < kIters; i++)                                                             \
            asm volatile("s_mov_b64 s[22:23], exec\n\ts_mov_b64 exec, 0\n\t" PAT "s_mov_b64 exec, s[22:23]\n\t" OPS : "vcc", "s20", "s21", "s22", "s23"); \
        out[blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;          \
    }
KERNEL0(k0_fast, P_FAST) KERNEL0(k0_slow, P_SLOW) KERNEL0(k0_sel, P_SEL) KERNEL0(k0_trans, P_TRANS)
struct Entry { const char* name; void (*fn)(float*, float, int); };
static int run() {
    CHECK(hipSetDevice(0));
    hipDeviceProp_t prop; CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    float* out; CHECK(hipMalloc(&out, sizeof(float) * 512 * cus * 8));
    std::vector<Entry> es = {
        {"fast  (v_add_f32) x16", k_fast}, {"slow  (v_max_f32) x16", k_slow}, {"sel   (v_cndmask sgpr) x16", k_sel}, {"trans (v_rcp_f32) x16", k_trans},
        {"one wave: F S F S ...", k_fs}, {"one wave: F C F C ... (cndmask)", k_fc}, {"one wave: F M F M ... (v_cmp->sgpr)", k_fm},
        {"one wave: F F F T ...", k_ffft}, {"one wave: F F S ...", k_ffs}, {"one wave: F min_u32 F and_or ...", k_fia},
        {"two waves/SIMD: fast | slow", k2_fast_slow}, {"two waves/SIMD: fast | trans", k2_fast_trans},
        {"two waves/SIMD: slow | trans", k2_slow_trans}, {"two waves/SIMD: fast | sel", k2_fast_sel},
        {"EXEC=0 fast x16", k0_fast}, {"EXEC=0 slow x16", k0_slow}, {"EXEC=0 sel x16", k0_sel}, {"EXEC=0 trans x16", k0_trans},
    };
    hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    for (int wps : {2, 4, 6}) {   // waves per SIMD: 512-thread blocks, 1 / 2 / 3 blocks per CU
        printf("---- %d waves per SIMD\n%-40s %10s %s\n", wps, "stream", "ms", "cycles per wave-instruction per SIMD @2.4 GHz");
        for (auto& e : es) {
            const int blocks = cus * (wps / 2);
            hipLaunchKernelGGL(e.fn, dim3(blocks), dim3(512), 0, 0, out, 1.0f, 0); CHECK(hipDeviceSynchronize());
            CHECK(hipEventRecord(e0));
            for (int r = 0; r < 5; r++) hipLaunchKernelGGL(e.fn, dim3(blocks), dim3(512), 0, 0, out, 1.0f, 0);
            CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1));
            float ms; CHECK(hipEventElapsedTime(&ms, e0, e1)); ms /= 5;
            const double winst = (double)blocks * 8 * kIters * 16;
            printf("%-40s %10.4f %8.3f\n", e.name, ms, (ms * 1e-3) * 2.4e9 * (cus * 4.0) / winst);
        }
    }
    return 0;
}
}  // namespace mix
#undef CHECK
#undef OPS
#undef F
#undef S
#undef C
#undef M
#undef T
#undef I
#undef A
#undef P_FAST
#undef P_SLOW
#undef P_SEL
#undef P_TRANS
#undef P_FS
#undef P_FC
#undef P_FM
#undef P_FFFT
#undef P_FFS
#undef P_FIA
#undef KERNEL
#undef KERNEL2
#undef KERNEL0

// ======================================================================================================================
// mode "among" — formerly tools/valu_microbench7.hip
// Seventh VALU survey for gfx950: does it matter WHERE the transcendentals of a stream sit?  valu_microbench3 measured a lone
// v_rcp_f32 among adds at ~11.6 cycles (F F F T: 4.7 per instruction) against 8.2 in a stream of its own — is the difference a
// price per SWITCH between the two pipes (then grouping the transcendentals of a block back to back pays), and does the
// dependency of the next instruction on the transcendental's result matter?
namespace among {
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)
constexpr int kIters = 2048;
#define OPS : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b), "v"(c), "s"(sm)
#define F(k) "v_add_f32_e32 %" #k ", %" #k ", %8\n\t"
#define S(k) "v_max_f32_e32 %" #k ", %" #k ", %8\n\t"
#define C(k) "v_cndmask_b32_e64 %" #k ", %" #k ", %8, %10\n\t"
#define M(k) "v_cmp_lt_f32_e64 s[20:21], %" #k ", %8\n\t"
#define T(k) "v_rcp_f32_e32 %" #k ", %" #k "\n\t"
#define I(k) "v_min_u32_e32 %" #k ", %" #k ", %8\n\t"
#define A(k) "v_and_or_b32 %" #k ", %" #k ", %8, %9\n\t"
#define Q(k) "v_sqrt_f32_e32 %" #k ", %" #k "\n\t"
// 16 instructions per trip: 12 adds + 4 transcendentals, differently placed (8 independent chains)
#define P_FFFT   F(0) F(1) F(2) T(3) F(4) F(5) F(6) T(7) F(1) F(2) F(3) T(0) F(5) F(6) F(7) T(4)
#define P_PAIR   F(0) F(1) F(2) F(3) F(4) F(5) T(6) T(7) F(0) F(1) F(2) F(3) F(6) F(7) T(4) T(5)
#define P_QUAD   F(0) F(1) F(2) F(3) F(0) F(1) F(2) F(3) F(0) F(1) F(2) F(3) T(4) T(5) T(6) T(7)
#define P_QUADQ  F(0) F(1) F(2) F(3) F(0) F(1) F(2) F(3) F(0) F(1) F(2) F(3) T(4) Q(5) T(6) Q(7)
// the instruction after a transcendental uses its result at once / the transcendental uses the result of the add before it
#define P_DEP    F(0) F(1) T(2) F(2) F(4) F(5) T(6) F(6) F(1) F(0) T(3) F(3) F(5) F(4) T(7) F(7)
#define P_DEPIN  F(0) F(1) F(2) T(2) F(4) F(5) F(6) T(6) F(1) F(0) F(3) T(3) F(5) F(4) F(7) T(7)
// 8 + 8, 14 + 2
#define P_FT     F(0) T(1) F(2) T(3) F(4) T(5) F(6) T(7) F(1) T(0) F(3) T(2) F(5) T(4) F(7) T(6)
#define P_F7T    F(0) F(1) F(2) F(3) F(4) F(5) F(6) T(7) F(0) F(1) F(2) F(3) F(4) F(5) F(7) T(6)
#define P_F14TT  F(0) F(1) F(2) F(3) F(4) F(5) F(0) F(1) F(2) F(3) F(4) F(5) F(0) F(1) T(6) T(7)
// slow-class neighbours: S S S T
#define P_SSST   S(0) S(1) S(2) T(3) S(4) S(5) S(6) T(7) S(1) S(2) S(3) T(0) S(5) S(6) S(7) T(4)
#define P_FAST   F(0) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(0) F(1) F(2) F(3) F(4) F(5) F(6) F(7)
#define P_TRANS  T(0) T(1) T(2) T(3) T(4) T(5) T(6) T(7) T(0) T(1) T(2) T(3) T(4) T(5) T(6) T(7)
#define KERNEL(NAME, PAT)                                                                           \
    __global__ void __launch_bounds__(512) NAME(float* out, float seed, int mode) {                  \
        float a0 = seed, a1 = seed + 1, a2 = seed + 2, a3 = seed + 3, a4 = seed + 4, a5 = seed + 5, a6 = seed + 6, a7 = seed + 7; \
        float b = seed * 0.5f + 1.0f, c = seed * 0.25f + 2.0f;                                      \
        unsigned long long sm = 0x5555aaaa3333ccccull;                                               \
        for (int i = 0; i < kIters; i++) asm volatile(PAT OPS : "vcc", "s20", "s21");                \
        out[blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;          \
    }
KERNEL(k_fast, P_FAST) KERNEL(k_trans, P_TRANS) KERNEL(k_ffft, P_FFFT) KERNEL(k_pair, P_PAIR) KERNEL(k_quad, P_QUAD) KERNEL(k_quadq, P_QUADQ)
KERNEL(k_dep, P_DEP) KERNEL(k_depin, P_DEPIN) KERNEL(k_ft, P_FT) KERNEL(k_f7t, P_F7T) KERNEL(k_f14tt, P_F14TT) KERNEL(k_ssst, P_SSST)
struct Entry { const char* name; void (*fn)(float*, float, int); };
static int run() {
    CHECK(hipSetDevice(0));
    hipDeviceProp_t prop; CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    float* out; CHECK(hipMalloc(&out, sizeof(float) * 512 * cus * 8));
    std::vector<Entry> es = {
        {"F x16", k_fast}, {"T x16", k_trans}, {"(F F F T) x4        12 F + 4 T, lone", k_ffft}, {"(F x6 T T) x2       12 F + 4 T, pairs", k_pair},
        {"F x12 T x4          12 F + 4 T, one group", k_quad}, {"F x12 rcp sqrt rcp sqrt", k_quadq},
        {"F F T F(dep) ...    result used at once", k_dep}, {"F F F(dep) T ...    operand just made", k_depin},
        {"(F T) x8", k_ft}, {"(F x7 T) x2", k_f7t}, {"F x14 T T", k_f14tt}, {"(S S S T) x4", k_ssst},
    };
    hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    for (int wps : {2, 4, 6}) {   // waves per SIMD: 512-thread blocks, 1 / 2 / 3 blocks per CU
        printf("---- %d waves per SIMD\n%-40s %10s %s\n", wps, "stream", "ms", "cycles per wave-instruction per SIMD @2.4 GHz");
        for (auto& e : es) {
            const int blocks = cus * (wps / 2);
            hipLaunchKernelGGL(e.fn, dim3(blocks), dim3(512), 0, 0, out, 1.0f, 0); CHECK(hipDeviceSynchronize());
            CHECK(hipEventRecord(e0));
            for (int r = 0; r < 5; r++) hipLaunchKernelGGL(e.fn, dim3(blocks), dim3(512), 0, 0, out, 1.0f, 0);
            CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1));
            float ms; CHECK(hipEventElapsedTime(&ms, e0, e1)); ms /= 5;
            const double winst = (double)blocks * 8 * kIters * 16;
            printf("%-40s %10.4f %8.3f\n", e.name, ms, (ms * 1e-3) * 2.4e9 * (cus * 4.0) / winst);
        }
    }
    return 0;
}
}  // namespace among
#undef CHECK
#undef OPS
#undef F
#undef S
#undef C
#undef M
#undef T
#undef I
#undef A
#undef Q
#undef P_FFFT
#undef P_PAIR
#undef P_QUAD
#undef P_QUADQ
#undef P_DEP
#undef P_DEPIN
#undef P_FT
#undef P_F7T
#undef P_F14TT
#undef P_SSST
#undef P_FAST
#undef P_TRANS
#undef KERNEL

// ======================================================================================================================
// mode "opcodes" — formerly tools/valu_microbench8.hip
// Eighth VALU survey for gfx950 (round 4): which transcendental opcodes cost what?  The fast path tracer spends 24 % of its time on
// 4.9 % of its instructions (profiles/r04_no_trans_pmc.txt: 13.2 cycles per transcendental among other instructions).  Rounds 1-3
// only timed v_rcp_f32 / v_sqrt_f32; this one times every opcode the kernels use or could use — v_rcp, v_rsq, v_sqrt, v_sin, v_cos,
// v_exp, v_log in f32 and the f16 forms — alone (16 per trip) and as 4 among 12 v_fmac_f32 (the in-kernel situation), at 6 waves per SIMD.
// If an f16 form or exp / log were markedly cheaper, a seed + Newton step could replace an f32 transcendental.
namespace opcodes {
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)
constexpr int kIters = 2048;
#define OPS : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b), "v"(c)
#define F(k) "v_fmac_f32_e32 %" #k ", %8, %9\n\t"
#define ALONE(OP) OP(0) OP(1) OP(2) OP(3) OP(4) OP(5) OP(6) OP(7) OP(0) OP(1) OP(2) OP(3) OP(4) OP(5) OP(6) OP(7)
#define MIXED(OP) F(0) F(1) F(2) OP(3) F(4) F(5) F(6) OP(7) F(1) F(2) F(3) OP(0) F(5) F(6) F(7) OP(4)
#define KERNEL(NAME, PAT)                                                                           \
    __global__ void __launch_bounds__(512) NAME(float* out, float seed) {                            \
        float a0 = seed, a1 = seed + 1, a2 = seed + 2, a3 = seed + 3, a4 = seed + 4, a5 = seed + 5, a6 = seed + 6, a7 = seed + 7; \
        float b = seed * 1e-6f, c = seed * 0.25f + 2.0f;                                             \
        for (int i = 0; i < kIters; i++) asm volatile(PAT OPS);                                      \
        out[blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;          \
    }
#define DEF(tag, insn)                                                              \
    _Pragma("clang diagnostic push")                                                \
    KERNEL(k_##tag##_alone, ALONE(T_##tag)) KERNEL(k_##tag##_mixed, MIXED(T_##tag)) \
    _Pragma("clang diagnostic pop")
#define T_rcp32(k) "v_rcp_f32_e32 %" #k ", %" #k "\n\t"
#define T_rsq32(k) "v_rsq_f32_e32 %" #k ", %" #k "\n\t"
#define T_sqrt32(k) "v_sqrt_f32_e32 %" #k ", %" #k "\n\t"
#define T_sin32(k) "v_sin_f32_e32 %" #k ", %" #k "\n\t"
#define T_cos32(k) "v_cos_f32_e32 %" #k ", %" #k "\n\t"
#define T_exp32(k) "v_exp_f32_e32 %" #k ", %" #k "\n\t"
#define T_log32(k) "v_log_f32_e32 %" #k ", %" #k "\n\t"
#define T_rcp16(k) "v_rcp_f16_e32 %" #k ", %" #k "\n\t"
#define T_rsq16(k) "v_rsq_f16_e32 %" #k ", %" #k "\n\t"
#define T_sqrt16(k) "v_sqrt_f16_e32 %" #k ", %" #k "\n\t"
#define T_sin16(k) "v_sin_f16_e32 %" #k ", %" #k "\n\t"
#define T_exp16(k) "v_exp_f16_e32 %" #k ", %" #k "\n\t"
#define T_fma(k) "v_fmac_f32_e32 %" #k ", %8, %9\n\t"
#define T_cvt(k) "v_cvt_f16_f32_e32 %" #k ", %" #k "\n\t"
DEF(rcp32, ) DEF(rsq32, ) DEF(sqrt32, ) DEF(sin32, ) DEF(cos32, ) DEF(exp32, ) DEF(log32, )
DEF(rcp16, ) DEF(rsq16, ) DEF(sqrt16, ) DEF(sin16, ) DEF(exp16, ) DEF(fma, ) DEF(cvt, )
struct Entry { const char* name; void (*alone)(float*, float); void (*mixed)(float*, float); };
static int run() {
    CHECK(hipSetDevice(0));
    hipDeviceProp_t prop; CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    float* out; CHECK(hipMalloc(&out, sizeof(float) * 512 * cus * 8));
#define E(tag) {#tag, k_##tag##_alone, k_##tag##_mixed}
    std::vector<Entry> es = {E(fma), E(cvt), E(rcp32), E(rsq32), E(sqrt32), E(sin32), E(cos32), E(exp32), E(log32), E(rcp16), E(rsq16), E(sqrt16), E(sin16), E(exp16)};
    hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    const int wps = 6, blocks = cus * (wps / 2);
    auto time = [&](void (*fn)(float*, float)) {
        hipLaunchKernelGGL(fn, dim3(blocks), dim3(512), 0, 0, out, 1.0f); CHECK(hipDeviceSynchronize());
        CHECK(hipEventRecord(e0));
        for (int r = 0; r < 5; r++) hipLaunchKernelGGL(fn, dim3(blocks), dim3(512), 0, 0, out, 1.0f);
        CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1));
        float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
        return (double)ms / 5;
    };
    const double winst = (double)blocks * 8 * kIters * 16;
    const double fma_alone = time(k_fma_alone) * 1e-3 * 2.4e9 * (cus * 4.0) / winst;
    printf("%d waves per SIMD; cycles per wave-instruction per SIMD @2.4 GHz.  'in a mix' = cost of ONE such instruction among v_fmac_f32 (4 per 12 fmac),\n"
           "i.e. (16 x mixed - 12 x fmac) / 4\n%-10s %12s %12s\n", wps, "opcode", "alone", "in a mix");
    for (auto& e : es) {
        const double a = time(e.alone) * 1e-3 * 2.4e9 * (cus * 4.0) / winst, m = time(e.mixed) * 1e-3 * 2.4e9 * (cus * 4.0) / winst;
        printf("%-10s %12.3f %12.3f\n", e.name, a, (16.0 * m - 12.0 * fma_alone) / 4.0);
    }
    return 0;
}
}  // namespace opcodes
#undef CHECK
#undef OPS
#undef F
#undef ALONE
#undef MIXED
#undef KERNEL
#undef DEF
#undef T_rcp32
#undef T_rsq32
#undef T_sqrt32
#undef T_sin32
#undef T_cos32
#undef T_exp32
#undef T_log32
#undef T_rcp16
#undef T_rsq16
#undef T_sqrt16
#undef T_sin16
#undef T_exp16
#undef T_fma
#undef T_cvt
#undef E

// ======================================================================================================================
// mode "prio" — does a wave that raises its priority get its transcendentals issued back to back?
// "among" found that a transcendental among other instructions costs 11.5-12.7 cycles against 8.1 in a stream of its own, and that
// putting a wave's four transcendentals next to each other changes nothing — but there six waves of EQUAL priority interleave on the
// SIMD, so the group is not back to back in the SIMD's issue order.  Here the group of n = 2, 4, 7 independent transcendentals
// (v_rsq / v_sqrt / v_sin / v_cos mixed as the path tracer's bounce mixes them) behind 12 v_add_f32 is issued once as it stands and
// once bracketed by s_setprio 3 ... s_setprio 0, at 6 and 7 waves per SIMD, with all waves in phase and with every wave started
// (wave id mod 13) adds late, as resident waves of the pool kernel are.  Cycles per transcendental = (trip - 12 x the F-only rate) / n.
namespace prio {
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)
constexpr int kIters = 2048;
#define OPS : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b)
#define F(k) "v_add_f32_e32 %" #k ", %" #k ", %8\n\t"
#define R(k) "v_rsq_f32_e32 %" #k ", %" #k "\n\t"
#define Q(k) "v_sqrt_f32_e32 %" #k ", %" #k "\n\t"
#define N(k) "v_sin_f32_e32 %" #k ", %" #k "\n\t"
#define O(k) "v_cos_f32_e32 %" #k ", %" #k "\n\t"
#define UP "s_setprio 3\n\t"
#define DOWN "s_setprio 0\n\t"
// (the loop's scalar instructions stand between a trip's last transcendental and the next trip's first add, and no add reads the
// transcendental directly before it: the wait state a transcendental's result needs is covered in every pattern)
#define P_F12   F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(1) F(2) F(3) F(4) F(0)
#define P_F16    F(0) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(0) F(1) F(2) F(3) F(4) F(5) F(6) F(7)
#define G2       N(1) O(2)
#define G4       R(1) Q(2) N(3) O(4)
#define G7       R(1) N(2) O(3) Q(4) N(5) O(6) Q(7)
// the same instructions with every transcendental alone: what the kernel pays today
#define P_LONE2  F(1) F(2) F(3) F(4) F(5) F(0) N(1) F(6) F(7) F(3) F(4) F(5) F(0) O(2)
#define P_LONE4  F(5) F(6) F(0) R(1) F(7) F(5) F(0) Q(2) F(6) F(7) F(0) N(3) F(5) F(6) F(0) O(4)
#define KERNEL(NAME, PAT)                                                                           \
    __global__ void __launch_bounds__(256) NAME(float* out, float seed, int dephase) {               \
        float a0 = seed, a1 = seed + 1, a2 = seed + 2, a3 = seed + 3, a4 = seed + 4, a5 = seed + 5, a6 = seed + 6, a7 = seed + 7; \
        float b = seed * 0.5f + 1.0f;                                                               \
        const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6))); \
        for (int j = dephase ? wave % 13 : 0; j > 0; j--) asm volatile(F(0) OPS);                   \
        for (int i = 0; i < kIters; i++) asm volatile(PAT OPS);                                     \
        out[blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;          \
    }
KERNEL(k_f16, P_F16)
KERNEL(k_g2, P_F12 G2) KERNEL(k_g2p, P_F12 UP G2 DOWN) KERNEL(k_l2, P_LONE2)
KERNEL(k_g4, P_F12 G4) KERNEL(k_g4p, P_F12 UP G4 DOWN) KERNEL(k_l4, P_LONE4)
KERNEL(k_g7, P_F12 G7) KERNEL(k_g7p, P_F12 UP G7 DOWN)
struct Entry { const char* name; void (*fn)(float*, float, int); int n; };
static int run() {
    CHECK(hipSetDevice(0));
    hipDeviceProp_t prop; CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    float* out; CHECK(hipMalloc(&out, sizeof(float) * 256 * cus * 8));
    std::vector<Entry> es = {
        {"F x12, sin / F x6 cos ... lone", k_l2, 2}, {"F x12 (sin cos)", k_g2, 2}, {"F x12 prio3 (sin cos) prio0", k_g2p, 2},
        {"(F F F T) x4          lone", k_l4, 4}, {"F x12 (rsq sqrt sin cos)", k_g4, 4}, {"F x12 prio3 (rsq sqrt sin cos) prio0", k_g4p, 4},
        {"F x12 (rsq sin cos sqrt sin cos sqrt)", k_g7, 7}, {"F x12 prio3 (the same seven) prio0", k_g7p, 7},
    };
    hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    printf("cycles per SIMD @2.4 GHz; trip = one wave's pass over the pattern x waves per SIMD (the SIMD's time per trip of one wave);\n"
           "per T = (trip - 12 x F) / n with F from the F x16 row of the same block; three timings of five launches each: min .. max\n");
    for (int wps : {6, 7}) {   // 256-thread blocks (one wave per SIMD each), wps blocks per CU
        const int blocks = cus * wps;
        // cycles one SIMD spends on one trip of one of its waves
        auto trip = [&](void (*fn)(float*, float, int), int dephase, double* lo, double* hi) {
            hipLaunchKernelGGL(fn, dim3(blocks), dim3(256), 0, 0, out, 1.0f, dephase); CHECK(hipDeviceSynchronize());
            *lo = 1e30; *hi = 0;
            for (int t = 0; t < 3; t++) {
                CHECK(hipEventRecord(e0));
                for (int r = 0; r < 5; r++) hipLaunchKernelGGL(fn, dim3(blocks), dim3(256), 0, 0, out, 1.0f, dephase);
                CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1));
                float ms; CHECK(hipEventElapsedTime(&ms, e0, e1)); ms /= 5;
                const double c = (ms * 1e-3) * 2.4e9 / ((double)wps * kIters);
                if (c < *lo) *lo = c;
                if (c > *hi) *hi = c;
            }
        };
        for (int dephase : {0, 1}) {
            double flo, fhi; trip(k_f16, dephase, &flo, &fhi);
            const double f = 0.5 * (flo + fhi) / 16.0;
            printf("---- %d waves per SIMD, %s\n%-40s %17s %s\n", wps, dephase ? "waves de-phased by (wave id mod 13) adds" : "waves in phase",
                   "stream", "trip", "per T");
            printf("%-40s %8.2f..%7.2f   F = %.3f per instruction\n", "F x16", flo, fhi, f);
            for (auto& e : es) {
                double lo, hi; trip(e.fn, dephase, &lo, &hi);
                printf("%-40s %8.2f..%7.2f %7.2f..%5.2f\n", e.name, lo, hi, (lo - 12.0 * f) / e.n, (hi - 12.0 * f) / e.n);
            }
        }
    }
    return 0;
}
}  // namespace prio
#undef CHECK
#undef OPS
#undef F
#undef R
#undef Q
#undef N
#undef O
#undef UP
#undef DOWN
#undef P_F12
#undef P_F16
#undef G2
#undef G4
#undef G7
#undef P_LONE2
#undef P_LONE4
#undef KERNEL

// ======================================================================================================================
// mode "ldsmov" — what does a register filled from LDS cost a SIMD against the same register filled by v_mov_b32 from an SGPR?
// The pool kernel's stash pick-up and its plane test write wave-uniform values into vector registers with v_mov_b32: VALU issue
// slots that compute nothing, in a kernel bound by VALU issue whose LDS pipe is idle.  A trip is 12 independent v_add_f32 plus
//   four v_mov_b32 from SGPRs                 against   one ds_read_b128 from a wave-uniform address (a broadcast: no bank conflict),
//   three v_mov_b32                           against   one ds_read_b96,
// the load once issued in front of the adds with its s_waitcnt lgkmcnt(0) behind them (latency covered by the wave's own adds) and
// once directly in front of its s_waitcnt (covered by the other waves only), at 6 and 7 waves per SIMD.  Cost of one v_mov =
// (trip with n moves - trip of the 12 adds) / n; the load form's saving = trip with moves - trip with the load.
namespace ldsmov {
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)
constexpr int kIters = 2048;
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f3 __attribute__((ext_vector_type(3)));
#define F(k, B) "v_add_f32_e32 %" #k ", %" #k ", %" #B "\n\t"
#define P_F12(B) F(1, B) F(2, B) F(3, B) F(4, B) F(5, B) F(6, B) F(7, B) F(1, B) F(2, B) F(3, B) F(4, B) F(0, B)
#define WAIT "s_waitcnt lgkmcnt(0)\n\t"
#define ADDS : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b)
// BODY: one trip.  m: the registers filled (summed into the result after the loop, so that the last trip's fill is live).
#define KERNEL(NAME, BODY)                                                                          \
    __global__ void __launch_bounds__(256) NAME(float* out, float seed) {                            \
        __shared__ __attribute__((aligned(16))) float row[8];                                        \
        if (threadIdx.x < 8u) row[threadIdx.x] = seed + (float)threadIdx.x;                          \
        __syncthreads();                                                                             \
        float a0 = seed, a1 = seed + 1, a2 = seed + 2, a3 = seed + 3, a4 = seed + 4, a5 = seed + 5, a6 = seed + 6, a7 = seed + 7; \
        float b = seed * 0.5f + 1.0f;                                                               \
        const unsigned addr = (unsigned)(size_t)row;   /* wave-uniform LDS byte address, in a vector register */ \
        const int sb = __float_as_int(seed), s0 = __builtin_amdgcn_readfirstlane(sb + 8), s1 = __builtin_amdgcn_readfirstlane(sb + 9), s2 = __builtin_amdgcn_readfirstlane(sb + 10), s3 = __builtin_amdgcn_readfirstlane(sb + 11); \
        f4 m = {0, 0, 0, 0}; f3 m3 = {0, 0, 0}; float q0 = 0, q1 = 0, q2 = 0, q3 = 0;                                                     \
        for (int i = 0; i < kIters; i++) { BODY; }                                                   \
        out[blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7 + m.x + m.y + m.z + m.w + m3.x + m3.y + m3.z + q0 + q1 + q2 + q3 + addr + (float)(s0 + s1 + s2 + s3); \
    }
KERNEL(k_f12, asm volatile(P_F12(8) ADDS))
KERNEL(k_f16, asm volatile(P_F12(8) F(5, 8) F(6, 8) F(7, 8) F(0, 8) ADDS))
#define FILL(M) : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7), "+v"(M)
#define MOVS : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7), "+v"(q0), "+v"(q1), "+v"(q2), "+v"(q3) : "v"(b), "s"(s0), "s"(s1), "s"(s2), "s"(s3)
KERNEL(k_mov4, asm volatile(P_F12(12) "v_mov_b32 %8, %13\n\tv_mov_b32 %9, %14\n\tv_mov_b32 %10, %15\n\tv_mov_b32 %11, %16\n\t" MOVS))
KERNEL(k_mov3, asm volatile(P_F12(12) "v_mov_b32 %8, %13\n\tv_mov_b32 %9, %14\n\tv_mov_b32 %10, %15\n\t" MOVS))
KERNEL(k_lds128_early, asm volatile("ds_read_b128 %8, %10\n\t" P_F12(9) WAIT FILL(m) : "v"(b), "v"(addr) : "memory"))
KERNEL(k_lds128_late, asm volatile(P_F12(9) "ds_read_b128 %8, %10\n\t" WAIT FILL(m) : "v"(b), "v"(addr) : "memory"))
KERNEL(k_lds96_early, asm volatile("ds_read_b96 %8, %10\n\t" P_F12(9) WAIT FILL(m3) : "v"(b), "v"(addr) : "memory"))
KERNEL(k_lds96_late, asm volatile(P_F12(9) "ds_read_b96 %8, %10\n\t" WAIT FILL(m3) : "v"(b), "v"(addr) : "memory"))
struct Entry { const char* name; void (*fn)(float*, float); };
static int run() {
    CHECK(hipSetDevice(0));
    hipDeviceProp_t prop; CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    float* out; CHECK(hipMalloc(&out, sizeof(float) * 256 * cus * 8));
    std::vector<Entry> es = {
        {"F x12", k_f12}, {"F x16", k_f16}, {"F x12, v_mov x4 (sgpr)", k_mov4}, {"ds_read_b128, F x12, wait", k_lds128_early},
        {"F x12, ds_read_b128, wait", k_lds128_late}, {"F x12, v_mov x3 (sgpr)", k_mov3}, {"ds_read_b96, F x12, wait", k_lds96_early},
        {"F x12, ds_read_b96, wait", k_lds96_late},
    };
    hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    printf("cycles per SIMD @2.4 GHz per trip of one wave (time x clock / (waves per SIMD x trips)); three timings of five launches: min .. max\n");
    for (int wps : {6, 7}) {   // 256-thread blocks (one wave per SIMD each), wps blocks per CU
        const int blocks = cus * wps;
        printf("---- %d waves per SIMD\n%-32s %17s\n", wps, "trip", "cycles");
        std::vector<double> mid;
        for (auto& e : es) {
            hipLaunchKernelGGL(e.fn, dim3(blocks), dim3(256), 0, 0, out, 1.0f); CHECK(hipDeviceSynchronize());
            double lo = 1e30, hi = 0;
            for (int t = 0; t < 3; t++) {
                CHECK(hipEventRecord(e0));
                for (int r = 0; r < 5; r++) hipLaunchKernelGGL(e.fn, dim3(blocks), dim3(256), 0, 0, out, 1.0f);
                CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1));
                float ms; CHECK(hipEventElapsedTime(&ms, e0, e1)); ms /= 5;
                const double c = (ms * 1e-3) * 2.4e9 / ((double)wps * kIters);
                if (c < lo) lo = c;
                if (c > hi) hi = c;
            }
            mid.push_back(0.5 * (lo + hi));
            printf("%-32s %8.2f..%7.2f\n", e.name, lo, hi);
        }
        const double mov4 = (mid[2] - mid[0]) / 4.0, mov3 = (mid[5] - mid[0]) / 3.0;
        printf("one v_mov: %.3f (of four), %.3f (of three); F: %.3f\n", mov4, mov3, (mid[1] - mid[0]) / 4.0);
        printf("ds_read_b128 for four moves saves %.2f (early) %.2f (late) cycles per trip; gate: at least %.2f\n", mid[2] - mid[3], mid[2] - mid[4], 2.0 * mov4);
        printf("ds_read_b96 for three moves saves %.2f (early) %.2f (late) cycles per trip; half of three moves: %.2f\n", mid[5] - mid[6], mid[5] - mid[7], 1.5 * mov3);
    }
    return 0;
}
}  // namespace ldsmov
#undef CHECK
#undef F
#undef P_F12
#undef WAIT
#undef ADDS
#undef FILL
#undef MOVS
#undef KERNEL

int main(int argc, char** argv) {
    const std::string m = argc > 1 ? argv[1] : "";
    if (m == "prio") return prio::run();
    if (m == "ldsmov") return ldsmov::run();
    if (m == "classes") return classes::run();
    if (m == "mix") return mix::run();
    if (m == "among") return among::run();
    if (m == "opcodes") return opcodes::run();
    if (m == "fp64") return classes::run_fp64();
    fprintf(stderr, "usage: valu_microbench classes | mix | among | opcodes | fp64 | prio | ldsmov\n");
    return 2;
}
