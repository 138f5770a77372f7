// Issue rate of the 32 x 32 + 64 -> 64 integer multiply-add (v_mad_u64_u32) on gfx950: the inner operation of the device orbit's product
// columns (csrc/mandel_orbit_fix.h).  Eight independent chains per lane, one and four waves per SIMD, every CU busy.
// Build: hipcc --offload-arch=gfx950 -O2 -o tools/bin/mad_u64_microbench tools/mad_u64_microbench.hip
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>

#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

constexpr int kChains = 8, kTrips = 4096;

__global__ void __launch_bounds__(256) mad_kernel(uint64_t* out, uint32_t seed) {
    uint64_t acc[kChains];
    uint32_t a[kChains];
    for (int q = 0; q < kChains; q++) { acc[q] = seed + threadIdx.x * 977u + q; a[q] = seed * (2u * q + 3u) + threadIdx.x; }
    for (int i = 0; i < kTrips; i++)
#pragma unroll
        for (int q = 0; q < kChains; q++) acc[q] = (uint64_t)a[q] * (uint32_t)(acc[q] >> 32) + acc[q];   // one v_mad_u64_u32
    uint64_t r = 0;
    for (int q = 0; q < kChains; q++) r ^= acc[q];
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = r;
}

int main() {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    printf("device %s  CUs %d\n%-8s %10s %s\n", prop.name, cus, "w/SIMD", "ms", "cycles per v_mad_u64_u32 wave-instruction per SIMD @2.4 GHz");
    uint64_t* out;
    CHECK(hipMalloc(&out, (size_t)cus * 4 * 256 * sizeof(uint64_t)));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    for (int wps : {1, 4}) {
        float best = 1e30f;
        for (int rep = 0; rep < 5; rep++) {
            CHECK(hipEventRecord(e0));
            hipLaunchKernelGGL(mad_kernel, dim3(cus * wps), dim3(256), 0, 0, out, 12345u + rep);
            CHECK(hipEventRecord(e1));
            CHECK(hipEventSynchronize(e1));
            float ms;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            if (rep && ms < best) best = ms;
        }
        const double winst = (double)cus * wps * 4.0 * kChains * kTrips;   // wave-instructions in all
        printf("%-8d %10.4f %8.3f\n", wps, best, (best * 1e-3) * 2.4e9 * (cus * 4.0) / winst);
    }
    return 0;
}
