// Helper kernels of tools/mandel_equalise_probe.py (never part of the library): what the histogram kernel is measured against.
//   probe_read_pass        the floor: a plain 16-B-per-lane read-only pass over the plane (every word ORed, one word stored per wave at the
//                          end so that the loads stay), grid-stride, 8 blocks of 256 per CU as the library's kernel
//   probe_naive_histogram  one atomicAdd per pixel on the global table: what the wave combining and the LDS table buy
// Built into tools/bin/libmandel_equalise_probe.so:
//   hipcc --offload-arch=gfx950 -O3 -shared -fPIC -o tools/bin/libmandel_equalise_probe.so tools/mandel_equalise_probe.hip
#include <hip/hip_runtime.h>

#include <cstdint>

__global__ void __launch_bounds__(256) read_pass_kernel(const uint4* __restrict__ in, uint64_t nvec, uint32_t* __restrict__ sink) {
    uint32_t acc = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nvec; i += (uint64_t)gridDim.x * 256u) {
        const uint4 q = in[i];
        acc |= q.x | q.y | q.z | q.w;
    }
    if (acc == 0xdeadbeefu) sink[blockIdx.x] = acc;   // (never for count planes: keeps the loads alive)
}

template <class T>
__global__ void __launch_bounds__(256) naive_histogram_kernel(const T* __restrict__ in, uint64_t n, uint32_t max_iter,
                                                              uint32_t* __restrict__ hist) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        uint32_t v = (uint32_t)in[i];
        if (v > max_iter) v = max_iter;
        atomicAdd(hist + v, 1u);
    }
}

extern "C" {

int probe_read_pass(const void* d_in, uint64_t bytes, void* d_sink, int blocks, void* stream) {
    hipLaunchKernelGGL(read_pass_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const uint4*)d_in, bytes / 16u,
                       (uint32_t*)d_sink);
    return (int)hipGetLastError();
}

int probe_naive_histogram(const void* d_in, uint32_t iters_bytes, uint64_t n, uint32_t max_iter, void* d_hist, int blocks, void* stream) {
    if (iters_bytes == 2u)
        hipLaunchKernelGGL(naive_histogram_kernel<uint16_t>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)d_in,
                           n, max_iter, (uint32_t*)d_hist);
    else
        hipLaunchKernelGGL(naive_histogram_kernel<uint32_t>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)d_in,
                           n, max_iter, (uint32_t*)d_hist);
    return (int)hipGetLastError();
}

}  // extern "C"
