// mc_mandelbrot_exact_counts_device: the exact counts of sampled pixels on the device (include/mc_compute.h).
//
//  * the host checks the arguments and builds every pixel's c (exact_prepare, mandel_orbit.cpp); nothing is launched before that.
//  * n <= 16 limbs: mandel_exact_wave_kernel, one pixel per wave in a block of ONE wave, the phases of mandel_exact_fix.h with a barrier
//    after each (a one-wave block's barrier orders that wave's LDS traffic; waves leave the loop at different iterations freely).
//  * n >= 17 limbs: mandel_exact_group_kernel, one pixel per workgroup of 1024 threads, the phases of mandel_orbit_fix.h.
//  * iterations run in slices.  Between launches a pixel's state lives in device memory (the workgroup kernel's in the layout of
//    mandel_orbit_device.hip); the host reads one status / count word per pixel after each launch and stops when none is running.  A
//    finished pixel's block returns at once.
#include <cstring>
#include <new>
#include <vector>

#include "mandel_exact.h"
#include "mandel_exact_fix.h"
#include "mandel_perturb.h"
#include "mandel_side_record.h"
#include "mc_internal.h"

namespace mc {

using namespace orbitfix;
using namespace exactfix;

namespace {

// The workgroup kernel's state: mandel_orbit_device.hip's, in 32-bit words: a header, then seven numbers of kHalfPad half-limbs.
constexpr int kStJ = 1, kStNeg = 2 /* 5 words */, kStHeader = 8;   // (word 0, the orbit's status, stays 0: the count word tells)
constexpr int kStWords = kStHeader + 7 * kHalfPad;
// The wave kernel's: the same header (no status: the count word tells), then seven numbers of kWaveHalf half-limbs.
constexpr int kWStWords = kStHeader + 7 * kWaveHalf;

__global__ void __launch_bounds__(kWaveLanes) mandel_exact_wave_kernel(uint32_t* __restrict__ state, uint32_t* __restrict__ done, int n,
                                                                       uint32_t iters, uint32_t max_iter) {
    __shared__ WaveMem m;
    const int lane = (int)threadIdx.x;
    const size_t pixel = blockIdx.x;
    if (done[pixel] != kRunningWord) return;   // uniform over the block
    uint32_t* const st = state + pixel * kWStWords;
    uint32_t* const words = reinterpret_cast<uint32_t*>(&m);
    for (int i = lane; i < (int)(sizeof(WaveMem) / sizeof(uint32_t)); i += kWaveLanes) words[i] = 0u;
    __syncthreads();
    if (lane == 0) { m.n = n; m.H = 2 * n; }
    if (lane < 5) m.neg[lane] = st[kStNeg + lane];
    if (lane < kWaveHalf) {
        m.zx[kPad + lane] = st[kStHeader + lane];
        m.zy[kPad + lane] = st[kStHeader + kWaveHalf + lane];
        m.sx[lane] = st[kStHeader + 2 * kWaveHalf + lane];
        m.sy[lane] = st[kStHeader + 3 * kWaveHalf + lane];
        m.pr[lane] = st[kStHeader + 4 * kWaveHalf + lane];
        m.cx[lane] = st[kStHeader + 5 * kWaveHalf + lane];
        m.cy[lane] = st[kStHeader + 6 * kWaveHalf + lane];
    }
    uint32_t j = st[kStJ], count = kRunningWord;
    __syncthreads();
    for (uint32_t it = 0; it < iters && j < max_iter; it++) {
        wave_phase(m, 0, lane); __syncthreads();
        wave_phase(m, 1, lane); __syncthreads();
        wave_phase(m, 2, lane); __syncthreads();
        wave_phase(m, 3, lane); __syncthreads();
        wave_phase(m, 4, lane); __syncthreads();
        wave_phase(m, 5, lane); __syncthreads();
        wave_phase(m, 6, lane); __syncthreads();
        wave_phase(m, 7, lane); __syncthreads();
        if (wave_escaped(m)) { count = j; break; }   // uniform: written before the last barrier
        j++;
    }
    if (count == kRunningWord && j >= max_iter) count = max_iter;
    if (count != kRunningWord) {
        if (lane == 0) done[pixel] = count;
        return;
    }
    if (lane == 0) st[kStJ] = j;
    if (lane < 3) st[kStNeg + lane] = m.neg[lane];
    if (lane < kWaveHalf) {
        st[kStHeader + lane] = m.zx[kPad + lane];
        st[kStHeader + kWaveHalf + lane] = m.zy[kPad + lane];
        st[kStHeader + 2 * kWaveHalf + lane] = m.sx[lane];
        st[kStHeader + 3 * kWaveHalf + lane] = m.sy[lane];
        st[kStHeader + 4 * kWaveHalf + lane] = m.pr[lane];
    }
}

__global__ void __launch_bounds__(kLanes) mandel_exact_group_kernel(uint32_t* __restrict__ state_all, uint32_t* __restrict__ done, int k,
                                                                    uint32_t iters, uint32_t max_iter) {
    __shared__ Mem m;
    const int lane = (int)threadIdx.x;
    const size_t pixel = blockIdx.x;
    if (done[pixel] != kRunningWord) return;   // uniform over the block
    uint32_t* const state = state_all + pixel * kStWords;
    uint32_t* const nums[7] = {m.zx, m.zy, m.sx, m.sy, m.pr, m.cx, m.cy};
    const int H = 2 * (k + 1);
    if (lane == 0) {
        m.k = k;
        m.H = H;
        m.status = kRunning;
        m.j = state[kStJ];
    }
    if (lane < 5) m.neg[lane] = state[kStNeg + lane];
    for (int q = 0; q < 7; q++)   // all kHalfPad words: the state is zero from H on, which prod_columns relies on
        for (int h = lane; h < kHalfPad; h += kLanes) nums[q][h] = state[kStHeader + q * kHalfPad + h];
    __syncthreads();
    uint32_t count = kRunningWord;
    for (uint32_t it = 0; it < iters; it++) {
        group_phase(m, 0, lane);
        __syncthreads();
        group_phase(m, 1, lane);
        __syncthreads();
        if (m.j == max_iter) {                         // uniform: only the escape test of z_(max_iter) is left
            count = escaped(m) ? max_iter - 1u : max_iter;
            break;
        }
        group_phase(m, 2, lane);
        __syncthreads();
        if (m.status != kRunning) { count = m.j - 1u; break; }
        group_phase(m, 3, lane);
        __syncthreads();
        group_phase(m, 4, lane);
        __syncthreads();
        group_phase(m, 5, lane);
        __syncthreads();
    }
    if (count != kRunningWord) {
        if (lane == 0) done[pixel] = count;
        return;
    }
    if (lane == 0) state[kStJ] = m.j;
    if (lane < 3) state[kStNeg + lane] = m.neg[lane];
    for (int q = 0; q < 5; q++)
        for (int h = lane; h < H; h += kLanes) state[kStHeader + q * kHalfPad + h] = nums[q][h];
}

struct ExactDevice {
    DeviceBuffer state, done;
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool valid = false;
    double device_ms = 0.0;
    uint32_t launches = 0, limbs = 0, iters_per_launch = 0, kernel = 0;
};
SideRecords<ExactDevice> g_exact_devices;

uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

}  // namespace

uint32_t exact_launch_iters(int n, uint64_t n_pixels, uint32_t cus) {
    if (cus == 0) cus = 1;
    uint64_t it;
    if (n > kWaveMaxLimbs) {
        it = kOrbitLaunchWork / ((uint64_t)n * (uint64_t)n) / ceil_div(n_pixels, cus);   // orbit_launch_iters' rule before its clamp
    } else {
        const uint64_t rounds = ceil_div(n_pixels, (uint64_t)cus * kExactWavesPerCu);
        it = kExactWaveLaunchNs / ((kExactWaveIterNs0 + kExactWaveIterNs1 * (uint64_t)n) * rounds);
    }
    return (uint32_t)(it < 1u ? 1u : it > 65536u ? 65536u : it);
}

void exact_device_release(mc_context* ctx) {
    g_exact_devices.erase(ctx, [](ExactDevice& d) {
        d.state.release();
        d.done.release();
        for (auto& e : d.ev)
            if (e) (void)hipEventDestroy(e);
    });
}

namespace {

int exact_device_run(mc_context* ctx, const ExactPixels& px, uint32_t max_iter, uint64_t n_pixels, uint32_t* out_n) {
    MC_HIP_TRY(hipSetDevice(ctx->device));
    ExactDevice* d = g_exact_devices.get(ctx);   // (the timing record is written on success only: a failed call leaves the last one)
    for (auto& e : d->ev)
        if (!e) MC_HIP_TRY(hipEventCreate(&e));
    const int n = px.n;
    const bool wave = n <= kWaveMaxLimbs;
    const size_t words = wave ? kWStWords : kStWords, half = wave ? kWaveHalf : kHalfPad;
    std::vector<uint32_t> st, done;
    try {
        st.assign(n_pixels * words, 0u);
        done.assign(n_pixels, kRunningWord);
    } catch (const std::bad_alloc&) {
        set_error_detail("mc_mandelbrot_exact_counts_device: the pixels' state does not fit in host memory");
        return MC_ERR_OUT_OF_MEMORY;
    }
    for (uint64_t p = 0; p < n_pixels; p++) {
        uint32_t* s = &st[p * words];
        s[kStNeg + kNegCx] = px.cx_neg[p];
        s[kStNeg + kNegCy] = px.cy_neg[p];
        for (int i = 0; i < n; i++) {
            const uint64_t x = px.cx[p * n + i], y = px.cy[p * n + i];
            s[kStHeader + 5 * half + 2 * i] = (uint32_t)x;
            s[kStHeader + 5 * half + 2 * i + 1] = (uint32_t)(x >> 32);
            s[kStHeader + 6 * half + 2 * i] = (uint32_t)y;
            s[kStHeader + 6 * half + 2 * i + 1] = (uint32_t)(y >> 32);
        }
    }
    int rc;
    if ((rc = d->state.reserve(st.size() * sizeof(uint32_t)))) return rc;
    if ((rc = d->done.reserve(done.size() * sizeof(uint32_t)))) return rc;
    const uint32_t chunk = exact_launch_iters(n, n_pixels, (uint32_t)ctx->props.multiProcessorCount);
    hipStream_t s = ctx->stream;
    MC_HIP_TRY(hipMemcpyAsync(d->state.ptr, st.data(), st.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    MC_HIP_TRY(hipMemcpyAsync(d->done.ptr, done.data(), done.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    MC_HIP_TRY(hipEventRecord(d->ev[0], s));
    // every launch advances every running pixel by `chunk` iterations; the workgroup kernel's last one only tests z_(max_iter)
    const uint64_t most = (uint64_t)max_iter / chunk + 2u;
    uint32_t launches = 0;
    for (bool running = true; running;) {
        if (launches >= most) {
            set_error_detail("mc_mandelbrot_exact_counts_device: pixels still running after every slice");
            return MC_ERR_HIP;
        }
        if (wave)
            hipLaunchKernelGGL(mandel_exact_wave_kernel, dim3((uint32_t)n_pixels), dim3(kWaveLanes), 0, s, (uint32_t*)d->state.ptr,
                               (uint32_t*)d->done.ptr, n, chunk, max_iter);
        else
            hipLaunchKernelGGL(mandel_exact_group_kernel, dim3((uint32_t)n_pixels), dim3(kLanes), 0, s, (uint32_t*)d->state.ptr,
                               (uint32_t*)d->done.ptr, n - 1, chunk, max_iter);
        MC_HIP_TRY(hipGetLastError());
        MC_HIP_TRY(hipEventRecord(d->ev[1], s));
        launches++;
        MC_HIP_TRY(hipMemcpyAsync(done.data(), d->done.ptr, done.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        MC_HIP_TRY(hipStreamSynchronize(s));
        running = false;
        for (uint64_t p = 0; p < n_pixels; p++) {
            if (done[p] == kRunningWord) running = true;
            else if (done[p] > max_iter) {
                set_error_detail("mc_mandelbrot_exact_counts_device: a count read back is not one the kernel writes");
                return MC_ERR_HIP;
            }
        }
    }
    std::memcpy(out_n, done.data(), done.size() * sizeof(uint32_t));
    float ms = 0.0f;
    MC_HIP_TRY(hipEventElapsedTime(&ms, d->ev[0], d->ev[1]));
    d->device_ms = ms;
    d->launches = launches;
    d->limbs = (uint32_t)n;
    d->iters_per_launch = chunk;
    d->kernel = wave ? MC_EXACT_KERNEL_WAVE : MC_EXACT_KERNEL_WORKGROUP;
    d->valid = true;
    return MC_OK;
}

}  // namespace
}  // namespace mc

extern "C" int mc_mandelbrot_exact_counts_device(mc_context* ctx, const mc_mandelbrot_orbit* o, uint32_t max_iter, uint32_t extra_limbs,
                                                 uint64_t n_pixels, const double* dcx, const double* dcy, int32_t dc_exp2,
                                                 uint32_t* out_n) {
    const char* fn = "mc_mandelbrot_exact_counts_device";
    if (!ctx) {
        mc::set_error_detail(std::string(fn) + ": NULL argument");
        return MC_ERR_INVALID_ARGUMENT;
    }
    mc::ExactPixels px;
    if (int rc = mc::exact_prepare(fn, o, max_iter, extra_limbs, n_pixels, dcx, dcy, dc_exp2, out_n, &px)) return rc;
    return mc::exact_device_run(ctx, px, max_iter, n_pixels, out_n);
}

extern "C" int mc_context_last_exact_timing(mc_context* ctx, double* device_ms, uint32_t* launches, uint32_t* limbs,
                                            uint32_t* iters_per_launch, uint32_t* kernel) {
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    const mc::ExactDevice* d = mc::g_exact_devices.find(ctx);
    if (!d || !d->valid) return MC_ERR_INVALID_ARGUMENT;
    if (device_ms) *device_ms = d->device_ms;
    if (launches) *launches = d->launches;
    if (limbs) *limbs = d->limbs;
    if (iters_per_launch) *iters_per_launch = d->iters_per_launch;
    if (kernel) *kernel = d->kernel;
    return MC_OK;
}
