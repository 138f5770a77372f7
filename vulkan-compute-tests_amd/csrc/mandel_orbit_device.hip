// mc_mandelbrot_orbit_create_device: the reference orbit's iteration loop on the device (include/mc_compute.h).
//
//  * one workgroup of 1024 threads runs the phases of mandel_orbit_fix.h with a barrier after each; the numbers live in LDS as 32-bit
//    half-limbs; the table entries go to a slice in device memory, one (re, im) pair per iteration.
//  * the orbit is computed in launches of at most orbit_launch_iters(k) iterations.  Between launches the state (status, j, the signs,
//    zx, zy, sx, sy and the rounded zx zy) lives in device memory; the host reads (status, j), 8 bytes, and the slice after each launch.
//    Nothing spins and nothing synchronises across workgroups.
//  * parsing, validation and the object are orbit_create's (mandel_orbit.cpp): this file is the loop, handed to it as an OrbitLoop.
#include <cstring>
#include <new>

#include "mandel_orbit_fix.h"
#include "mandel_perturb.h"
#include "mandel_side_record.h"
#include "mc_internal.h"

namespace mc {

using namespace orbitfix;

namespace {

// The state in device memory, in 32-bit words: a header, then seven numbers of kHalfPad half-limbs.
constexpr int kStStatus = 0, kStJ = 1, kStNeg = 2 /* 5 words */, kStHeader = 8;
constexpr int kStWords = kStHeader + 7 * kHalfPad;

__global__ void __launch_bounds__(kLanes) mandel_orbit_kernel(uint32_t* __restrict__ state, double* __restrict__ out, int k,
                                                              uint32_t iters, uint32_t max_iter, int deep) {
    __shared__ Mem m;
    const int lane = (int)threadIdx.x;
    uint32_t* const nums[7] = {m.zx, m.zy, m.sx, m.sy, m.pr, m.cx, m.cy};
    const int H = 2 * (k + 1);
    if (lane == 0) {
        m.k = k;
        m.H = H;
        m.status = state[kStStatus];
        m.j = state[kStJ];
    }
    if (lane < 5) m.neg[lane] = state[kStNeg + lane];
    for (int q = 0; q < 7; q++)   // all kHalfPad words: the state is zero from H on, which prod_columns relies on
        for (int h = lane; h < kHalfPad; h += kLanes) nums[q][h] = state[kStHeader + q * kHalfPad + h];
    __syncthreads();
    const uint32_t j0 = m.j;
    for (uint32_t it = 0; it < iters; it++) {
        if (m.status != kRunning || m.j >= max_iter) break;   // uniform: written before the last barrier
        orbit_phase(m, 0, lane, deep != 0, out, j0);
        __syncthreads();
        orbit_phase(m, 1, lane, deep != 0, out, j0);
        __syncthreads();
        orbit_phase(m, 2, lane, deep != 0, out, j0);
        __syncthreads();
        if (m.status != kRunning) break;                      // escaped: Z_j was the last entry
        orbit_phase(m, 3, lane, deep != 0, out, j0);
        __syncthreads();
        orbit_phase(m, 4, lane, deep != 0, out, j0);
        __syncthreads();
        orbit_phase(m, 5, lane, deep != 0, out, j0);
        __syncthreads();
    }
    if (lane == 0) {
        state[kStStatus] = m.status;
        state[kStJ] = m.j;
    }
    if (lane < 3) state[kStNeg + lane] = m.neg[lane];
    for (int q = 0; q < 5; q++)
        for (int h = lane; h < H; h += kLanes) state[kStHeader + q * kHalfPad + h] = nums[q][h];
}

struct OrbitDevice {
    DeviceBuffer state, slice;
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool valid = false;
    double device_ms = 0.0;
    uint32_t launches = 0, limbs = 0;
};
SideRecords<OrbitDevice> g_orbit_devices;

void init_state(std::vector<uint32_t>& st, int k, const uint64_t* cx, const uint64_t* cy, bool cx_neg, bool cy_neg) {
    st.assign(kStWords, 0u);
    st[kStStatus] = kRunning;
    st[kStNeg + kNegCx] = cx_neg;
    st[kStNeg + kNegCy] = cy_neg;
    for (int i = 0; i <= k; i++) {
        st[kStHeader + 5 * kHalfPad + 2 * i] = (uint32_t)cx[i];
        st[kStHeader + 5 * kHalfPad + 2 * i + 1] = (uint32_t)(cx[i] >> 32);
        st[kStHeader + 6 * kHalfPad + 2 * i] = (uint32_t)cy[i];
        st[kStHeader + 6 * kHalfPad + 2 * i + 1] = (uint32_t)(cy[i] >> 32);
    }
}

// The loop on ctx's device, otherwise an OrbitLoop (mandel_orbit.h).
int orbit_device_run(mc_context* ctx, int k, const uint64_t* cx, const uint64_t* cy, bool cx_neg, bool cy_neg, uint32_t max_iter,
                     bool deep, std::vector<double>& z, uint32_t* length, uint32_t* tiny_j) {
    MC_HIP_TRY(hipSetDevice(ctx->device));
    OrbitDevice* d = g_orbit_devices.get(ctx);
    d->valid = false;
    for (auto& e : d->ev)
        if (!e) MC_HIP_TRY(hipEventCreate(&e));
    const uint32_t chunk = orbit_launch_iters(k);
    const uint32_t slice_entries = chunk < max_iter ? chunk : max_iter;
    int rc;
    if ((rc = d->state.reserve(kStWords * sizeof(uint32_t)))) return rc;
    if ((rc = d->slice.reserve((size_t)slice_entries * 2 * sizeof(double)))) return rc;
    std::vector<uint32_t> st;
    init_state(st, k, cx, cy, cx_neg, cy_neg);
    hipStream_t s = ctx->stream;
    MC_HIP_TRY(hipMemcpyAsync(d->state.ptr, st.data(), st.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    MC_HIP_TRY(hipEventRecord(d->ev[0], s));
    uint32_t head[2] = {kRunning, 0u}, launches = 0;
    while (head[0] == kRunning && head[1] < max_iter) {
        const uint32_t j0 = head[1];
        hipLaunchKernelGGL(mandel_orbit_kernel, dim3(1), dim3(kLanes), 0, s, (uint32_t*)d->state.ptr, (double*)d->slice.ptr, k, chunk,
                           max_iter, deep ? 1 : 0);
        MC_HIP_TRY(hipGetLastError());
        MC_HIP_TRY(hipEventRecord(d->ev[1], s));
        launches++;
        MC_HIP_TRY(hipMemcpyAsync(head, d->state.ptr, sizeof head, hipMemcpyDeviceToHost, s));
        MC_HIP_TRY(hipStreamSynchronize(s));
        if (head[0] > kTiny || head[1] < j0 || head[1] - j0 > chunk || head[1] > max_iter) {
            set_error_detail("mandel_orbit_kernel: the state read back is not one the kernel writes");
            return MC_ERR_HIP;
        }
        const size_t got = head[1] - j0;
        if (got) {
            const size_t at = z.size();
            z.resize(at + 2 * got);   // (std::bad_alloc: caught by orbit_create)
            MC_HIP_TRY(hipMemcpyAsync(&z[at], d->slice.ptr, 2 * got * sizeof(double), hipMemcpyDeviceToHost, s));
            MC_HIP_TRY(hipStreamSynchronize(s));
        } else if (head[0] == kRunning) {
            set_error_detail("mandel_orbit_kernel: a launch made no progress");
            return MC_ERR_HIP;
        }
    }
    if (head[0] == kTiny) {
        *tiny_j = head[1] + 1u;
        return kOrbitTinyEntry;
    }
    *length = head[0] == kEscaped ? head[1] : max_iter;
    float ms = 0.0f;
    MC_HIP_TRY(hipEventElapsedTime(&ms, d->ev[0], d->ev[1]));
    d->device_ms = ms;
    d->launches = launches;
    d->limbs = (uint32_t)k + 1u;
    d->valid = true;
    return MC_OK;
}

// The same loop with the host's lane loops in place of threads (the CPU check of the shared arithmetic; no device).
int orbit_lanes_run(int k, const uint64_t* cx, const uint64_t* cy, bool cx_neg, bool cy_neg, uint32_t max_iter, bool deep,
                    std::vector<double>& z, uint32_t* length, uint32_t* tiny_j) {
    Mem* m = new (std::nothrow) Mem();
    if (!m) return MC_ERR_OUT_OF_MEMORY;
    struct Free { Mem* m; ~Free() { delete m; } } free_m{m};
    std::vector<uint32_t> st;
    init_state(st, k, cx, cy, cx_neg, cy_neg);
    m->k = k;
    m->H = 2 * (k + 1);
    m->neg[kNegCx] = cx_neg;
    m->neg[kNegCy] = cy_neg;
    std::memcpy(m->cx, &st[kStHeader + 5 * kHalfPad], sizeof m->cx);
    std::memcpy(m->cy, &st[kStHeader + 6 * kHalfPad], sizeof m->cy);
    double entry[2];
    while (m->status == kRunning && m->j < max_iter) {
        const uint32_t j0 = m->j;
        for (int ph = 0; ph < kPhases && m->status == kRunning; ph++)
            for (int lane = 0; lane < kLanes; lane++) orbit_phase(*m, ph, lane, deep, entry, j0);
        if (m->j != j0) { z.push_back(entry[0]); z.push_back(entry[1]); }
    }
    if (m->status == kTiny) {
        *tiny_j = m->j + 1u;
        return kOrbitTinyEntry;
    }
    *length = m->status == kEscaped ? m->j : max_iter;
    return MC_OK;
}

}  // namespace

uint32_t orbit_launch_iters(int k) {
    const uint64_t n = (uint64_t)k + 1u, it = kOrbitLaunchWork / (n * n);
    return (uint32_t)(it < 1u ? 1u : it > 65536u ? 65536u : it);
}

int orbit_create_lanes(const char* centre_x, const char* centre_y, double scale_x, double scale_y, int32_t scale_exp2, uint32_t max_iter,
                       mc_mandelbrot_orbit** out) {
    return orbit_create("orbit_create_lanes", "orbit_create_lanes", orbit_lanes_run, centre_x, centre_y, scale_x, scale_y, scale_exp2,
                        max_iter, out);
}

void orbit_device_release(mc_context* ctx) {
    g_orbit_devices.erase(ctx, [](OrbitDevice& d) {
        d.state.release();
        d.slice.release();
        for (auto& e : d.ev)
            if (e) (void)hipEventDestroy(e);
    });
}

}  // namespace mc

// The object of mc_mandelbrot_orbit_create_deep with the iteration loop on ctx's device.  Every refusal of the arguments comes first.
extern "C" int mc_mandelbrot_orbit_create_device(mc_context* ctx, const char* centre_x, const char* centre_y, double scale_x,
                                                 double scale_y, int32_t scale_exp2, uint32_t max_iter, mc_mandelbrot_orbit** out) {
    if (!ctx) {
        mc::set_error_detail("mc_mandelbrot_orbit_create_device: NULL argument");
        return MC_ERR_INVALID_ARGUMENT;
    }
    const char* fn = "mc_mandelbrot_orbit_create_device";
    return mc::orbit_create(fn, fn, [ctx](auto&&... a) { return mc::orbit_device_run(ctx, a...); }, centre_x, centre_y, scale_x, scale_y,
                            scale_exp2, max_iter, out);
}

extern "C" int mc_context_last_orbit_timing(mc_context* ctx, double* device_ms, uint32_t* launches, uint32_t* limbs) {
    if (!ctx) return MC_ERR_INVALID_ARGUMENT;
    const mc::OrbitDevice* d = mc::g_orbit_devices.find(ctx);
    if (!d || !d->valid) return MC_ERR_INVALID_ARGUMENT;
    if (device_ms) *device_ms = d->device_ms;
    if (launches) *launches = d->launches;
    if (limbs) *limbs = d->limbs;
    return MC_OK;
}
