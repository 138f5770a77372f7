// The noise plane's and the noise-guided filter's host path (csrc/pt_noise.h over csrc/pt_denoise.h) alone, for a sanitizer: this file and
// those headers, no HIP and no library.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/pt_noise_host_check.cpp -o pt_noise_host_check && ./pt_noise_host_check
// Every buffer is a std::vector of exactly the size the contract names, so a tap or a store one pixel outside it is a heap overflow the
// sanitizer reports.  The window's and the taps' indexing is where an out-of-bounds read would hide: the shapes are the border-heavy ones
// of tools/pt_denoise_host_check.cpp with every radius 0 .. 4 (windows wider than the image, clipped on every side) and pass counts 1, 5
// and 8.  The contract's identities are checked on the way (V finite and not negative, radius 0 returns v, a window that covers the whole
// image returns one value everywhere, V of a half that encodes to the full buffer is 0; the filter leaves alpha and miss pixels alone, an
// all-miss plane as it is, a constant plane constant, and with V = 0 runs at kc = 4^i whatever k_noise).  A failed check prints its line and
// exits 1; the last line of a clean run is "pt_noise_host_check: <n> cases OK".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../vulkan-compute-tests_amd/csrc/pt_noise.h"

using mc::ptd::vec4;

static int g_cases = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("pt_noise_host_check: line %d: %s\n", __LINE__, #cond); \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

static uint32_t g_seed = 54321u;
static float rnd() {
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)(g_seed >> 8) * (1.0f / 16777216.0f);
}

static void noise_case(uint32_t W, uint32_t H, uint32_t radius, float scale) {
    const size_t npix = (size_t)W * H;
    std::vector<vec4> half(npix), full(npix);
    for (size_t i = 0; i < npix; i++) {   // half * scale from -0.2 to 1.8: both sides of the clamp; a few exact zeros
        half[i] = vec4{rnd() - 0.1f, rnd() - 0.1f, rnd() < 0.1f ? 0.0f : rnd() - 0.1f, rnd()};
        full[i] = vec4{255.5f * rnd(), 255.5f * rnd(), 255.5f * rnd(), rnd()};
    }
    std::vector<float> V(npix, -1.0f), v0(npix, -1.0f);
    mc::ptd::noise_host(W, H, half.data(), scale, full.data(), radius, V.data());
    mc::ptd::noise_host(W, H, half.data(), scale, full.data(), 0, v0.data());
    for (size_t i = 0; i < npix; i++) {
        CHECK(std::isfinite(V[i]) && V[i] >= 0.0f && V[i] <= 3.0f * 256.0f * 256.0f);
        CHECK(v0[i] == mc::ptd::noise_pixel(half[i], scale, full[i]));
        if (radius + 1u >= W && radius + 1u >= H) CHECK(V[i] == V[0]);   // the window covers the image from every pixel
    }
    // a full buffer that IS the half's encoding: no noise
    for (size_t i = 0; i < npix; i++)
        full[i] = vec4{mc::ptd::encode_strict(half[i].x * scale), mc::ptd::encode_strict(half[i].y * scale), mc::ptd::encode_strict(half[i].z * scale), 0.0f};
    mc::ptd::noise_host(W, H, half.data(), scale, full.data(), radius, V.data());
    for (size_t i = 0; i < npix; i++) CHECK(V[i] == 0.0f);
    g_cases++;
}

static void filter_case(uint32_t W, uint32_t H, uint32_t passes, int mode) {   // mode 0: random ids, 1: all miss, 2: one id and a constant colour
    const size_t npix = (size_t)W * H;
    std::vector<vec4> rgba(npix), nt(npix), pid(npix), out(npix, vec4{-1, -1, -1, -1});
    std::vector<float> var(npix), zero(npix, 0.0f);
    for (size_t i = 0; i < npix; i++) {
        rgba[i] = mode == 2 ? vec4{100.0f, 50.0f, 25.0f, rnd()} : vec4{255.5f * rnd(), 255.5f * rnd(), 255.5f * rnd(), rnd()};
        nt[i] = vec4{rnd(), rnd(), rnd(), 9.0f * rnd()};
        const float id = mode == 1 ? -1.0f : mode == 2 ? 3.0f : std::floor(4.0f * rnd()) - 1.0f;
        pid[i] = vec4{0.6f * rnd(), 0.6f * rnd(), 0.6f * rnd(), id};
        const float r = rnd();
        var[i] = r < 0.1f ? 0.0f : r > 0.9f ? 1e30f : 2000.0f * r * r;
    }
    mc::ptd::denoise_adaptive_host(W, H, passes, 4.0f, 8.0f, 4.0f, rgba.data(), nt.data(), pid.data(), var.data(), out.data());
    for (size_t i = 0; i < npix; i++) {
        CHECK(out[i].w == rgba[i].w);
        if (pid[i].w < 0.0f) CHECK(std::memcmp(&out[i], &rgba[i], sizeof(vec4)) == 0);
        CHECK(out[i].x >= -1e-3f && out[i].x <= 255.6f && out[i].y >= -1e-3f && out[i].y <= 255.6f && out[i].z >= -1e-3f && out[i].z <= 255.6f);
        if (mode == 2) CHECK(std::fabs(out[i].x - 100.0f) < 1e-3f && std::fabs(out[i].y - 50.0f) < 1e-3f && std::fabs(out[i].z - 25.0f) < 1e-3f);
    }
    // in place: the same bits
    std::vector<vec4> inplace = rgba;
    mc::ptd::denoise_adaptive_host(W, H, passes, 4.0f, 8.0f, 4.0f, inplace.data(), nt.data(), pid.data(), var.data(), inplace.data());
    CHECK(std::memcmp(inplace.data(), out.data(), npix * sizeof(vec4)) == 0);
    // V = 0: kc_i = 4^i, the fixed filter at sigma_colour = 1, whatever k_noise
    std::vector<vec4> fixed(npix);
    mc::ptd::denoise_host(W, H, passes, 1.0f, 8.0f, 4.0f, rgba.data(), nt.data(), pid.data(), fixed.data());
    mc::ptd::denoise_adaptive_host(W, H, passes, 7.0f, 8.0f, 4.0f, rgba.data(), nt.data(), pid.data(), zero.data(), out.data());
    CHECK(std::memcmp(fixed.data(), out.data(), npix * sizeof(vec4)) == 0);
    g_cases++;
}

int main() {
    const uint32_t shapes[][2] = {{1, 1}, {1, 7}, {7, 1}, {2, 2}, {3, 5}, {7, 5}, {9, 9}, {64, 4}, {65, 5}, {130, 67}, {131, 3}};
    const uint32_t pass_counts[] = {1, 5, 8};
    for (const auto& s : shapes) {
        for (uint32_t radius = 0; radius <= mc::ptd::kMaxNoiseRadius; radius++) {
            noise_case(s[0], s[1], radius, 2.0f);
            noise_case(s[0], s[1], radius, 2.5f);
        }
        for (uint32_t passes : pass_counts)
            for (int mode = 0; mode < 3; mode++) filter_case(s[0], s[1], passes, mode);
    }
    std::printf("pt_noise_host_check: %d cases OK\n", g_cases);
    return 0;
}
