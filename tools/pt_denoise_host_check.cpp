// The path-tracer denoiser's host path (csrc/pt_denoise.h) alone, for a sanitizer: this file and that header, no HIP and no library.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/pt_denoise_host_check.cpp -o pt_denoise_host_check && ./pt_denoise_host_check
// Every buffer is a std::vector of exactly the size the contract names, so a tap or a store one pixel outside it is a heap overflow the
// sanitizer reports.  The tap indexing is where an out-of-bounds read would hide: the shapes are the border-heavy ones (one pixel on an
// axis, fewer pixels than the widest tap offset, one more than a block, odd sizes) with every pass count 1 .. 8, so that steps up to 128
// meet images of 1 .. 131 pixels; the guides run on the same shapes for a closed scene, an open one and an empty one.  The contract's
// identities are checked on the way (alpha and miss pixels untouched, an all-miss plane returned as it is, a constant plane returned
// constant, the output inside the input's range).  A failed check prints its line and exits 1; the last line of a clean run is
// "pt_denoise_host_check: <n> cases OK".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../vulkan-compute-tests_amd/csrc/pt_denoise.h"

using mc::ptd::vec4;

static int g_cases = 0;
#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::printf("pt_denoise_host_check: line %d: %s\n", __LINE__, #cond); \
            std::exit(1);                                                         \
        }                                                                         \
    } while (0)

static uint32_t g_seed = 12345u;
static float rnd() {
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)(g_seed >> 8) * (1.0f / 16777216.0f);
}

static const float kPlanes[6 * 12] = {
    -1, 0, 0, 2.6f, 0, 0, 0, 0, .85f, .25f, .25f, 1, 1, 0, 0, 2.6f, 0, 0, 0, 0, .25f, .35f, .85f, 1, 0, 1,  0, 2.0f, 0, 0, 0, 0, .75f, .75f, .75f, 1,
    0,  -1, 0, 2.0f, 0, 0, 0, 0, .75f, .75f, .75f, 1, 0, 0, -1, 2.8f, 0, 0, 0, 0, .85f, .85f, .25f, 1, 0, 0, 1, 7.9f, 0, 0, 0, 0, .1f,  .7f,  .7f,  1};
static const float kSpheres[3 * 12] = {-1.3f, -1.2f, -1.3f, 0.8f, 0, 0, 0, 0, .999f, .999f, .999f, 2, 1.3f, -1.2f, -0.2f, 0.8f, 0, 0, 0, 0, .999f, .999f, .999f, 3,
                                       0,     1.6f,  0,     0.2f, 100, 100, 100, 0, 0, 0, 0, 1};

static void guides_case(uint32_t W, uint32_t H, uint32_t n_planes, uint32_t n_spheres, bool expect_all_hit) {
    std::vector<float> rec;
    rec.insert(rec.end(), kPlanes, kPlanes + 12 * n_planes);
    rec.insert(rec.end(), kSpheres, kSpheres + 12 * n_spheres);
    const size_t npix = (size_t)W * H;
    std::vector<vec4> nt(npix, vec4{7, 7, 7, 7}), pid(npix, vec4{7, 7, 7, 7});
    mc::ptd::guides_host(W, H, rec.data(), n_planes, n_spheres, nt.data(), pid.data());
    for (size_t i = 0; i < npix; i++) {
        const float id = pid[i].w;
        CHECK(id == -1.0f || (id >= 0.0f && id < (float)(n_planes + n_spheres) && id == std::floor(id)));
        if (id < 0.0f) {
            CHECK(!expect_all_hit);
            CHECK(nt[i].x == 0.0f && nt[i].y == 0.0f && nt[i].z == 0.0f && nt[i].w == 1e20f && pid[i].x == 0.0f && pid[i].y == 0.0f && pid[i].z == 0.0f);
        } else {
            const float len2 = nt[i].x * nt[i].x + nt[i].y * nt[i].y + nt[i].z * nt[i].z;
            CHECK(std::fabs(len2 - 1.0f) < 1e-4f && nt[i].w > 0.0f && nt[i].w < 1e20f);
        }
    }
    g_cases++;
}

static void filter_case(uint32_t W, uint32_t H, uint32_t passes, int mode) {   // mode 0: random ids, 1: all miss, 2: one id and a constant colour
    const size_t npix = (size_t)W * H;
    std::vector<vec4> rgba(npix), nt(npix), pid(npix), out(npix, vec4{-1, -1, -1, -1});
    for (size_t i = 0; i < npix; i++) {
        rgba[i] = mode == 2 ? vec4{100.0f, 50.0f, 25.0f, rnd()} : vec4{255.5f * rnd(), 255.5f * rnd(), 255.5f * rnd(), rnd()};
        nt[i] = vec4{rnd(), rnd(), rnd(), 9.0f * rnd()};
        const float id = mode == 1 ? -1.0f : mode == 2 ? 3.0f : std::floor(4.0f * rnd()) - 1.0f;
        pid[i] = vec4{0.6f * rnd(), 0.6f * rnd(), 0.6f * rnd(), id};
    }
    mc::ptd::denoise_host(W, H, passes, 128.0f, 8.0f, 4.0f, rgba.data(), nt.data(), pid.data(), out.data());
    for (size_t i = 0; i < npix; i++) {
        CHECK(out[i].w == rgba[i].w);
        if (pid[i].w < 0.0f) CHECK(std::memcmp(&out[i], &rgba[i], sizeof(vec4)) == 0);
        // a weighted mean of inputs with positive weights, per pass: inside the plane's range up to rounding
        CHECK(out[i].x >= -1e-3f && out[i].x <= 255.6f && out[i].y >= -1e-3f && out[i].y <= 255.6f && out[i].z >= -1e-3f && out[i].z <= 255.6f);
        if (mode == 2) CHECK(std::fabs(out[i].x - 100.0f) < 1e-3f && std::fabs(out[i].y - 50.0f) < 1e-3f && std::fabs(out[i].z - 25.0f) < 1e-3f);
    }
    // in place: the same bits
    std::vector<vec4> inplace = rgba;
    mc::ptd::denoise_host(W, H, passes, 128.0f, 8.0f, 4.0f, inplace.data(), nt.data(), pid.data(), inplace.data());
    CHECK(std::memcmp(inplace.data(), out.data(), npix * sizeof(vec4)) == 0);
    g_cases++;
}

int main() {
    const uint32_t shapes[][2] = {{1, 1}, {1, 7}, {7, 1}, {2, 2}, {3, 5}, {7, 5}, {9, 9}, {64, 4}, {65, 5}, {130, 67}, {131, 3}};
    for (const auto& s : shapes) {
        guides_case(s[0], s[1], 6, 3, true);    // the reference scene: a closed box, every ray hits
        guides_case(s[0], s[1], 1, 1, false);   // one wall and the mirror sphere: misses
        guides_case(s[0], s[1], 0, 0, false);   // nothing: every pixel a miss
        for (uint32_t passes = 1; passes <= mc::ptd::kMaxPasses; passes++)
            for (int mode = 0; mode < 3; mode++) filter_case(s[0], s[1], passes, mode);
    }
    std::printf("pt_denoise_host_check: %d cases OK\n", g_cases);
    return 0;
}
