// The zoom compose's host path (csrc/mandel_zoom.h) alone, for a sanitizer: this file and that header, no HIP and no library.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/zoom_host_check.cpp -o zoom_host_check && ./zoom_host_check
// Every buffer is a std::vector of exactly the size the contract names, so a tap or a store one texel outside it is a heap overflow the
// sanitizer reports.  The cases are the shapes at which the tap clamps can act or fail to (one texel on an axis, two, odd, more than a
// block) at the ends of r, next to them and in between, with the deep keyframe present and absent, for the vec4 output, the byte output
// and both; the contract's identities are checked on the way.  A failed check prints its line and exits 1; the last line of a clean run is
// "zoom_host_check: <n> cases OK".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../vulkan-compute-tests_amd/csrc/mandel_zoom.h"

static int g_cases = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("zoom_host_check: line %d: %s\n", __LINE__, #cond);  \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

static std::vector<float> keyframe(uint32_t W, uint32_t H, uint32_t seed) {
    std::vector<float> a((size_t)W * H * 4);
    uint32_t s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < a.size(); i++) {
        s = s * 1664525u + 1013904223u;
        const uint32_t k = s >> 8;
        a[i] = (i & 3u) == 3u ? 1.0f : (k % 11u == 0u ? 0.0f : k % 13u == 0u ? 1.0f : k % 17u == 0u ? -0.0f : (float)k * (1.0f / 16777216.0f));
    }
    return a;
}

static void one_case(uint32_t W, uint32_t H, double r, bool with_deep) {
    const std::vector<float> wide = keyframe(W, H, 1u), deep = keyframe(W, H, 2u);
    const size_t npix = (size_t)W * H;
    const float* d = with_deep ? deep.data() : nullptr;
    std::vector<float> f(npix * 4, -1.0f), f2(npix * 4, -1.0f);
    std::vector<uint8_t> b(npix * 4, 7u), b2(npix * 4, 7u);
    mc::zoom::compose_host(W, H, wide.data(), d, r, f.data(), nullptr);
    mc::zoom::compose_host(W, H, wide.data(), d, r, nullptr, b.data());
    mc::zoom::compose_host(W, H, wide.data(), d, r, f2.data(), b2.data());
    CHECK(std::memcmp(f.data(), f2.data(), npix * 16) == 0);
    CHECK(std::memcmp(b.data(), b2.data(), npix * 4) == 0);
    for (size_t i = 0; i < npix; i++) {
        for (int c = 0; c < 3; c++) {
            const float v = f[4 * i + c];
            CHECK(v >= 0.0f && v <= 1.0f);
            CHECK(b[4 * i + c] == (uint8_t)(int32_t)(255.0f * v));
        }
        CHECK(f[4 * i + 3] == 1.0f && b[4 * i + 3] == 255u);
    }
    if (r == 1.0 && !with_deep) CHECK(std::memcmp(f.data(), wide.data(), npix * 16) == 0);
    if (r == 0.5 && with_deep) CHECK(std::memcmp(f.data(), deep.data(), npix * 16) == 0);
    // every tap index the frame used lies inside its axis (the sanitizer sees the loads; this sees the indices)
    for (uint32_t g = 0; g < W; g++) {
        const mc::zoom::Axis a = mc::zoom::axis(g, W, r, with_deep);
        CHECK(a.wide.i0 < W && a.wide.i1 < W && a.deep.i0 < W && a.deep.i1 < W);
        CHECK(a.wide.f >= 0.0f && a.wide.f <= 1.0f && a.deep.f >= 0.0f && a.deep.f <= 1.0f);
    }
    for (uint32_t g = 0; g < H; g++) {
        const mc::zoom::Axis a = mc::zoom::axis(g, H, r, with_deep);
        CHECK(a.wide.i0 < H && a.wide.i1 < H && a.deep.i0 < H && a.deep.i1 < H);
    }
    g_cases++;
}

int main() {
    const uint32_t shapes[][2] = {{1, 1}, {1, 7}, {7, 1}, {2, 2}, {3, 5}, {8, 8}, {67, 35}, {257, 130}};
    const double rs[] = {1.0, 0.5, std::exp2(-1.0 / 3.0), std::exp2(-2.0 / 3.0), 0.75, std::nextafter(0.5, 1.0), std::nextafter(1.0, 0.0)};
    for (const auto& s : shapes)
        for (double r : rs)
            for (int with_deep = 0; with_deep < 2; with_deep++) one_case(s[0], s[1], r, with_deep != 0);
    std::printf("zoom_host_check: %d cases OK\n", g_cases);
    return 0;
}
