// The area filter's host path (csrc/mandel_zoom.h, csrc/mandel_zoom_counts.h) alone, for a sanitizer: this file and those headers, no HIP
// and no library.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/zoom_filter_host_check.cpp -o zoom_filter_host_check && ./zoom_filter_host_check
// Every buffer is a std::vector of exactly the size the contract names, so a tap or a store one texel outside it is a heap overflow the
// sanitizer reports.  The cases are the shapes at which the box's clamps can act (one texel on an axis, two, odd, more than a block) at
// the ends of r, next to them and in between, with the deep keyframe present and absent, for vec4 keyframes and for count keyframes in
// all four colourings; the contract's identities are checked on the way.  A failed check prints its line and exits 1; the last line of a
// clean run is "zoom_filter_host_check: <n> cases OK".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../vulkan-compute-tests_amd/csrc/mandel_zoom_counts.h"

static int g_cases = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::printf("zoom_filter_host_check: line %d: %s\n", __LINE__, #cond);  \
            std::exit(1);                                                           \
        }                                                                           \
    } while (0)

static uint32_t g_seed = 1u;
static uint32_t next() {
    g_seed = g_seed * 1664525u + 1013904223u;
    return g_seed >> 8;
}

static std::vector<float> keyframe(uint32_t W, uint32_t H) {
    std::vector<float> a((size_t)W * H * 4);
    for (size_t i = 0; i < a.size(); i++) {
        const uint32_t k = next();
        a[i] = (i & 3u) == 3u ? 1.0f : (k % 11u == 0u ? 0.0f : k % 13u == 0u ? 1.0f : k % 17u == 0u ? -0.0f : (float)k * (1.0f / 16777216.0f));
    }
    return a;
}

static void vec4_case(uint32_t W, uint32_t H, double r, bool with_deep) {
    const std::vector<float> wide = keyframe(W, H), deep = keyframe(W, H);
    const size_t npix = (size_t)W * H;
    const float* d = with_deep ? deep.data() : nullptr;
    std::vector<float> f(npix * 4, -1.0f), f2(npix * 4, -1.0f), plain(npix * 4, -1.0f);
    std::vector<uint8_t> b(npix * 4, 7u), b2(npix * 4, 7u);
    mc::zoom::compose_area_host(W, H, wide.data(), d, r, f.data(), nullptr);
    mc::zoom::compose_area_host(W, H, wide.data(), d, r, nullptr, b.data());
    mc::zoom::compose_area_host(W, H, wide.data(), d, r, f2.data(), b2.data());
    mc::zoom::compose_host(W, H, wide.data(), d, r, plain.data(), nullptr);
    CHECK(std::memcmp(f.data(), f2.data(), npix * 16) == 0);
    CHECK(std::memcmp(b.data(), b2.data(), npix * 4) == 0);
    for (uint32_t gy = 0; gy < H; gy++) {
        const mc::zoom::AxisArea ay = mc::zoom::axis_area(gy, H, r, with_deep);
        for (int j = 0; j < 3; j++) CHECK(ay.box.i[j] < H && ay.box.w[j] >= 0.0f && ay.box.w[j] <= 1.0f);
        CHECK(ay.box.w[0] + ay.box.w[1] + ay.box.w[2] > 0.0f);
        for (uint32_t gx = 0; gx < W; gx++) {
            const mc::zoom::AxisArea ax = mc::zoom::axis_area(gx, W, r, with_deep);
            for (int j = 0; j < 3; j++) CHECK(ax.box.i[j] < W && ax.box.w[j] >= 0.0f && ax.box.w[j] <= 1.0f);
            const size_t i = (size_t)gy * W + gx;
            for (int c = 0; c < 3; c++) {
                const float v = f[4 * i + c];
                CHECK(v >= 0.0f && v <= 1.0f);
                CHECK(b[4 * i + c] == (uint8_t)(int32_t)(255.0f * v));
            }
            CHECK(f[4 * i + 3] == 1.0f && b[4 * i + 3] == 255u);
            if (!(ax.bil.in_deep && ay.bil.in_deep)) CHECK(std::memcmp(&f[4 * i], &plain[4 * i], 16) == 0);
        }
    }
    if (r == 1.0 && !with_deep) CHECK(std::memcmp(f.data(), wide.data(), npix * 16) == 0);
    if (r == 0.5 && with_deep) CHECK(std::memcmp(f.data(), deep.data(), npix * 16) == 0);
    g_cases++;
}

static void counts_case(uint32_t W, uint32_t H, uint32_t M, int mode, double r, bool with_deep) {
    const size_t npix = (size_t)W * H;
    const bool smooth = mode >= mc::zoom_counts::Smooth;
    const uint32_t top = smooth ? 256u * M : M;
    std::vector<uint32_t> wide(npix), deep(npix);
    for (auto* p : {&wide, &deep})
        for (auto& v : *p) {
            const uint32_t k = next();
            v = k % 7u == 0u ? top : (smooth ? k % (top + 1u) : (k % 19u == 0u ? 0xffffffffu : k % (top + 3u)));
        }
    std::vector<float> lut(((size_t)M + 1) * 4);
    for (size_t i = 0; i < lut.size(); i++) lut[i] = (i & 3u) == 3u ? 1.0f : (float)next() * (1.0f / 16777216.0f);
    std::vector<uint32_t> map((size_t)M + 1);
    for (uint32_t j = 0; j <= M; j++) map[j] = smooth ? 256u * j : M - j;
    const uint32_t* d = with_deep ? deep.data() : nullptr;
    std::vector<float> f(npix * 4, -1.0f), ref(npix * 4, -1.0f);
    std::vector<uint8_t> b(npix * 4, 7u);
    mc::zoom_counts::compose_counts_area_host(W, H, M, mode, wide.data(), d, lut.data(), map.data(), r, f.data(), b.data());
    // the colours of the two planes through the unfiltered host form at r = 1 without a deep keyframe, then the vec4 filter of those
    std::vector<float> cw(npix * 4), cd(npix * 4);
    mc::zoom_counts::compose_counts_host(W, H, M, mode, wide.data(), nullptr, lut.data(), map.data(), 1.0, cw.data(), nullptr);
    mc::zoom_counts::compose_counts_host(W, H, M, mode, deep.data(), nullptr, lut.data(), map.data(), 1.0, cd.data(), nullptr);
    mc::zoom::compose_area_host(W, H, cw.data(), with_deep ? cd.data() : nullptr, r, ref.data(), nullptr);
    CHECK(std::memcmp(f.data(), ref.data(), npix * 16) == 0);
    for (size_t i = 0; i < npix; i++) CHECK(b[4 * i + 3] == 255u);
    g_cases++;
}

int main() {
    const uint32_t shapes[][2] = {{1, 1}, {1, 7}, {7, 1}, {2, 2}, {3, 5}, {8, 8}, {67, 35}, {257, 130}};
    const double rs[] = {1.0, 0.5, std::exp2(-1.0 / 3.0), std::exp2(-2.0 / 3.0), 0.75, std::nextafter(0.5, 1.0), std::nextafter(1.0, 0.0)};
    for (const auto& s : shapes)
        for (double r : rs)
            for (int with_deep = 0; with_deep < 2; with_deep++) {
                vec4_case(s[0], s[1], r, with_deep != 0);
                if (s[0] <= 67u)
                    for (int mode = 0; mode < 4; mode++)
                        for (uint32_t M : {1u, 37u}) counts_case(s[0], s[1], M, mode, r, with_deep != 0);
            }
    std::printf("zoom_filter_host_check: %d cases OK\n", g_cases);
    return 0;
}
