// The resolve over fractional counts' host path (csrc/mandel_resolve_smooth.h and the two headers it composes) alone, for a sanitizer:
// this file and those headers, no HIP and no library.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/mandel_resolve_smooth_host_check.cpp -o mandel_resolve_smooth_host_check && ./mandel_resolve_smooth_host_check
// Every buffer is a std::vector of exactly the size the contract names (the (rows * s) x (s * width) plane, max_iter pairs,
// max_iter + 1 colours, rows * width vec4), so a read or a store one entry outside it is a heap overflow the sanitizer reports.  The
// planes hold the values that form the largest indices: 256 M - 1, 256 M, counts above it and 0xffffffff (clamped before any index is
// formed).  The cases: the border-heavy shapes 1 x 1, 3 x 2, 5 x 3, 33 x 7, 130 x 5 for s = 2, 4, 8 at M = 1, 7 and 300, with and
// without a knot map (random knots, coinciding knots, the identity), and one knot map at M = 2^24 - 1.  Each case compares every pixel,
// bit for bit, with the composition written out: smooth::smooth_colour of smooth_equalise::remap of the clamped count, summed by an
// explicit pairwise loop.  A failed check prints its line and exits 1; the last line of a clean run is
// "mandel_resolve_smooth_host_check: <n> cases OK".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../vulkan-compute-tests_amd/csrc/mandel_resolve_smooth.h"

namespace rs = mc::resolve_smooth;
namespace sq = mc::smooth_equalise;

static int g_cases = 0;
#define CHECK(cond)                                                                         \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            std::printf("mandel_resolve_smooth_host_check: line %d: %s\n", __LINE__, #cond); \
            std::exit(1);                                                                   \
        }                                                                                   \
    } while (0)

static uint32_t g_seed = 2463534242u;
static uint32_t rnd() {
    g_seed ^= g_seed << 13; g_seed ^= g_seed >> 17; g_seed ^= g_seed << 5;
    return g_seed;
}

static std::vector<float> make_lut(uint32_t M) {
    std::vector<float> lut(((size_t)M + 1) * 4);
    for (size_t n = 0; n <= M; n++) {
        for (int c = 0; c < 3; c++) lut[4 * n + c] = (float)(rnd() & 0xffffffu) * (1.0f / 16777216.0f);
        lut[4 * n + 3] = 1.0f;
    }
    return lut;
}

// kind 0: identity; 1: random non-decreasing knots; 2: long runs of coinciding knots
static std::vector<uint32_t> make_qmap(uint32_t M, int kind) {
    const uint32_t top = 256u * M;
    std::vector<uint32_t> m((size_t)M + 1);
    for (size_t j = 0; j <= M; j++) m[j] = kind == 0 ? 256u * (uint32_t)j : kind == 1 ? rnd() % (top + 1u) : (rnd() % 5u) * (top / 4u);
    std::sort(m.begin(), m.end());
    m[M] = top;
    return m;
}

static std::vector<uint32_t> make_plane(uint32_t M, size_t count) {
    const uint32_t top = 256u * M;
    std::vector<uint32_t> q(count);
    const uint32_t edge[] = {0u, 255u, 256u, top - 1u, top, top + 1u, 0xffffffffu, top > 256u ? top - 256u : 0u};
    for (size_t i = 0; i < count; i++) {
        const uint32_t k = rnd() % 16u;
        q[i] = k < 8u ? edge[k] : k < 10u ? (rnd() % (top + 1u)) & ~255u : k < 12u ? std::min((rnd() % (top + 1u)) | 255u, top) : rnd() % (top + 1u);
    }
    return q;
}

static void pairwise(std::vector<rs::Rgba> v, rs::Rgba* out) {
    while (v.size() > 1) {
        std::vector<rs::Rgba> n(v.size() / 2);
        for (size_t k = 0; k < n.size(); k++)
            n[k] = rs::Rgba{v[2 * k].r + v[2 * k + 1].r, v[2 * k].g + v[2 * k + 1].g, v[2 * k].b + v[2 * k + 1].b, v[2 * k].a + v[2 * k + 1].a};
        v.swap(n);
    }
    *out = v[0];
}

static void run_case(uint32_t M, uint32_t s, uint32_t W, uint32_t rows, const std::vector<float>& lut, const std::vector<uint32_t>* qmap) {
    CHECK(lut.size() == ((size_t)M + 1) * 4);
    const uint32_t top = 256u * M;
    const std::vector<uint32_t> q = make_plane(M, (size_t)rows * s * W * s);
    std::vector<uint32_t> pairs;
    if (qmap) {
        CHECK(qmap->size() == (size_t)M + 1);
        pairs.assign((size_t)M * 2, 0xdeadbeefu);
        sq::compose_pairs(M, qmap->data(), pairs.data());
    }
    std::vector<float> out((size_t)rows * W * 4, -1.0f);
    CHECK(rs::resolve_plane(s, M, W, rows, q.data(), qmap ? pairs.data() : nullptr, lut.data(), out.data()));
    const size_t pitch = (size_t)s * W;
    const float inv = 1.0f / (float)(s * s);
    for (uint32_t y = 0; y < rows; y++)
        for (uint32_t x = 0; x < W; x++) {
            std::vector<rs::Rgba> rsum(s);
            bool flat = true;
            for (uint32_t i = 0; i < s; i++) {
                std::vector<rs::Rgba> a(s);
                for (uint32_t j = 0; j < s; j++) {
                    uint32_t v = q[((size_t)y * s + i) * pitch + (size_t)x * s + j];
                    flat = flat && v == q[(size_t)y * s * pitch + (size_t)x * s];
                    v = v < top ? v : top;
                    if (qmap) v = sq::remap(v, M, pairs.data());
                    float c[4];
                    mc::smooth::smooth_colour(v, M, lut.data(), c);
                    a[j] = rs::Rgba{c[0], c[1], c[2], c[3]};
                }
                pairwise(a, &rsum[i]);
            }
            rs::Rgba t;
            pairwise(rsum, &t);
            const float want[4] = {t.r * inv, t.g * inv, t.b * inv, t.a * inv};
            const float* got = &out[4 * ((size_t)y * W + x)];
            CHECK(std::memcmp(got, want, sizeof want) == 0);
            CHECK(got[3] == 1.0f);
            if (flat) {   // consequence 1: exactly the smooth colour of the shared count
                uint32_t v = q[(size_t)y * s * pitch + (size_t)x * s];
                v = v < top ? v : top;
                if (qmap) v = sq::remap(v, M, pairs.data());
                float c[4];
                mc::smooth::smooth_colour(v, M, lut.data(), c);
                CHECK(std::memcmp(got, c, sizeof c) == 0);
            }
        }
    g_cases++;
}

int main() {
    const uint32_t shapes[][2] = {{1, 1}, {3, 2}, {5, 3}, {33, 7}, {130, 5}};   // width x rows
    for (uint32_t M : {1u, 7u, 300u}) {
        const std::vector<float> lut = make_lut(M);
        std::vector<std::vector<uint32_t>> maps;
        for (int kind = 0; kind < 3; kind++) maps.push_back(make_qmap(M, kind));
        for (uint32_t s : {2u, 4u, 8u})
            for (const auto& sh : shapes) {
                run_case(M, s, sh[0], sh[1], lut, nullptr);
                for (const auto& m : maps) run_case(M, s, sh[0], sh[1], lut, &m);
            }
    }
    {   // a knot map at the largest max_iter: the pair and colour tables at their largest
        const uint32_t M = 0x00ffffffu;
        const std::vector<float> lut = make_lut(M);
        const std::vector<uint32_t> qmap = make_qmap(M, 1);
        run_case(M, 2, 3, 2, lut, &qmap);
        run_case(M, 8, 1, 1, lut, &qmap);
        run_case(M, 4, 5, 3, lut, nullptr);
    }
    CHECK(!rs::resolve_plane(3u, 1u, 1u, 1u, nullptr, nullptr, nullptr, nullptr));
    std::printf("mandel_resolve_smooth_host_check: %d cases OK\n", g_cases);
    return 0;
}
