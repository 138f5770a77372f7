// The smooth equalised colouring's host path (csrc/mandel_smooth_equalise.h) alone, for a sanitizer: this file and that header, no HIP
// and no library.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/mandel_smooth_equalise_host_check.cpp -o mandel_smooth_equalise_host_check && ./mandel_smooth_equalise_host_check
// Every table is a std::vector of exactly the size the contract names (max_iter + 1 bins and knots, max_iter pairs), so a read or a store
// one entry outside it is a heap overflow the sanitizer reports, and the unsigned-overflow-free products (256 M C(j) below 2^64, a step
// times a fraction below 2^40) are what the undefined-behaviour sanitizer's shift and conversion checks watch.  The cases are the
// degenerate ones: M = 1; no escaped pixel; one occupied bin; more escaped pixels than palette positions (knot differences round to 0);
// a total at 2^32 - 1 and one past it; M = 2^24 - 1 with a sparse histogram (the product passes 2^63).  Each case checks the map against
// a 128-bit restatement, the contract's consequences (non-decreasing knots, the last knot at 256 M, an occupied bin's knot below it, the
// integer part equal to the integer rank map, q' non-decreasing in q and below 256 M for an escaped q).  A failed check prints its line
// and exits 1; the last line of a clean run is "mandel_smooth_equalise_host_check: <n> cases OK".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../vulkan-compute-tests_amd/csrc/mandel_smooth_equalise.h"

namespace sq = mc::smooth_equalise;

static int g_cases = 0;
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            std::printf("mandel_smooth_equalise_host_check: line %d: %s\n", __LINE__, #cond); \
            std::exit(1);                                                                    \
        }                                                                                    \
    } while (0)

static uint32_t g_seed = 2463534242u;
static uint32_t rnd() {
    g_seed ^= g_seed << 13; g_seed ^= g_seed >> 17; g_seed ^= g_seed << 5;
    return g_seed;
}

// hist: max_iter + 1 bins.  probes: extra q values to remap beside the ones every case takes (each occupied bin's ends, the table's ends).
static void run_case(uint32_t M, const std::vector<uint32_t>& hist, bool expect_ok) {
    CHECK(hist.size() == (size_t)M + 1);
    std::vector<uint32_t> qmap((size_t)M + 1, 0xdeadbeefu);
    const bool ok = sq::knot_map(M, hist.data(), qmap.data());
    CHECK(ok == expect_ok);
    g_cases++;
    if (!ok) return;
    const uint64_t top = 256u * (uint64_t)M;
    unsigned __int128 below = 0, escaped = 0;
    for (uint32_t j = 0; j < M; j++) escaped += hist[j];
    CHECK(qmap[M] == top);
    for (uint32_t j = 0; j < M; j++) {
        const uint64_t want = escaped ? (uint64_t)(((unsigned __int128)top * below) / escaped) : 0u;
        CHECK(qmap[j] == want);
        CHECK(qmap[j] <= qmap[j + 1]);
        if (hist[j]) CHECK(qmap[j] < top);
        // the integer rank map of the same table: (M * C(j)) / E
        CHECK((qmap[j] >> 8) == (escaped ? (uint64_t)(((unsigned __int128)M * below) / escaped) : 0u));
        below += hist[j];
    }
    std::vector<uint32_t> pairs((size_t)M * 2, 0xdeadbeefu);
    sq::compose_pairs(M, qmap.data(), pairs.data());
    std::vector<uint32_t> bins;   // the bins probed: the occupied ones (at most 64 of them), the first and last, some at random
    for (uint32_t j = 0; j < M && bins.size() < 64; j++)
        if (hist[j]) bins.push_back(j);
    bins.push_back(0);
    bins.push_back(M - 1);
    for (int k = 0; k < 32; k++) bins.push_back(rnd() % M);
    for (uint32_t j : bins) {
        uint32_t last = 0;
        for (uint32_t f = 0; f < 256; f++) {
            const uint32_t q = 256u * j + f;
            const uint32_t r = sq::remap(q, M, pairs.data());
            CHECK(r == qmap[j] + (uint32_t)(((uint64_t)(qmap[j + 1] - qmap[j]) * f) >> 8));
            CHECK(r >= qmap[j] && r <= qmap[j + 1] && (f == 0 || r >= last));
            if (hist[j]) CHECK(r < top);
            last = r;
        }
    }
    CHECK(sq::remap((uint32_t)top, M, pairs.data()) == top);
    if (top + 1 <= 0xffffffffull) CHECK(sq::remap((uint32_t)top + 1u, M, pairs.data()) == top);
    CHECK(sq::remap(0xffffffffu, M, pairs.data()) == top);
}

int main() {
    // M = 1
    run_case(1, {3, 5}, true);
    run_case(1, {0, 5}, true);
    run_case(1, {7, 0}, true);
    // no escaped pixel, an empty table
    {
        std::vector<uint32_t> h(101, 0);
        run_case(100, h, true);
        h[100] = 6144;
        run_case(100, h, true);
    }
    // one occupied bin: the first, one in the middle, the last
    for (uint32_t j : {0u, 37u, 99u}) {
        std::vector<uint32_t> h(101, 0);
        h[j] = 6144;
        h[100] = 9;
        run_case(100, h, true);
    }
    // more escaped pixels than palette positions: knot differences round to 0
    run_case(4, {1, 5000, 1, 1, 9}, true);
    run_case(2, {1000000, 1, 0}, true);
    // a total at 2^32 - 1 (accepted) and at 2^32 (refused); interior pixels count
    run_case(3, {0x80000000u, 0x7fffffffu, 0, 0}, true);
    run_case(3, {0xfffffffeu, 0, 1, 0}, true);
    run_case(3, {1, 0, 0, 0xfffffffeu}, true);
    run_case(3, {0x80000000u, 0x80000000u, 0, 0}, false);
    run_case(3, {1, 0, 0, 0xffffffffu}, false);
    // random tables of a few sizes
    for (uint32_t M : {2u, 3u, 17u, 255u, 4096u})
        for (int k = 0; k < 4; k++) {
            std::vector<uint32_t> h((size_t)M + 1);
            const uint32_t bits = 1u + rnd() % 18u;
            for (auto& v : h) v = (rnd() % 3u) ? (rnd() & ((1u << bits) - 1u)) : 0u;
            run_case(M, h, true);
        }
    // M = 2^24 - 1 with a sparse histogram: 256 M C(j) passes 2^63
    {
        const uint32_t M = 0x00ffffffu;
        std::vector<uint32_t> h((size_t)M + 1, 0);
        h[5] = 0xfffffffcu;
        h[1u << 20] = 2;
        h[M - 1] = 1;
        run_case(M, h, true);
        h[M] = 1;   // one interior pixel more: the total is 2^32
        run_case(M, h, false);
    }
    std::printf("mandel_smooth_equalise_host_check: %d cases OK\n", g_cases);
    return 0;
}
