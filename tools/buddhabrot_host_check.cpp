// The Buddhabrot's host path (csrc/buddhabrot_host.cpp + csrc/buddhabrot.h) alone, for a sanitizer: no HIP and no library.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude
//       tools/buddhabrot_host_check.cpp vulkan-compute-tests_amd/csrc/buddhabrot_host.cpp -o buddhabrot_host_check && ./buddhabrot_host_check
// Every plane, map and image is a std::vector of exactly the size the contract names, so a bin, a map entry or a pixel one word outside
// it is a heap overflow the sanitizer reports.  The bin index is where an out-of-bounds store would hide: the shapes are the border-heavy
// ones (one bin on an axis, no round size), under views that put most orbit points just outside an edge, mirrored views, a view so
// narrow that fx overflows to infinity, sample indices across 2^32 and up to 2^64 - 1.  The contract's identities are checked on the way
// (the plane's sum is `added`, ranges compose, a refused call writes nothing).  The importance map, the cell list and the guided density
//  likewise: a map of exactly G * G words at g = 1, 6 and 12 (the shifts by 31 and 20), a list buffer of exactly the
// queried length, lists naming the grid's corner cells, the map's sum is `added`, list and complement partition the grid, a guided
// plane's sum is weight * added.  A failed check prints its line and exits 1; the last line of a clean run is
// "buddhabrot_host_check: <n> cases OK".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "mc_compute.h"

namespace mc {
static std::string g_detail;
void set_error_detail(const std::string& s) { g_detail = s; }   // (api.hip's, in the library)
}  // namespace mc

static int g_cases = 0;
#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::printf("buddhabrot_host_check: line %d: %s\n", __LINE__, #cond); \
            std::exit(1);                                                         \
        }                                                                         \
    } while (0)

static uint64_t sum(const std::vector<uint32_t>& v) {
    uint64_t s = 0;
    for (uint32_t x : v) s += x;
    return s;
}

static void density_case(uint32_t W, uint32_t H, const double view[4], uint64_t begin, uint64_t n, uint32_t M, uint32_t min_iter) {
    mc_buddhabrot_params p;
    CHECK(mc_buddhabrot_default_params(W, H, n, &p) == MC_OK);
    p.view_centre_x = view[0]; p.view_centre_y = view[1]; p.view_scale_x = view[2]; p.view_scale_y = view[3];
    p.sample_begin = begin; p.sample_end = begin + n;
    p.max_iter = M; p.min_iter = min_iter; p.seed = 7;
    std::vector<uint32_t> whole((size_t)W * H, 0), parts((size_t)W * H, 0);
    mc_buddhabrot_stats sw = {0, 0, 0, 0, 0}, sp = {0, 0, 0, 0, 0};
    CHECK(mc_buddhabrot_density(&p, whole.data(), &sw) == MC_OK);
    CHECK(sw.samples == n && sw.skipped + sw.contributing <= n && sw.added <= sw.points && sum(whole) == sw.added);
    if (min_iter >= M || M == 1) CHECK(sw.points == 0 && sw.added == 0);
    p.sample_end = begin + n / 3;
    CHECK(mc_buddhabrot_density(&p, parts.data(), &sp) == MC_OK);
    p.sample_begin = begin + n / 3; p.sample_end = begin + n;
    CHECK(mc_buddhabrot_density(&p, parts.data(), &sp) == MC_OK);
    CHECK(parts == whole && sp.samples == sw.samples && sp.skipped == sw.skipped && sp.contributing == sw.contributing &&
          sp.points == sw.points && sp.added == sw.added);
    g_cases++;
}

// The importance map at grid g (its plane EQUAL to the uniform call's), the list and its complement for two thresholds and dilations, and
// the guided density over the list, over the complement and over the corner cells, ranges across 2^32 included.
static void guided_case(uint32_t W, uint32_t H, const double view[4], uint32_t g, uint64_t begin, uint64_t n, uint32_t M) {
    mc_buddhabrot_params p;
    CHECK(mc_buddhabrot_default_params(W, H, n, &p) == MC_OK);
    p.view_centre_x = view[0]; p.view_centre_y = view[1]; p.view_scale_x = view[2]; p.view_scale_y = view[3];
    p.sample_begin = begin; p.sample_end = begin + n;
    p.max_iter = M; p.seed = 7;
    const size_t cells_all = (size_t)1 << (2 * g);
    std::vector<uint32_t> map(cells_all, 0), again(cells_all, 0), plane((size_t)W * H, 0), uniform((size_t)W * H, 0);
    mc_buddhabrot_stats si = {0, 0, 0, 0, 0}, su = {0, 0, 0, 0, 0}, sn = {0, 0, 0, 0, 0};
    CHECK(mc_buddhabrot_importance(&p, g, map.data(), plane.data(), &si) == MC_OK);
    CHECK(mc_buddhabrot_density(&p, uniform.data(), &su) == MC_OK);
    CHECK(plane == uniform && si.samples == su.samples && si.skipped == su.skipped && si.contributing == su.contributing &&
          si.points == su.points && si.added == su.added && sum(map) == si.added);
    CHECK(mc_buddhabrot_importance(&p, g, again.data(), nullptr, &sn) == MC_OK);   // no plane: the same map, the same statistics
    CHECK(again == map && sn.added == si.added && sn.points == si.points);
    for (uint32_t threshold : {1u, 3u})
        for (uint32_t dilate : {0u, 1u, 8u}) {
            if (g == 12 && (threshold != 1 || dilate == 8)) continue;   // (16 M cells: one threshold, the short dilations)
            uint32_t n_list = 0, n_comp = 0, n_again = 0;
            CHECK(mc_buddhabrot_importance_cells(g, map.data(), threshold, dilate, 0, nullptr, &n_list) == MC_OK);
            CHECK(mc_buddhabrot_importance_cells(g, map.data(), threshold, dilate, MC_BUDDHA_CELLS_COMPLEMENT, nullptr, &n_comp) == MC_OK);
            CHECK((size_t)n_list + n_comp == cells_all);
            std::vector<uint32_t> list(n_list), comp(n_comp);   // exactly the queried lengths
            CHECK(mc_buddhabrot_importance_cells(g, map.data(), threshold, dilate, 0, list.data(), &n_again) == MC_OK && n_again == n_list);
            CHECK(mc_buddhabrot_importance_cells(g, map.data(), threshold, dilate, MC_BUDDHA_CELLS_COMPLEMENT, comp.data(), &n_again) == MC_OK &&
                  n_again == n_comp);
            for (size_t j = 0; j < list.size(); j++) CHECK(list[j] < cells_all && (!j || list[j] > list[j - 1]));
            for (size_t j = 0; j < comp.size(); j++) CHECK(comp[j] < cells_all && (!j || comp[j] > comp[j - 1]));
            if (!dilate)
                for (uint32_t c : list) CHECK(map[c] >= threshold);
            for (const std::vector<uint32_t>* which : {&list, &comp}) {
                if (which->empty() || dilate == 8) continue;
                for (uint32_t weight : {1u, 5u, 0x80000000u}) {
                    std::vector<uint32_t> guided((size_t)W * H, 0);
                    mc_buddhabrot_stats sg = {0, 0, 0, 0, 0};
                    CHECK(mc_buddhabrot_density_guided(&p, which->data(), (uint32_t)which->size(), g, weight, guided.data(), &sg) == MC_OK);
                    CHECK(sg.samples == n && sg.added <= sg.points && (uint32_t)sum(guided) == (uint32_t)(sg.added * weight));
                }
            }
        }
    const uint32_t corners[5] = {0u, (1u << g) - 1u, (uint32_t)cells_all - (1u << g), (uint32_t)cells_all - 1u, 0u};
    std::vector<uint32_t> guided((size_t)W * H, 0);
    mc_buddhabrot_stats sg = {0, 0, 0, 0, 0};
    CHECK(mc_buddhabrot_density_guided(&p, corners, 5, g, 1, guided.data(), &sg) == MC_OK && sum(guided) == sg.added);
    g_cases++;
}

static void tone_case(uint32_t W, uint32_t H, uint32_t L) {
    std::vector<uint32_t> m0((size_t)L + 1), m1((size_t)L + 1), d0((size_t)W * H), d1((size_t)W * H);
    CHECK(mc_buddhabrot_sqrt_map(L, m0.data()) == MC_OK);
    CHECK(m0[0] == 0 && m0[L] == L);
    for (uint32_t j = 0; j <= L; j++) {
        CHECK(m0[j] <= L && (!j || m0[j] >= m0[j - 1]));
        m1[j] = L - j;
    }
    for (size_t i = 0; i < d0.size(); i++) {
        d0[i] = (uint32_t)(i * 2654435761u) % (2 * L + 3);   // below, at and above L
        d1[i] = i % 3 ? 0xffffffffu : (uint32_t)i;
    }
    std::vector<float> out((size_t)W * H * 4, -1.0f);
    CHECK(mc_buddhabrot_tonemap(W, H, d0.data(), d1.data(), d0.data(), L, m0.data(), m1.data(), m0.data(), out.data()) == MC_OK);
    for (size_t i = 0; i < d0.size(); i++) {
        CHECK(out[4 * i + 3] == 1.0f && out[4 * i] == out[4 * i + 2]);
        for (int c = 0; c < 3; c++) CHECK(out[4 * i + c] >= 0.0f && out[4 * i + c] <= 1.0f);
        CHECK(out[4 * i] == (float)m0[d0[i] > L ? L : d0[i]] / (float)L);
    }
    m1[L / 2] = L + 1;   // refused before a pixel is written
    std::vector<float> untouched((size_t)W * H * 4, -1.0f);
    CHECK(mc_buddhabrot_tonemap(W, H, d0.data(), d1.data(), d0.data(), L, m0.data(), m1.data(), m0.data(), untouched.data()) == MC_ERR_INVALID_ARGUMENT);
    for (float v : untouched) CHECK(v == -1.0f);
    g_cases++;
}

int main() {
    const uint32_t shapes[][2] = {{1, 1}, {1, 7}, {7, 1}, {2, 2}, {7, 5}, {65, 3}, {48, 32}};
    const double views[][4] = {
        {-0.5, 0.0, 3.0, 2.0},        // the default picture
        {-0.5, 0.0, -3.0, -2.0},      // mirrored on both axes
        {1.9, 1.9, 0.5, 0.5},         // a corner of the escape disc: most points just outside an edge
        {-2.0, 0.0, 0.01, 4.0},       // a sliver on the disc's rim
        {0.0, 0.0, 1e-300, 1e-300},   // kx overflows: fx is infinite or NaN except at z = the centre
        {0.0, 0.0, 1e300, 1e300},     // every point in the middle bin
    };
    for (const auto& s : shapes)
        for (const auto& v : views) {
            density_case(s[0], s[1], v, 0, 3000, 64, 0);
            density_case(s[0], s[1], v, (5ull << 32) - 17, 65, 200, 3);
            density_case(s[0], s[1], v, ~0ull - 300, 300, 32, 31);    // k up to 2^64 - 1; only n = M - 1 contributes
            density_case(s[0], s[1], v, 100, 500, 16, 16);            // min_iter = M: nothing is added
            density_case(s[0], s[1], v, 100, 500, 1, 0);              // M = 1: nothing is plotted
        }
    for (const auto& s : {shapes[0], shapes[4], shapes[5]})
        for (const auto& v : {views[0], views[1], views[2], views[4]})
            for (uint32_t g : {1u, 6u}) {
                guided_case(s[0], s[1], v, g, 0, 2000, 64);
                guided_case(s[0], s[1], v, g, (5ull << 32) - 17, 65, 200);
                guided_case(s[0], s[1], v, g, ~0ull - 300, 300, 32);
            }
    guided_case(7, 5, views[0], 12, 0, 2000, 64);   // the largest grid once: shifts by 20, a map of 2^24 words
    for (uint32_t L : {1u, 2u, 3u, 255u, 1000u}) {
        tone_case(1, 1, L);
        tone_case(65, 3, L);
    }
    // refusals write nothing and name their field
    mc_buddhabrot_params p;
    CHECK(mc_buddhabrot_default_params(4, 4, 10, &p) == MC_OK);
    std::vector<uint32_t> plane(16, 0);
    p.width = 0;
    CHECK(mc_buddhabrot_density(&p, plane.data(), nullptr) == MC_ERR_INVALID_ARGUMENT && mc::g_detail.find("width is 0") != std::string::npos);
    p.width = 4; p.view_scale_y = NAN;
    CHECK(mc_buddhabrot_density(&p, plane.data(), nullptr) == MC_ERR_INVALID_ARGUMENT && mc::g_detail.find("view_scale_y") != std::string::npos);
    CHECK(sum(plane) == 0);
    std::vector<uint32_t> one(2);
    CHECK(mc_buddhabrot_sqrt_map(0, one.data()) == MC_ERR_INVALID_ARGUMENT && mc_buddhabrot_sqrt_map(1, one.data()) == MC_OK);
    // the guided calls' refusals: nothing is written, the field is named
    p.view_scale_y = 2.0;
    std::vector<uint32_t> map4(16, 0), out4(16, 0);
    uint32_t n4 = 99;
    const uint32_t beyond[2] = {3u, 16u};
    CHECK(mc_buddhabrot_importance(&p, 0, map4.data(), plane.data(), nullptr) == MC_ERR_INVALID_ARGUMENT && mc::g_detail.find("grid_log2") != std::string::npos);
    CHECK(mc_buddhabrot_importance(&p, 13, map4.data(), plane.data(), nullptr) == MC_ERR_INVALID_ARGUMENT);
    CHECK(mc_buddhabrot_importance_cells(2, map4.data(), 0, 0, 0, out4.data(), &n4) == MC_ERR_INVALID_ARGUMENT && mc::g_detail.find("threshold is 0") != std::string::npos);
    CHECK(mc_buddhabrot_importance_cells(2, map4.data(), 1, 9, 0, out4.data(), &n4) == MC_ERR_INVALID_ARGUMENT && n4 == 99);
    CHECK(mc_buddhabrot_importance_cells(2, map4.data(), 1, 8, 0, out4.data(), &n4) == MC_OK && n4 == 0);   // an empty result is valid
    CHECK(mc_buddhabrot_density_guided(&p, beyond, 2, 2, 1, plane.data(), nullptr) == MC_ERR_INVALID_ARGUMENT && mc::g_detail.find("outside the grid") != std::string::npos);
    CHECK(mc_buddhabrot_density_guided(&p, beyond, 0, 2, 1, plane.data(), nullptr) == MC_ERR_INVALID_ARGUMENT);
    CHECK(mc_buddhabrot_density_guided(&p, beyond, 1, 2, 0, plane.data(), nullptr) == MC_ERR_INVALID_ARGUMENT);
    CHECK(sum(plane) == 0 && sum(map4) == 0 && sum(out4) == 0);
    mc_buddhabrot_guide_params gp;
    CHECK(mc_buddhabrot_guide_default_params(&gp) == MC_OK && gp.grid_log2 == 8 && gp.pilot_samples == (1ull << 24) && gp.threshold == 1 &&
          gp.dilate == 1 && gp.complement_weight == 0);
    g_cases++;
    std::printf("buddhabrot_host_check: %d cases OK\n", g_cases);
    return 0;
}
