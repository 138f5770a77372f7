// mc_pathtrace_accel_guides on the host (csrc/pt_bvh_guides.h, csrc/pt_bvh_host.cpp) alone, for a sanitizer: no HIP and no library.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude
//       tools/pt_accel_guides_host_check.cpp vulkan-compute-tests_amd/csrc/pt_bvh_host.cpp -o pt_accel_guides_host_check
//       && ./pt_accel_guides_host_check
// Every table and every output plane is a std::vector of exactly the size the contract names, so a record, a node or a pixel touched one
// element outside it is a heap overflow the sanitizer reports.  The border shapes of the host guides: 1 x 1, 1 x 130, 257 x 1, an odd
// 37 x 23; the scenes: a closed room of random spheres, no planes (misses), empty tables (every pixel a miss), spheres that cannot be
// boxed (a NaN centre, an infinite radius, a box that overflows, a negative radius) among finite ones; aligned and misaligned outputs.
// On every pixel the two planes are compared, word for word, with ptd::guide_pixel (the table form's arithmetic, csrc/pt_denoise.h)
// over the same tables; every refusal is made.  A failed check prints its line and exits 1; the last line of a clean run is
// "pt_accel_guides_host_check: <n> cases OK".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../vulkan-compute-tests_amd/csrc/pt_bvh_guides.h"
#include "../vulkan-compute-tests_amd/csrc/pt_bvh_host.h"

namespace mc {   // what api.hip and pt_bvh.hip give the library build
static std::string g_detail;
void set_error_detail(const std::string& s) { g_detail = s; }
void pt_accel_release_device(const mc_pathtrace_accel*) {}
uint32_t pt_accel_device_copies(const mc_pathtrace_accel*) { return 0; }
}  // namespace mc

using mc::ptd::vec4;

static int g_cases = 0;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::printf("pt_accel_guides_host_check: line %d: %s\n", __LINE__, #cond);  \
            std::exit(1);                                                               \
        }                                                                               \
    } while (0)

static uint32_t g_seed = 4242u;
static float rnd() {
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)(g_seed >> 8) * (1.0f / 16777216.0f);
}
static float rnd(float lo, float hi) { return lo + (hi - lo) * rnd(); }

static const float kRoom[6 * 12] = {
    -1, 0, 0, 2.6f, 0, 0, 0, 0, .85f, .25f, .25f, 1, 1, 0, 0, 2.6f, 0, 0, 0, 0, .25f, .35f, .85f, 1, 0, 1,  0, 2.0f, 0, 0, 0, 0, .75f, .75f, .75f, 1,
    0,  -1, 0, 2.0f, 0, 0, 0, 0, .75f, .75f, .75f, 1, 0, 0, -1, 2.8f, 0, 0, 0, 0, .85f, .85f, .25f, 1, 0, 0, 1, 7.9f, 0, 0, 0, 0, .1f,  .7f,  .7f,  1};

static std::vector<float> random_spheres(uint32_t n) {
    std::vector<float> s(12 * (size_t)n, 0.0f);
    for (uint32_t i = 0; i < n; i++) {
        float* r = s.data() + 12 * (size_t)i;
        r[0] = rnd(-2.2f, 2.2f); r[1] = rnd(-1.8f, 1.2f); r[2] = rnd(-2.4f, 2.5f); r[3] = rnd(0.05f, 0.35f);
        r[8] = r[9] = r[10] = 0.6f; r[11] = 1.0f;
    }
    return s;
}

struct Counts { size_t sphere = 0, plane = 0, miss = 0; };

// The accel guides of (planes, spheres) at W x H against the table form's arithmetic, every word; outputs at byte offset `shift` (0 or 4)
// of their allocation, so that both the in-place and the copied path of a misaligned plane run.
static void compare(const std::vector<float>& planes, const std::vector<float>& spheres, uint32_t W, uint32_t H, size_t shift, Counts& seen) {
    const uint32_t np = (uint32_t)(planes.size() / 12), ns = (uint32_t)(spheres.size() / 12);
    mc_pathtrace_accel* a = nullptr;
    CHECK(mc_pathtrace_accel_create(planes.data(), np, spheres.data(), ns, &a) == MC_OK && a);
    const size_t npix = (size_t)W * H, words = npix * 4;
    // exactly the plane (plus the shift in front): the last pixel's last word is the allocation's last
    std::vector<float> nt(words + shift / 4, -7.0f), pid(words + shift / 4, -7.0f);
    CHECK(mc_pathtrace_accel_guides(a, W, H, nt.data() + shift / 4, pid.data() + shift / 4) == MC_OK);
    for (size_t k = 0; k < shift / 4; k++) CHECK(nt[k] == -7.0f && pid[k] == -7.0f);
    std::vector<float> rec(planes);
    rec.insert(rec.end(), spheres.begin(), spheres.end());
    const mc::ptd::Camera cam = mc::ptd::camera();
    for (uint32_t gy = 0; gy < H; gy++)
        for (uint32_t gx = 0; gx < W; gx++) {
            vec4 want_nt, want_pid;
            mc::ptd::guide_pixel(cam, W, H, gx, gy, rec.data(), np, ns, want_nt, want_pid);
            const size_t gid = (size_t)(H - 1u - gy) * W + gx;
            CHECK(std::memcmp(nt.data() + shift / 4 + 4 * gid, &want_nt, 16) == 0);
            CHECK(std::memcmp(pid.data() + shift / 4 + 4 * gid, &want_pid, 16) == 0);
            if (want_pid.w < 0.0f) {
                seen.miss++;
                CHECK(want_nt.x == 0.0f && want_nt.y == 0.0f && want_nt.z == 0.0f && want_nt.w == 1e20f);
            } else if (want_pid.w >= (float)np) seen.sphere++;
            else seen.plane++;
        }
    CHECK(mc_pathtrace_accel_destroy(a) == MC_OK);
    g_cases++;
}

int main() {
    const std::vector<float> room(kRoom, kRoom + 72), none;
    const std::vector<float> many = random_spheres(300);
    std::vector<float> unboxable = random_spheres(24);
    unboxable[12 * 3 + 0] = std::numeric_limits<float>::quiet_NaN();
    unboxable[12 * 7 + 3] = std::numeric_limits<float>::infinity();
    unboxable[12 * 11 + 0] = 3.0e38f; unboxable[12 * 11 + 1] = 0.0f; unboxable[12 * 11 + 2] = 0.0f; unboxable[12 * 11 + 3] = 3.0e38f;
    unboxable[12 * 15 + 3] = -unboxable[12 * 15 + 3];
    const uint32_t shapes[][2] = {{1, 1}, {1, 130}, {257, 1}, {37, 23}};
    Counts seen;
    for (const auto& wh : shapes)
        for (size_t shift : {(size_t)0, (size_t)4}) {
            compare(room, many, wh[0], wh[1], shift, seen);         // a closed room
            compare(none, many, wh[0], wh[1], shift, seen);         // no planes: rays between the spheres miss
            compare(none, none, wh[0], wh[1], shift, seen);         // empty tables: every pixel a miss
            compare(room, none, wh[0], wh[1], shift, seen);         // planes alone: no tree
            compare(room, unboxable, wh[0], wh[1], shift, seen);    // the second linear list beside the tree
            compare(none, unboxable, wh[0], wh[1], shift, seen);
        }
    CHECK(seen.sphere > 0 && seen.plane > 0 && seen.miss > 0);
    // refusals
    {
        mc_pathtrace_accel* a = nullptr;
        CHECK(mc_pathtrace_accel_create(room.data(), 6, many.data(), 300, &a) == MC_OK);
        std::vector<float> nt(4 * 8), pid(4 * 8);
        CHECK(mc_pathtrace_accel_guides(nullptr, 4, 2, nt.data(), pid.data()) == MC_ERR_INVALID_ARGUMENT);
        CHECK(mc_pathtrace_accel_guides(a, 0, 2, nt.data(), pid.data()) == MC_ERR_INVALID_ARGUMENT);
        CHECK(mc_pathtrace_accel_guides(a, 4, 0, nt.data(), pid.data()) == MC_ERR_INVALID_ARGUMENT);
        CHECK(mc_pathtrace_accel_guides(a, 4, 2, nullptr, pid.data()) == MC_ERR_INVALID_ARGUMENT);
        CHECK(mc_pathtrace_accel_guides(a, 4, 2, nt.data(), nullptr) == MC_ERR_INVALID_ARGUMENT);
        CHECK(mc_pathtrace_accel_guides(a, 4, 2, nt.data(), pid.data()) == MC_OK);
        CHECK(mc_pathtrace_accel_destroy(a) == MC_OK);
        CHECK(mc_pathtrace_accel_guides(a, 4, 2, nt.data(), pid.data()) == MC_ERR_INVALID_ARGUMENT);   // destroyed: the pointer is only looked up
        CHECK(mc::g_detail.find("destroyed") != std::string::npos);
        g_cases++;
    }
    std::printf("pt_accel_guides_host_check: pixels with a sphere / a plane / nothing as first hit: %zu / %zu / %zu\n", seen.sphere, seen.plane,
                seen.miss);
    std::printf("pt_accel_guides_host_check: %d cases OK\n", g_cases);
    return 0;
}
