// The exact counts' host code and the lane-loop form of both device kernels' arithmetic alone, for a sanitizer: this file,
// csrc/mandel_orbit.cpp and the two headers of the shared arithmetic; no HIP, no device and no library.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Wno-unknown-pragmas -Iinclude
//       tools/mandel_exact_host_check.cpp vulkan-compute-tests_amd/csrc/mandel_orbit.cpp -o mandel_exact_host_check
//       && ./mandel_exact_host_check
// (tests/test_mandel_exact_sanitized.py does exactly that).  Checked against FixOps (mandel_orbit.cpp):
//  * the wave kernel's rounded products a b, a^2, b^2 for n = 2 .. 16 on random and crafted operands: zero, one unit in the last place,
//    all-ones limbs (every column at its largest), operands whose product's carries ripple through the full length;
//  * the workgroup kernel's rounded product (mul_phase) at n = 17, 18 and 131 on the same kinds of operands;
//  * both kernels' whole iteration as counts, n = 2 .. 18 and 131 (the wave kernel up to 16, the workgroup kernel from 2 up: its
//    arithmetic has no lower bound), on c's of both signs that escape at once, after a few iterations and never;
//  * the public calls on the same c's, with every array of exactly the size the call reads or writes.
// A failed check prints its line and exits 1; the last line of a clean run is "mandel_exact_host_check: <n> cases OK".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../vulkan-compute-tests_amd/csrc/mandel_exact_fix.h"
#include "../vulkan-compute-tests_amd/csrc/mandel_orbit.h"

static std::string g_detail;
void mc::set_error_detail(const std::string& s) { g_detail = s; }

static int g_cases = 0;
#define CHECK(cond)                                                                                        \
    do {                                                                                                   \
        if (!(cond)) {                                                                                     \
            std::printf("mandel_exact_host_check: line %d: %s  [%s]\n", __LINE__, #cond, g_detail.c_str()); \
            std::exit(1);                                                                                  \
        }                                                                                                  \
    } while (0)

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {   // splitmix64
    uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

using Limbs = std::vector<uint64_t>;

// |value| < 8, as every number of the iteration is: the integer limb holds at most 7.
static Limbs operand(int n, int kind) {
    Limbs a((size_t)n, 0u);
    switch (kind) {
        case 0: break;                                                       // zero
        case 1: a[0] = 1; break;                                             // one unit in the last place
        case 2: for (int i = 0; i < n - 1; i++) a[i] = ~0ull; a[n - 1] = 7; break;   // all ones
        case 3: for (int i = 0; i < n - 1; i++) a[i] = ~0ull; break;         // 1 - 2^-F: squares to 1 - 2^(1-F) + 2^-2F, a full ripple
        case 4: a[n - 1] = 1; break;                                         // exactly 1
        case 5: a[n - 1] = 1; a[0] = 1; break;                               // 1 + 2^-F
        case 6: a[n - 2 < 0 ? 0 : n - 2] = 1ull << 63; break;                // exactly 1/2: the rounding bit's own weight
        default:
            for (int i = 0; i < n - 1; i++) a[i] = rnd();
            a[n - 1] = rnd() % 8;
            if (kind & 1) a[(size_t)(rnd() % (uint64_t)n)] = ~0ull >> (rnd() % 64);   // a run of ones somewhere
            if (n > 1 && (kind & 2)) a[(size_t)(rnd() % (uint64_t)(n - 1))] = 0;
            a[n - 1] %= 8;
            break;
    }
    return a;
}

static void check_wave_products(int n) {
    const int kinds = 7 + 24;
    Limbs ab((size_t)n), aa((size_t)n), bb((size_t)n), want((size_t)n);
    for (int ka = 0; ka < kinds; ka++)
        for (int kb = 0; kb < (ka < 7 ? kinds : 8); kb++) {
            const Limbs a = operand(n, ka), b = operand(n, kb);
            mc::exactfix::wave_mul_lanes(n, a.data(), b.data(), ab.data(), aa.data(), bb.data());
            mc::fix_mul_round(n, a.data(), b.data(), want.data());
            CHECK(ab == want);
            mc::fix_mul_round(n, a.data(), a.data(), want.data());
            CHECK(aa == want);
            mc::fix_mul_round(n, b.data(), b.data(), want.data());
            CHECK(bb == want);
            g_cases++;
        }
}

// The workgroup kernel's rounded product (mandel_orbit_fix.h: mul_phase, a in zx, b in zy, the result in pr) on the same operand kinds.
static void check_group_products(int n) {
    namespace of = mc::orbitfix;
    of::Mem* m = new of::Mem();
    const int kinds = 7 + 8;
    Limbs got((size_t)n), want((size_t)n);
    for (int ka = 0; ka < kinds; ka++)
        for (int kb = 0; kb < (n > 18 && ka >= 7 ? 2 : kinds); kb++) {
            const Limbs a = operand(n, ka), b = operand(n, kb);
            *m = of::Mem();
            m->k = n - 1;
            m->H = 2 * n;
            for (int i = 0; i < n; i++) {
                m->zx[2 * i] = (uint32_t)a[i]; m->zx[2 * i + 1] = (uint32_t)(a[i] >> 32);
                m->zy[2 * i] = (uint32_t)b[i]; m->zy[2 * i + 1] = (uint32_t)(b[i] >> 32);
            }
            for (int ph = 0; ph < 3; ph++)
                for (int lane = 0; lane < of::kLanes; lane++) of::mul_phase(*m, ph, lane);
            for (int i = 0; i < n; i++) got[i] = (uint64_t)m->pr[2 * i] | ((uint64_t)m->pr[2 * i + 1] << 32);
            mc::fix_mul_round(n, a.data(), b.data(), want.data());
            CHECK(got == want);
            g_cases++;
        }
    delete m;
}

// value * 2^F for a small rational p / 2^q, q <= 60, |p / 2^q| < 8
static Limbs fixed(int n, uint64_t p, int q) {
    Limbs a((size_t)n, 0u);
    // p * 2^(64 (n - 1) - q): the top limb gets p >> q, the one below the remainder
    a[n - 1] = p >> q;
    if (n > 1 && q > 0) a[n - 2] = (p & ((1ull << q) - 1ull)) << (64 - q);
    return a;
}

struct C0 {
    uint64_t px; int qx; bool nx;
    uint64_t py; int qy; bool ny;
};

static void check_counts(int n, uint32_t M) {
    static const C0 cs[] = {
        {0, 0, false, 0, 0, false},                 // 0: never
        {1, 0, true, 0, 0, false},                  // -1: the 2-cycle, never
        {3, 1, false, 0, 0, false},                 // 1.5: |c|^2 > 2, n = 0
        {1, 0, false, 1, 0, false},                 // 1 + i: |c|^2 = 2 exactly, n = 1
        {1, 0, false, 1, 0, true},                  // 1 - i
        {3, 2, true, 1, 3, false},                  // -0.75 + 0.125 i: slow
        {0x5f3759dfull, 32, true, 0x0a3d70a3ull, 32, false},   // near the seahorse valley
        {0x1ull << 28 | 12345, 30, false, 99999, 20, true},
        {7, 2, true, 0, 0, false},                  // -1.75: the period-3 window's neighbourhood
        {1, 2, false, 1, 1, false},                 // 0.25 + 0.5 i
    };
    for (const C0& c : cs) {
        Limbs cx = fixed(n, c.px, c.qx), cy = fixed(n, c.py, c.qy);
        if (n > 2) { cx[0] = rnd(); cy[0] = rnd(); cx[1] ^= rnd() >> 40; }   // bits in the lowest limbs: full-length operands
        bool zx = true, zy = true;
        for (uint64_t v : cx) zx = zx && v == 0;
        for (uint64_t v : cy) zy = zy && v == 0;
        const bool nx = c.nx && !zx, ny = c.ny && !zy;
        const uint32_t want = mc::exact_count_host(n, cx.data(), cy.data(), nx, ny, M);
        CHECK(want <= M);
        if (n <= mc::exactfix::kWaveMaxLimbs) CHECK(mc::exactfix::wave_count_lanes(n, cx.data(), cy.data(), nx, ny, M) == want);
        CHECK(mc::exactfix::group_count_lanes(n, cx.data(), cy.data(), nx, ny, M) == want);
        if (want >= 1 && want < M) {   // the loop's ends: M placed on the escape and one either side of it
            for (uint32_t m2 : {want, want + 1u, want > 1 ? want - 1u : 1u}) {
                const uint32_t w2 = mc::exact_count_host(n, cx.data(), cy.data(), nx, ny, m2);
                CHECK(w2 == (m2 <= want ? m2 : want));
                if (n <= mc::exactfix::kWaveMaxLimbs) CHECK(mc::exactfix::wave_count_lanes(n, cx.data(), cy.data(), nx, ny, m2) == w2);
                CHECK(mc::exactfix::group_count_lanes(n, cx.data(), cy.data(), nx, ny, m2) == w2);
            }
        }
        g_cases++;
    }
}

static void check_public_calls() {
    mc_mandelbrot_orbit* o = nullptr;
    CHECK(mc_mandelbrot_orbit_create("-0.7436438870371587", "0.13182590420531198", 1e-8, 1e-8, 50, &o) == MC_OK);
    const uint32_t W = 24, H = 16, N = 7;
    std::vector<uint32_t> gx(N), gy(N), out(N, 77u), lanes(N);
    for (uint32_t i = 0; i < N; i++) { gx[i] = (5 * i) % W; gy[i] = (3 * i) % H; }
    std::vector<double> dcx(N, -1.0), dcy(N, -1.0);
    int32_t e = 9;
    CHECK(mc_mandelbrot_exact_pixel_offsets(o, W, H, N, gx.data(), gy.data(), dcx.data(), dcy.data(), &e) == MC_OK && e == 0);
    for (uint32_t extra : {0u, 1u, 2u, 128u}) {
        CHECK(mc_mandelbrot_exact_counts(o, 40, extra, N, dcx.data(), dcy.data(), e, out.data()) == MC_OK);
        mc::ExactPixels px;
        CHECK(mc::exact_prepare("check", o, 40, extra, N, dcx.data(), dcy.data(), e, out.data(), &px) == MC_OK);
        CHECK(px.n == 3 + (int)extra);
        for (uint32_t p = 0; p < N; p++) {
            const uint64_t* x = &px.cx[(size_t)p * px.n];
            const uint64_t* y = &px.cy[(size_t)p * px.n];
            if (px.n <= mc::exactfix::kWaveMaxLimbs)
                CHECK(mc::exactfix::wave_count_lanes(px.n, x, y, px.cx_neg[p] != 0, px.cy_neg[p] != 0, 40) == out[p]);
            CHECK(mc::exactfix::group_count_lanes(px.n, x, y, px.cx_neg[p] != 0, px.cy_neg[p] != 0, 40) == out[p]);
        }
        g_cases++;
    }
    gx[N - 1] = W;
    CHECK(mc_mandelbrot_exact_pixel_offsets(o, W, H, N, gx.data(), gy.data(), dcx.data(), dcy.data(), &e) == MC_ERR_INVALID_ARGUMENT);
    CHECK(mc_mandelbrot_exact_counts(o, 40, 129, N, dcx.data(), dcy.data(), 0, out.data()) == MC_ERR_UNSUPPORTED);
    CHECK(mc_mandelbrot_exact_counts(o, 40, 0, N, dcx.data(), dcy.data(), -2000, out.data()) == MC_ERR_UNSUPPORTED);
    CHECK(mc_mandelbrot_exact_counts(o, 40, 0, N, dcx.data(), dcy.data(), 60, out.data()) == MC_ERR_UNSUPPORTED);
    CHECK(mc_mandelbrot_exact_counts(o, 40, 0, N, dcx.data(), dcy.data(), 2000000000, out.data()) == MC_ERR_UNSUPPORTED);
    CHECK(mc_mandelbrot_exact_counts(o, 40, 0, N, dcx.data(), dcy.data(), -2000000000, out.data()) == MC_ERR_UNSUPPORTED);
    CHECK(mc_mandelbrot_exact_counts(o, 0, 0, N, dcx.data(), dcy.data(), 0, out.data()) == MC_ERR_INVALID_ARGUMENT);
    CHECK(mc_mandelbrot_exact_counts(o, 40, 0, 0, dcx.data(), dcy.data(), 0, out.data()) == MC_ERR_INVALID_ARGUMENT);
    mc_mandelbrot_orbit* r = nullptr;
    CHECK(mc_mandelbrot_orbit_rescale(o, 1e-7, 1e-7, 0, &r) == MC_OK);
    mc_mandelbrot_orbit_destroy(o);   // the copy owns its centre
    dcx.assign(N, 0.0); dcy.assign(N, 0.0);
    CHECK(mc_mandelbrot_exact_counts(r, 40, 0, N, dcx.data(), dcy.data(), 0, out.data()) == MC_OK && out[0] == 40);
    mc_mandelbrot_orbit_destroy(r);
    g_cases++;
}

int main() {
    for (int n = 2; n <= 16; n++) check_wave_products(n);
    for (int n : {17, 18, 131}) check_group_products(n);
    for (int n = 2; n <= 18; n++) check_counts(n, 60);
    check_counts(131, 12);
    check_public_calls();
    std::printf("mandel_exact_host_check: %d cases OK\n", g_cases);
    return 0;
}
