// Entry point — same shape as the reference's src/main.cpp:15-41: mode selected by macro, the path
// tracer takes argv[1] = spp (default 500) and argv[2] = resy (default 600) with resx = resy*3/2, the
// Mandelbrot app renders 2000x2000; lifecycle init() -> preRun() -> run() -> saveRenderedImage();
// std::runtime_error -> message + EXIT_FAILURE.  Options (never reinterpreting the two positional
// arguments) expose what the reference hard-codes: --gpus N, --out FILE, --quiet, and per mode
// --width/--height/--max-iter/--centre X Y/--scale SX SY/--precision f32|ds|f64|perturb|perturb-bla|perturb-bla-deep (perturb, perturb-bla-deep: X Y are decimal text; SX SY may lie below the doubles, e.g. 1e-1000; perturb-bla: the same text, SX SY >= 2^-960), --colour reference|equalised|smooth|distance|smooth-equalised (smooth-equalised: the smooth count ranked among the image's escaped pixels; equalised: histogram-equalised colouring of the whole image; smooth: fractional escape counts, no bands; distance: the smooth colour darkened where the boundary is closer than a pixel), --supersample 1|2|4|8 (S x S samples per pixel, box-filtered on the device), --adaptive (with --supersample 2|4|8: only pixels whose count differs from a neighbour's are sampled S x S), --orbit host|device|auto (where the perturbation precisions compute their reference orbit)  or  --math strict|fast|careful,
// --zoom K F (the Mandelbrot app: --centre / --scale is the DEEPEST of K + 1 keyframes one octave apart; K * F + 1 frames, each composed on
// the device from the two keyframes that bracket it and written as <out>_%05u.<ext>), --zoom-keyframes colours|counts
// (counts: the keyframes are kept as count planes and every frame is coloured through one map blended from theirs),
// --zoom-filter bilinear|area (area: the minified deep keyframe is filtered over each pixel's footprint),
// --supersample-smooth (with --supersample 2|4|8 and --colour smooth|smooth-equalised: the samples are smooth counts),
// --buddhabrot SAMPLES (the Mandelbrot app: the orbit-density plane of SAMPLES pseudo-random c instead of the set, DESIGN.md §3.26;
// --centre / --scale / --width / --height / --max-iter / --out / --gpu-postprocess mean what they mean without it, the defaults being the
// library's view (-0.5, 0, 3, 3 H / W) and max_iter 1000), with --min-iter m, --seed s, --sample-window CX CY SX SY (where c is drawn
// from; default -0.5 0 4 4), --nebula MR MG MB (three renders of those max_iter, one per colour channel), --tone sqrt|equalised
// (default sqrt) and --white PCT (default 99.9: the white level L is the density not exceeded by PCT % of the non-empty bins, read from
// one histogram capped at 2^20 - 1 — the app's policy, not the library's), and for zoomed views --guided[=G] with --pilot P, --dilate D,
// --unbiased B (mc_buddhabrot_render_guided, DESIGN.md §3.27: a pilot's importance map over the 2^G x 2^G cells of the sample window,
// the samples drawn from the cells whose orbits reach the view), --locate[=N] (the Mandelbrot app with --precision f32|f64|perturb: after
// the save, the N largest atom domains of the view, their periods, the nucleus Newton's method finds from each one's best pixel and a
// ready --centre X Y for the dive); --help prints this list,
// --large-sphere-walls, --sphere-precision f32|fp64|ds|df64 (the reference's compile-time precision experiment);
// --reference-png writes the file through the reference's own lodepng (a build with `make REFERENCE=<checkout>`): its bytes.
// A value none of these lists name is an error (EXIT_FAILURE) — never a silent default.
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cmath>
#include <cstdlib>
#include <initializer_list>
#include <utility>
#include <cstring>
#include <stdexcept>
#include <memory>
#include <string>
#include <vector>

// make sure that one token is defined
#if !defined(MANDELBROT_MODE) && !defined(PATHTRACER_MODE)
#define PATHTRACER_MODE
#endif

#if defined(MANDELBROT_MODE)
#include "mandelbrotApp.h"
#elif defined(PATHTRACER_MODE)
#include "pathtracerApp.h"
#endif

int main(int argc, char* argv[]) {
    printf("starting main!\n");

    // split options from positional arguments
    std::vector<const char*> pos;
    int gpus = 1;
    bool quiet = false, gpuPost = false, timingJson = false, referencePng = false, overlapStart = true, fullTeardown = false;
    int streamedSave = ComputeApp::kStreamAuto;
    int pngThreads = 0;
    uint32_t colour = 0;   // --colour reference | equalised (MC_MANDEL_COLOUR_EQUALISED) | smooth (MC_MANDEL_COLOUR_SMOOTH) | distance (MC_MANDEL_COLOUR_DISTANCE) | smooth-equalised (MC_MANDEL_COLOUR_SMOOTH_EQUALISED)
    uint32_t supersample = 1;   // --supersample 1 | 2 | 4 | 8 (MC_MANDEL_SUPERSAMPLE)
    bool adaptive = false;      // --adaptive (MC_MANDEL_SUPERSAMPLE_ADAPTIVE): valid with --supersample 2 | 4 | 8 only
    bool adaptiveSmooth = false;      // --adaptive-smooth[=Q] (MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE): with --supersample 2 | 4 | 8 and --colour smooth | smooth-equalised
    uint32_t adaptiveSmoothQ = MC_MANDEL_ADAPTIVE_SMOOTH_THRESHOLD;   // Q: the threshold in units of 1/256 iteration
    bool supersampleSmooth = false;   // --supersample-smooth (MC_MANDEL_SUPERSAMPLE_SMOOTH): with --supersample 2 | 4 | 8 and --colour smooth | smooth-equalised
    enum : uint32_t { kOrbitHost = 0, kOrbitDevice = 1, kOrbitAuto = 2 };
    uint32_t orbitWhere = kOrbitHost;   // --orbit host | device | auto (mc_mandelbrot_orbit_create_device)
    bool orbitSet = false;              // given at all: the run prints its "orbit:" line
    uint32_t locate = 0;                // --locate[=N]: after the save, the N largest atom domains and their nuclei; 0: off
    unsigned long long exactCheck = 0, exactExtraLimbs = 0;   // --exact-check N [--exact-extra-limbs E]: N pixels iterated exactly after the render
    bool exactExtraSet = false;
    int zoomK = 0, zoomF = 0;           // --zoom K F: K octaves of F frames each (mc_mandelbrot_zoom_*)
    bool zoomSet = false;
    bool blaDevice = false, blaTableSet = false;       // --bla-table host | device: where the BLA precisions' table is built
    bool zoomOrbitShared = false, zoomOrbitSet = false;   // --zoom-orbit keyframe | shared: one orbit per keyframe, or the deepest one's for all
    uint32_t zoomFilter = MC_MANDEL_ZOOM_FILTER_BILINEAR;   // --zoom-filter bilinear | area: the area filter of the minified deep keyframe
    bool zoomFilterSet = false;
    bool zoomCounts = false;            // --zoom-keyframes colours | counts: count keyframes, one rank map per frame
    uint32_t denoise = 0;               // --denoise [P]: the path tracer's a-trous filter with P passes (mc_pathtrace_render_denoised); 0 = off
    float noiseGuided = 0.0f;           // --noise-guided [K]: with --denoise, the colour tolerance from a measured noise plane, k_noise = K
                                        // (mc_pathtrace_render_denoised_adaptive); 0 = off
    bool noiseGuidedSet = false;
    mc_pathtrace_budget_params budget;  // --budget [L] [--noise-target T]: per-pixel sample budgets (mc_pathtrace_render_budgeted), the pilot = spp
    mc_pathtrace_budget_default_params(&budget);
    bool budgetSet = false, noiseTargetSet = false;
    const char* outFile = nullptr;
    uint32_t width = 2000, height = 2000, maxIter = 128, precision = MC_PRECISION_F32, mathMode = MC_PT_MATH_STRICT;
    double cx = -0.445, cy = 0.0, sx = 2.34, sy = 2.34;
    const char* cxText = "-0.445";   // --precision perturb: the centre as decimal text, verbatim (mc_mandelbrot_orbit_create)
    const char* cyText = "0";
    const char* sxText = "2.34";     // --precision perturb: the scale as text too (strtold reaches about 1e-4951; atof stops at 1e-308)
    const char* syText = "2.34";
    bool viewSet = false, centreSet = false, scaleSet = false, largeSpheres = false;
    uint32_t spherePrec = MC_PT_PREC_F32;
    const char* sceneFile = nullptr;    // --scene FILE: the path tracer's tables from a text file, one `plane` or `sphere` and 12 floats per line
    uint32_t accel = 0;                 // --accel linear | bvh: the plain calls (every ray tests every object) or mc_pathtrace_render_accel*
    // --buddhabrot SAMPLES with --min-iter, --seed, --sample-window, --nebula, --tone, --white (mc_buddhabrot_*)
    unsigned long long buddhaSamples = 0, buddhaMinIter = 0, buddhaSeed = 1;
    bool buddhaSet = false, buddhaOptions = false, buddhaWindowSet = false, buddhaNebula = false, buddhaEqualised = false, maxIterSet = false;
    double buddhaWindow[4] = {-0.5, 0.0, 4.0, 4.0}, buddhaWhite = 99.9;
    unsigned long long buddhaNebulaIter[3] = {0, 0, 0};
    // --guided[=G] with --pilot, --dilate, --unbiased (mc_buddhabrot_render_guided)
    bool guidedSet = false, guidedOptions = false, pilotSet = false, dilateSet = false;
    unsigned long long guidedLog2 = 0, guidedPilot = 0, guidedDilate = 0, guidedUnbiased = 0;
    // a whole non-negative number up to `most`, or the run ends
    auto count = [](const std::string& opt, const char* v, unsigned long long most) -> unsigned long long {
        char* end = nullptr;
        const unsigned long long n = std::strtoull(v, &end, 10);
        if (!*v || std::strspn(v, "0123456789") != std::strlen(v) || n > most) {
            printf("%s %s: a whole number from 0 to %llu\n", opt.c_str(), v, most);
            exit(EXIT_FAILURE);
        }
        return n;
    };
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto need = [&](int n) { if (i + n >= argc) { printf("missing value for %s\n", a.c_str()); exit(EXIT_FAILURE); } };
        // one of a closed list of words -> its code; anything else ends the run (a typo must not render something else)
        auto choice = [&](const char* v, std::initializer_list<std::pair<const char*, uint32_t>> words) -> uint32_t {
            std::string all;
            for (const auto& w : words) { if (std::strcmp(v, w.first) == 0) return w.second; all += (all.empty() ? "" : " | ") + std::string(w.first); }
            printf("%s %s: not one of %s\n", a.c_str(), v, all.c_str());
            exit(EXIT_FAILURE);
        };
        if (a == "--gpus") { need(1); gpus = atoi(argv[++i]); }
        else if (a == "--out") { need(1); outFile = argv[++i]; }
        else if (a == "--quiet") quiet = true;
        else if (a == "--gpu-postprocess") gpuPost = true;     // float->u8 (+rotation) on the device, RGBA8-only download
        else if (a == "--png-threads") { need(1); pngThreads = atoi(argv[++i]); }   // 0 = all cores (default), 1 = serial
        else if (a == "--timing-json") timingJson = true;      // one JSON line: where the wall time of this run went (bench.py end_to_end)
        else if (a == "--fast-png")                             // (round-3 command lines: the stripe-parallel writer is the only one now)
            printf("note: --fast-png has no effect — the apps always write their own standard PNG (identical pixels; the reference "
                   "codec's exact file bytes come from a reference tree that calls this library, INTEGRATION.md route B)\n");
        else if (a == "--width") { need(1); width = (uint32_t)atoi(argv[++i]); }
        else if (a == "--height") { need(1); height = (uint32_t)atoi(argv[++i]); }
        else if (a == "--max-iter") { need(1); maxIter = (uint32_t)atoi(argv[++i]); maxIterSet = true; }
        else if (a == "--help") {
            printf("options: --gpus N, --out FILE, --quiet, --gpu-postprocess, --png-threads T, --timing-json, --width W, --height H, --max-iter M,\n"
                   "  --centre X Y, --scale SX SY, --precision f32|ds|f64|perturb|perturb-bla|perturb-bla-deep,\n"
                   "  --colour reference|equalised|smooth|distance|smooth-equalised, --supersample 1|2|4|8, --adaptive, --supersample-smooth, --adaptive-smooth[=Q],\n"
                   "  --exact-check N [--exact-extra-limbs E]  (the perturbation precisions) N sampled pixels iterated exactly on the device,\n"
                   "  --orbit host|device|auto, --zoom K F, --zoom-keyframes colours|counts, --zoom-filter bilinear|area,\n"
                   "  --locate[=N]  (--precision f32|f64|perturb) after the save: the N (default 8) largest atom domains of the view, each with its\n"
                   "      period, the nucleus Newton's method finds from its best pixel, and a ready --centre X Y,\n"
                   "  --math strict|fast|careful, --denoise [P], --noise-guided [K], --budget [L], --noise-target T, --scene FILE, --accel linear|bvh,\n"
                   "  --buddhabrot SAMPLES  the orbit-density plane of SAMPLES pseudo-random c (the Mandelbrot app); --centre / --scale default to\n"
                   "      the view -0.5 0 / 3 3H/W and --max-iter to 1000; with it:\n"
                   "    --min-iter m            only orbits that escape after at least m iterations are plotted (default 0)\n"
                   "    --seed s                the sample sequence (default 1)\n"
                   "    --sample-window CX CY SX SY   the window c is drawn from (default -0.5 0 4 4)\n"
                   "    --nebula MR MG MB       three renders of those max_iter, one per colour channel\n"
                   "    --tone sqrt|equalised   the map from density to brightness (default sqrt)\n"
                   "    --white PCT             the white level: the density not exceeded by PCT %% of the non-empty bins, read from one\n"
                   "                            histogram capped at 2^20 - 1 (default 99.9)\n"
                   "    --guided[=G]            for zoomed views: a pilot finds the cells of the 2^G x 2^G grid over the sample window (G in\n"
                   "                            1 .. 12, default 8) whose orbits reach the view; the SAMPLES are drawn from those cells only\n"
                   "      --pilot P             the pilot's uniform samples (default 2^24)\n"
                   "      --dilate D            rings of neighbouring cells added to the list, 0 .. 8 (default 1)\n"
                   "      --unbiased B          a second pass over all the other cells with 1 / B of the samples per cell at weight B\n");
            return EXIT_SUCCESS;
        }
        else if (a == "--buddhabrot") { need(1); buddhaSamples = count(a, argv[++i], 1ull << 40); buddhaSet = true; }
        else if (a == "--min-iter") { need(1); buddhaMinIter = count(a, argv[++i], 0xffffffffull); buddhaOptions = true; }
        else if (a == "--seed") { need(1); buddhaSeed = count(a, argv[++i], 0xffffffffull); buddhaOptions = true; }
        else if (a == "--sample-window") { need(4); for (double& w : buddhaWindow) w = atof(argv[++i]); buddhaWindowSet = buddhaOptions = true; }
        else if (a == "--nebula") { need(3); for (unsigned long long& n : buddhaNebulaIter) n = count(a, argv[++i], 1ull << 24); buddhaNebula = buddhaOptions = true; }
        else if (a == "--tone") { need(1); buddhaEqualised = choice(argv[++i], {{"sqrt", 0u}, {"equalised", 1u}}) != 0u; buddhaOptions = true; }
        else if (a == "--white") {
            need(1);
            const char* v = argv[++i];
            char* end = nullptr;
            buddhaWhite = std::strtod(v, &end);
            if (end == v || *end || !(buddhaWhite > 0.0) || !(buddhaWhite <= 100.0)) { printf("--white %s: a percentage above 0, at most 100\n", v); exit(EXIT_FAILURE); }
            buddhaOptions = true;
        }
        else if (a == "--guided") guidedSet = true;
        else if (a.rfind("--guided=", 0) == 0) {
            guidedLog2 = count("--guided=", a.c_str() + 9, 12);
            if (!guidedLog2) { printf("%s: G is 1 to 12\n", a.c_str()); exit(EXIT_FAILURE); }
            guidedSet = true;
        }
        else if (a == "--pilot") { need(1); guidedPilot = count(a, argv[++i], 1ull << 40); pilotSet = guidedOptions = true; }
        else if (a == "--dilate") { need(1); guidedDilate = count(a, argv[++i], 8); dilateSet = guidedOptions = true; }
        else if (a == "--unbiased") { need(1); guidedUnbiased = count(a, argv[++i], 0xffffffffull); guidedOptions = true; }
        else if (a == "--centre") { need(2); cxText = argv[++i]; cyText = argv[++i]; cx = atof(cxText); cy = atof(cyText); viewSet = centreSet = true; }
        else if (a == "--scale") { need(2); sxText = argv[++i]; syText = argv[++i]; sx = atof(sxText); sy = atof(syText); viewSet = scaleSet = true; }
        else if (a == "--precision") { need(1); precision = choice(argv[++i], {{"f32", MC_PRECISION_F32}, {"ds", MC_PRECISION_DS}, {"f64", MC_PRECISION_F64}, {"perturb", MC_PRECISION_PERTURB}, {"perturb-bla", MC_PRECISION_PERTURB_BLA}, {"perturb-bla-deep", MC_PRECISION_PERTURB_BLA_DEEP}}); }
        else if (a == "--colour") {   // reference: t = n / M (mandelbrot.comp:50-56) | equalised: the count's rank among the image's escaped pixels
                                      // | smooth: the fractional escape count, interpolated between neighbouring palette entries
            need(1);
            colour = choice(argv[++i], {{"reference", 0u}, {"equalised", (uint32_t)MC_MANDEL_COLOUR_EQUALISED},
                                        {"smooth", (uint32_t)MC_MANDEL_COLOUR_SMOOTH}, {"distance", (uint32_t)MC_MANDEL_COLOUR_DISTANCE},
                                        {"smooth-equalised", (uint32_t)MC_MANDEL_COLOUR_SMOOTH_EQUALISED}});
#if !defined(MANDELBROT_MODE)
            printf("--colour: a Mandelbrot option\n");
            exit(EXIT_FAILURE);
#endif
        }
        else if (a == "--supersample") {   // S x S samples per pixel, box-filtered on the device (1: off)
            need(1);
            supersample = choice(argv[++i], {{"1", 1u}, {"2", 2u}, {"4", 4u}, {"8", 8u}});
#if !defined(MANDELBROT_MODE)
            printf("--supersample: a Mandelbrot option\n");
            exit(EXIT_FAILURE);
#endif
        }
        else if (a == "--adaptive") {   // supersample only the pixels whose count differs from a neighbour's
            adaptive = true;
#if !defined(MANDELBROT_MODE)
            printf("--adaptive: a Mandelbrot option\n");
            exit(EXIT_FAILURE);
#endif
        }
        else if (a == "--adaptive-smooth" || a.rfind("--adaptive-smooth=", 0) == 0) {   // smooth samples only where the smooth count moves by more than Q
            adaptiveSmooth = true;
#if !defined(MANDELBROT_MODE)
            printf("--adaptive-smooth: a Mandelbrot option\n");
            exit(EXIT_FAILURE);
#endif
            if (a.size() > 17) {
                const std::string v = a.substr(18);
                char* end = nullptr;
                errno = 0;
                const unsigned long long q = strtoull(v.c_str(), &end, 10);
                if (v.empty() || v[0] < '0' || v[0] > '9' || *end || errno || q > 0xffffffffull) {
                    printf("--adaptive-smooth=Q: Q is a decimal number of 1/256 iterations, 0 .. 4294967295; got '%s'\n", v.c_str());
                    exit(EXIT_FAILURE);
                }
                adaptiveSmoothQ = (uint32_t)q;
            }
        }
        else if (a == "--supersample-smooth") {   // the samples are smooth counts: the resolve over fractional counts
            supersampleSmooth = true;
#if !defined(MANDELBROT_MODE)
            printf("--supersample-smooth: a Mandelbrot option\n");
            exit(EXIT_FAILURE);
#endif
        }
        else if (a == "--orbit") {   // where the perturbation precisions compute their reference orbit
            need(1);
            orbitWhere = choice(argv[++i], {{"host", (uint32_t)kOrbitHost}, {"device", (uint32_t)kOrbitDevice}, {"auto", (uint32_t)kOrbitAuto}});
            orbitSet = true;
#if !defined(MANDELBROT_MODE)
            printf("--orbit: a Mandelbrot option\n");
            exit(EXIT_FAILURE);
#endif
        }
        else if (a == "--exact-check") { need(1); exactCheck = count(a, argv[++i], 1ull << 20); }   // 0: off
        else if (a == "--exact-extra-limbs") { need(1); exactExtraLimbs = count(a, argv[++i], 128); exactExtraSet = true; }
        else if (a == "--zoom") {   // a zoom sequence: K + 1 keyframes, K * F + 1 frames composed from them
            need(2);
            zoomK = atoi(argv[++i]);
            zoomF = atoi(argv[++i]);
            zoomSet = true;
#if !defined(MANDELBROT_MODE)
            printf("--zoom: a Mandelbrot option\n");
            exit(EXIT_FAILURE);
#endif
        }
        else if (a == "--zoom-keyframes") {   // what --zoom keeps of a keyframe: its colours (mc_mandelbrot_zoom_*) or its counts (mc_mandelbrot_zoom_counts_*)
            need(1);
            zoomCounts = choice(argv[++i], {{"colours", 0u}, {"counts", 1u}}) != 0u;
#if !defined(MANDELBROT_MODE)
            printf("--zoom-keyframes: a Mandelbrot option\n");
            exit(EXIT_FAILURE);
#endif
        }
        else if (a == "--bla-table") {   // where perturb-bla / perturb-bla-deep build their table: on the host, or on the device at the bind
            need(1);
            blaDevice = choice(argv[++i], {{"host", 0u}, {"device", 1u}}) != 0u;
            blaTableSet = true;
#if !defined(MANDELBROT_MODE)
            printf("--bla-table: a Mandelbrot option\n");
            exit(EXIT_FAILURE);
#endif
        }
        else if (a == "--zoom-orbit") {   // --zoom with a perturbation precision: an orbit per keyframe, or the deepest keyframe's rescaled for each
            need(1);
            zoomOrbitShared = choice(argv[++i], {{"keyframe", 0u}, {"shared", 1u}}) != 0u;
            zoomOrbitSet = true;
#if !defined(MANDELBROT_MODE)
            printf("--zoom-orbit: a Mandelbrot option\n");
            exit(EXIT_FAILURE);
#endif
        }
        else if (a == "--zoom-filter") {   // how --zoom's frames read the minified deep keyframe: one bilinear tap, or a box over the pixel's footprint
            need(1);
            zoomFilter = choice(argv[++i], {{"bilinear", (uint32_t)MC_MANDEL_ZOOM_FILTER_BILINEAR}, {"area", (uint32_t)MC_MANDEL_ZOOM_FILTER_AREA}});
            zoomFilterSet = true;
#if !defined(MANDELBROT_MODE)
            printf("--zoom-filter: a Mandelbrot option\n");
            exit(EXIT_FAILURE);
#endif
        }
        else if (a == "--locate" || a.rfind("--locate=", 0) == 0) {   // N is optional, as --denoise's P is (default 8)
            const char* v = nullptr;
            if (a.size() > 8) v = argv[i] + 9;
            else if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') v = argv[++i];
            const int n = v ? atoi(v) : 8;
            if (n < 1 || n > 64 || (v && (!*v || std::strspn(v, "0123456789") != std::strlen(v)))) {
                printf("--locate %s: the number of domains is 1 .. 64\n", v ? v : "");
                exit(EXIT_FAILURE);
            }
            locate = (uint32_t)n;
#if !defined(MANDELBROT_MODE)
            printf("--locate: a Mandelbrot option\n");
            exit(EXIT_FAILURE);
#endif
        }
        else if (a == "--denoise" || a.rfind("--denoise=", 0) == 0) {   // render + guide planes + a-trous filter on the device
            // P is optional (default 5): `--denoise=P`, or `--denoise P` where the next argument is a number (so the positional spp and
            // resy go in front of a bare --denoise)
            const char* v = nullptr;
            if (a.size() > 9) v = argv[i] + 10;
            else if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') v = argv[++i];
            const int passes = v ? atoi(v) : 5;
            if (passes < 1 || passes > 8 || (v && std::strspn(v, "0123456789") != std::strlen(v))) {
                printf("--denoise %s: the pass count is 1 .. 8\n", v ? v : "");
                exit(EXIT_FAILURE);
            }
            denoise = (uint32_t)passes;
#if !defined(PATHTRACER_MODE)
            printf("--denoise: a path tracer option\n");
            exit(EXIT_FAILURE);
#endif
        }
        else if (a == "--noise-guided" || a.rfind("--noise-guided=", 0) == 0) {   // K is optional, as --denoise's P is (default: the library's)
            const char* v = nullptr;
            if (a.size() > 14) v = argv[i] + 15;
            else if (i + 1 < argc && ((argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') || argv[i + 1][0] == '.')) v = argv[++i];
            uint32_t radius = 0;
            mc_pathtrace_noise_default_params(&noiseGuided, &radius);
            char* end = nullptr;
            if (v) noiseGuided = std::strtof(v, &end);
            if (v && (end == v || *end || !(noiseGuided > 0.0f) || !(noiseGuided * noiseGuided < 3e38f))) {
                printf("--noise-guided %s: k_noise is a number above 0 with a finite square\n", v);
                exit(EXIT_FAILURE);
            }
            noiseGuidedSet = true;
#if !defined(PATHTRACER_MODE)
            printf("--noise-guided: a path tracer option\n");
            exit(EXIT_FAILURE);
#endif
        }
        else if (a == "--budget" || a.rfind("--budget=", 0) == 0) {   // L is optional, as --denoise's P is (default: the library's)
            const char* v = nullptr;
            if (a.size() > 8) v = argv[i] + 9;
            else if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') v = argv[++i];
            const int level = v ? atoi(v) : (int)budget.max_level;
            if (level < 0 || level > 8 || (v && (!*v || std::strspn(v, "0123456789") != std::strlen(v)))) {
                printf("--budget %s: the deepest level is 0 .. 8 (a pixel gets at most spp << level samples)\n", v ? v : "");
                exit(EXIT_FAILURE);
            }
            budget.max_level = (uint32_t)level;
            budgetSet = true;
#if !defined(PATHTRACER_MODE)
            printf("--budget: a path tracer option\n");
            exit(EXIT_FAILURE);
#endif
        }
        else if (a == "--noise-target") {   // with --budget: the noise a pixel may keep, in units of the encoded buffer
            need(1);
            const char* v = argv[++i];
            char* end = nullptr;
            budget.target = std::strtof(v, &end);
            if (end == v || *end || !(budget.target > 0.0f) || !(budget.target * budget.target < 3e38f)) {
                printf("--noise-target %s: a number above 0 with a finite square\n", v);
                exit(EXIT_FAILURE);
            }
            noiseTargetSet = true;
#if !defined(PATHTRACER_MODE)
            printf("--noise-target: a path tracer option\n");
            exit(EXIT_FAILURE);
#endif
        }
        else if (a == "--math") {   // strict (the default: bit-identical to the oracle) | fast | careful (mc_compute.h MC_PT_MATH_*)
            need(1);
            mathMode = choice(argv[++i], {{"strict", MC_PT_MATH_STRICT}, {"fast", MC_PT_MATH_FAST}, {"careful", MC_PT_MATH_FAST_CAREFUL}});
        }
        else if (a == "--reference-png") referencePng = true;       // the reference's lodepng::encode (make REFERENCE=<checkout>)
        else if (a == "--no-streamed-save") streamedSave = ComputeApp::kStreamOff;   // render everything, then encode (see setStreamedSave)
        else if (a == "--streamed-save") streamedSave = ComputeApp::kStreamOn;       // ... stream whatever the size (default: where it pays)
        else if (a == "--full-teardown") fullTeardown = true;        // run the destructors and the HIP runtime's exit handlers (see the end of main)
        else if (a == "--serial-start") overlapStart = false;        // measurements: the round-5 start-up order (no warm-up thread)
        else if (a == "--large-sphere-walls") largeSpheres = true;   // TEST_PRECISION_WITH_LARGE_SPHERE_WALLS (pathtracerApp.h:11)
        else if (a == "--sphere-precision") {                        // which #if branch of pathTracer.comp:132-256 is active
            need(1);
            spherePrec = choice(argv[++i], {{"f32", MC_PT_PREC_F32}, {"fp64", MC_PT_PREC_FP64}, {"ds", MC_PT_PREC_DS}, {"df64", MC_PT_PREC_DF64}});
        }
        else if (a == "--scene") { need(1); sceneFile = argv[++i]; }
        else if (a == "--accel") { need(1); accel = choice(argv[++i], {{"linear", 0u}, {"bvh", 1u}}); }
        else if (a.size() > 2 && a[0] == '-' && a[1] == '-') { printf("unknown option %s\n", a.c_str()); exit(EXIT_FAILURE); }
        else pos.push_back(argv[i]);
    }
    if (buddhaOptions && !buddhaSet) { printf("--min-iter / --seed / --sample-window / --nebula / --tone / --white: only with --buddhabrot SAMPLES\n"); exit(EXIT_FAILURE); }
    if ((guidedSet || guidedOptions) && !buddhaSet) { printf("--guided / --pilot / --dilate / --unbiased: only with --buddhabrot SAMPLES\n"); exit(EXIT_FAILURE); }
    if (guidedOptions && !guidedSet) { printf("--pilot / --dilate / --unbiased: only with --guided\n"); exit(EXIT_FAILURE); }
    if (buddhaSet) {
        const char* why = !buddhaSamples                    ? "SAMPLES is at least 1"
                          : maxIterSet && !maxIter          ? "--max-iter is at least 1"
                          : gpus > 1                        ? "one GPU (sample ranges compose: add the planes of several processes)"
                          : colour                          ? "not with --colour (the density has its own tone maps: --tone)"
                          : supersample > 1u || adaptive    ? "not with --supersample / --adaptive"
                          : zoomSet                         ? "not with --zoom"
                          : precision != MC_PRECISION_F32   ? "not with --precision (the orbits are iterated in fp64)"
                          : orbitSet                        ? "not with --orbit"
                                                            : nullptr;
        if (why) { printf("--buddhabrot: %s\n", why); exit(EXIT_FAILURE); }
    }
#if !defined(MANDELBROT_MODE)
    if (buddhaSet) { printf("--buddhabrot: a Mandelbrot option\n"); exit(EXIT_FAILURE); }
#endif
    (void)maxIterSet; (void)centreSet; (void)scaleSet; (void)buddhaMinIter; (void)buddhaSeed; (void)buddhaWindowSet; (void)buddhaNebula; (void)buddhaEqualised; (void)buddhaWindow; (void)buddhaWhite; (void)buddhaNebulaIter;
    (void)guidedSet; (void)pilotSet; (void)dilateSet; (void)guidedLog2; (void)guidedPilot; (void)guidedDilate; (void)guidedUnbiased;
    if (adaptiveSmooth) {   // (before the two options it does not combine with word their own refusals)
        const char* why = adaptive            ? "not with --adaptive (that option compares integer counts; this one is given without it)"
                          : supersampleSmooth ? "not with --supersample-smooth (that option is the full resolve; this one is given without it)"
                          : supersample <= 1u ? "needs --supersample 2 | 4 | 8"
                          : colour != MC_MANDEL_COLOUR_SMOOTH && colour != MC_MANDEL_COLOUR_SMOOTH_EQUALISED ? "needs --colour smooth | smooth-equalised"
                          : gpus > 1          ? "one GPU (a device's tile cannot see its neighbours' counts)"
                          : buddhaSet         ? "not with --buddhabrot"
                          : zoomCounts        ? "not with --zoom-keyframes counts (a supersampled pixel has no single count; use --zoom-keyframes colours)"
                          : zoomSet && adaptiveSmoothQ != MC_MANDEL_ADAPTIVE_SMOOTH_THRESHOLD ? "with --zoom the threshold is the default 256 (keyframes render through mc_mandelbrot_zoom_push)"
                                              : nullptr;
        if (why) { printf("--adaptive-smooth: %s\n", why); exit(EXIT_FAILURE); }
    }
    if (adaptive && supersample <= 1u) { printf("--adaptive: needs --supersample 2 | 4 | 8\n"); exit(EXIT_FAILURE); }
    if (supersampleSmooth) {
        const char* why = supersample <= 1u ? "needs --supersample 2 | 4 | 8"
                          : colour != MC_MANDEL_COLOUR_SMOOTH && colour != MC_MANDEL_COLOUR_SMOOTH_EQUALISED ? "needs --colour smooth | smooth-equalised"
                          : adaptive ? "not with --adaptive (adaptive refinement compares integer counts)"
                          : gpus > 1 ? "one GPU (the resolve runs on the device that holds the samples)"
                                     : nullptr;
        if (why) { printf("--supersample-smooth: %s\n", why); exit(EXIT_FAILURE); }
    }
    if (zoomSet && (zoomK < 1 || zoomF < 1)) {
        printf("usage: --zoom K F: K octaves (keyframes K + 1, the given view the deepest) of F frames each, both at least 1; got %d %d\n", zoomK, zoomF);
        exit(EXIT_FAILURE);
    }
    if (zoomSet && gpus > 1) { printf("--zoom: one GPU (the keyframes stay on the context's device)\n"); exit(EXIT_FAILURE); }
    if (zoomFilterSet && !zoomSet) { printf("--zoom-filter: needs --zoom K F (it chooses how a zoom sequence's frames read the deep keyframe)\n"); exit(EXIT_FAILURE); }
    {
        const bool orbitView = precision == MC_PRECISION_PERTURB || precision == MC_PRECISION_PERTURB_BLA || precision == MC_PRECISION_PERTURB_BLA_DEEP;
        if (zoomOrbitSet && !(zoomSet && orbitView)) {
            printf("--zoom-orbit: needs --zoom K F and --precision perturb | perturb-bla | perturb-bla-deep (it chooses how a dive's keyframes get their reference orbit)\n");
            exit(EXIT_FAILURE);
        }
        if (blaTableSet && !(precision == MC_PRECISION_PERTURB_BLA || precision == MC_PRECISION_PERTURB_BLA_DEEP)) {
            printf("--bla-table: needs --precision perturb-bla | perturb-bla-deep (it chooses where their table is built)\n");
            exit(EXIT_FAILURE);
        }
        if (exactCheck || exactExtraSet) {
            const char* why = !exactCheck   ? "--exact-extra-limbs: needs --exact-check N"
                              : !orbitView  ? "--exact-check: needs --precision perturb | perturb-bla | perturb-bla-deep (the check iterates c_ref + the pixel's offset)"
                              : zoomSet     ? "--exact-check: not with --zoom (it checks one still)"
                              : gpus > 1    ? "--exact-check: one GPU"
                                            : nullptr;
            if (why) { printf("%s\n", why); exit(EXIT_FAILURE); }
        }
        if (locate) {
            const char* why = !(precision == MC_PRECISION_F32 || precision == MC_PRECISION_F64 || precision == MC_PRECISION_PERTURB)
                                  ? "--locate: needs --precision f32 | f64 | perturb (the period plane is built for those: mc_mandelbrot_render_atom)"
                              : zoomSet       ? "--locate: not with --zoom (it reads one still)"
                              : buddhaSet     ? "--locate: not with --buddhabrot"
                              : gpus > 1      ? "--locate: one GPU"
                                              : nullptr;
            if (why) { printf("%s\n", why); exit(EXIT_FAILURE); }
        }
        if (blaDevice && gpus > 1) { printf("--bla-table device: one GPU (the table is built into the context's binding)\n"); exit(EXIT_FAILURE); }
    }
    if (zoomCounts) {   // count keyframes carry one count per pixel: the colourings and resolves that need more stay with --zoom-keyframes colours
        const char* why = !zoomSet                                ? "needs --zoom K F (it chooses what a zoom sequence keeps of a keyframe)"
                          : colour == MC_MANDEL_COLOUR_DISTANCE   ? "not with --colour distance (a stencil over a whole smooth plane; use --zoom-keyframes colours)"
                          : adaptive                              ? "not with --adaptive (a supersampled pixel has no single count; use --zoom-keyframes colours)"
                          : supersample > 1u                      ? "not with --supersample above 1 (a supersampled pixel has no single count; use --zoom-keyframes colours)"
                                                                  : nullptr;
        if (why) { printf("--zoom-keyframes counts: %s\n", why); exit(EXIT_FAILURE); }
    }
    if (noiseGuidedSet && gpus > 1) { printf("--noise-guided: one GPU (the chain has no multi-GPU form)\n"); exit(EXIT_FAILURE); }
    if (denoise && gpus > 1) { printf("--denoise: one GPU (the filter reads across the rows of the whole image)\n"); exit(EXIT_FAILURE); }
    if (noiseGuidedSet && !denoise) { printf("--noise-guided: only with --denoise (it steers that filter's colour tolerance)\n"); exit(EXIT_FAILURE); }
    if (noiseTargetSet && !budgetSet) { printf("--noise-target: only with --budget (it is the noise a budgeted pixel may keep)\n"); exit(EXIT_FAILURE); }
    if (budgetSet && denoise) {
        printf("--budget: not with --denoise (a budgeted-then-filtered chain is not offered: the noise-guided filter needs a half / full pair per pixel)\n");
        exit(EXIT_FAILURE);
    }
    if (budgetSet && gpus > 1) { printf("--budget: one GPU (the chain has no multi-GPU form)\n"); exit(EXIT_FAILURE); }
    if (budgetSet && spherePrec != MC_PT_PREC_F32) { printf("--budget: the fp32 sphere test only (--sphere-precision f32)\n"); exit(EXIT_FAILURE); }
    if (accel && gpus > 1) { printf("--accel bvh: one GPU (the accelerated calls have no multi-GPU form)\n"); exit(EXIT_FAILURE); }
    if (accel && denoise && !noiseGuidedSet) {
        printf("--accel bvh --denoise: only with --noise-guided (the app runs the accelerated noise-guided chain; the fixed-tolerance one, "
               "mc_pathtrace_render_accel_denoised, is a library call)\n");
        exit(EXIT_FAILURE);
    }
    if (accel && spherePrec != MC_PT_PREC_F32) { printf("--accel bvh: the fp32 sphere test only (--sphere-precision f32)\n"); exit(EXIT_FAILURE); }
#if !defined(PATHTRACER_MODE)
    if (sceneFile || accel) { printf("--scene / --accel: path tracer options\n"); exit(EXIT_FAILURE); }
#endif
    (void)budgetSet; (void)noiseTargetSet; (void)zoomSet; (void)zoomCounts; (void)zoomFilter; (void)zoomFilterSet; (void)denoise; (void)noiseGuided; (void)noiseGuidedSet; (void)sceneFile; (void)accel;
    (void)exactCheck; (void)exactExtraLimbs; (void)exactExtraSet; (void)locate;
    (void)orbitWhere; (void)orbitSet; (void)blaDevice; (void)blaTableSet; (void)zoomOrbitShared; (void)zoomOrbitSet; (void)colour; (void)supersample; (void)supersampleSmooth; (void)adaptiveSmooth; (void)adaptiveSmoothQ; (void)width; (void)height; (void)maxIter; (void)precision; (void)mathMode; (void)cx; (void)cy; (void)sx; (void)sy; (void)viewSet; (void)largeSpheres; (void)spherePrec; (void)cxText; (void)cyText; (void)sxText; (void)syText; (void)sxText; (void)syText;

#if defined(MANDELBROT_MODE)
    MandelbrotApp app = MandelbrotApp(width, height);   // reference: 2000 x 2000 (main.cpp:20)
    app.setMaxIter(maxIter);
    if (viewSet) app.setView(cx, cy, sx, sy);
    app.setPrecision(precision);
    app.setZoomCounts(zoomCounts);
    app.setZoomFilter(zoomFilter);
    if (buddhaSet) {   // one blocking render per channel, then the tone map: never the banded, streamed save
        MandelbrotApp::Buddhabrot b;
        b.samples = buddhaSamples;
        b.maxIter = maxIterSet ? maxIter : 0u;
        b.minIter = (uint32_t)buddhaMinIter;
        b.seed = (uint32_t)buddhaSeed;
        b.viewSet = viewSet;   // --centre or --scale alone: the other half is the library's default view, not the set's
        b.view[0] = centreSet ? cx : -0.5; b.view[1] = centreSet ? cy : 0.0;
        b.view[2] = scaleSet ? sx : 3.0; b.view[3] = scaleSet ? sy : (3.0 * (double)height) / (double)width;
        b.windowSet = buddhaWindowSet;
        for (int k = 0; k < 4; k++) b.window[k] = buddhaWindow[k];
        b.nebula = buddhaNebula;
        for (int k = 0; k < 3; k++) b.nebulaIter[k] = (uint32_t)buddhaNebulaIter[k];
        b.equalised = buddhaEqualised;
        b.whitePct = buddhaWhite;
        b.guided = guidedSet;
        b.guideLog2 = (uint32_t)guidedLog2;
        b.pilotSet = pilotSet; b.pilot = guidedPilot;
        b.dilateSet = dilateSet; b.dilate = (uint32_t)guidedDilate;
        b.unbiased = (uint32_t)guidedUnbiased;
        app.setBuddhabrot(b);
        if (streamedSave == ComputeApp::kStreamOn) printf("note: --buddhabrot renders whole planes; --streamed-save has no effect\n");
        streamedSave = ComputeApp::kStreamOff;
    }
    if (colour == MC_MANDEL_COLOUR_SMOOTH) {   // a per-pixel function: the normal banded, streamed save
        if (supersample > 1u && !supersampleSmooth && !adaptiveSmooth) {
            printf("--colour smooth: does not combine with --supersample yet (a resolve over fractional counts) unless --supersample-smooth asks for it\n");
            return EXIT_FAILURE;
        }
        app.setColourFlags(colour);
    } else if (colour == MC_MANDEL_COLOUR_DISTANCE) {   // a stencil over the whole image's smooth plane: the whole-image calls, as equalised
        if (supersample > 1u) { printf("--colour distance: does not combine with --supersample (a resolve over fractional counts)\n"); return EXIT_FAILURE; }
        app.setColourFlags(colour);
        if (streamedSave == ComputeApp::kStreamOn) printf("note: --colour distance renders the whole image in one call; --streamed-save has no effect\n");
        streamedSave = ComputeApp::kStreamOff;
    } else if (colour == MC_MANDEL_COLOUR_SMOOTH_EQUALISED) {   // the rank over the whole image's smooth plane: the whole-image calls, as equalised
        if (supersample > 1u && !supersampleSmooth && !adaptiveSmooth) {
            printf("--colour smooth-equalised: does not combine with --supersample (a resolve over fractional counts) unless --supersample-smooth asks for it\n");
            return EXIT_FAILURE;
        }
        app.setColourFlags(colour);
        if (streamedSave == ComputeApp::kStreamOn) printf("note: --colour smooth-equalised renders the whole image in one call; --streamed-save has no effect\n");
        streamedSave = ComputeApp::kStreamOff;
    } else if (colour) {   // the histogram needs the whole image: one mc_mandelbrot_render(_rgba8), never the banded, streamed save
        app.setColourFlags(colour);
        if (streamedSave == ComputeApp::kStreamOn) printf("note: --colour equalised renders the whole image in one call; --streamed-save has no effect\n");
        streamedSave = ComputeApp::kStreamOff;
    }
    if (supersample > 1u) {   // the sample plane is resolved by the whole-image calls: never the banded, streamed save
        app.setSupersample(supersample);
        if (adaptive) app.setColourFlags(MC_MANDEL_SUPERSAMPLE_ADAPTIVE);   // (whole-image calls as well: the save is never streamed)
        if (supersampleSmooth) app.setColourFlags(MC_MANDEL_SUPERSAMPLE_SMOOTH);
        if (adaptiveSmooth) {
            app.setColourFlags(MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE);
            app.setAdaptiveSmoothThreshold(adaptiveSmoothQ);
        }
        if (streamedSave == ComputeApp::kStreamOn) printf("note: --supersample renders the whole image in one call; --streamed-save has no effect\n");
        streamedSave = ComputeApp::kStreamOff;
    }
    if (zoomSet) {   // every frame is composed from keyframes rendered whole: never the banded, streamed save
        if (streamedSave == ComputeApp::kStreamOn) printf("note: --zoom composes every frame from whole keyframes; --streamed-save has no effect\n");
        streamedSave = ComputeApp::kStreamOff;
        // (without --centre / --scale the still's view is the default params' float words: the same doubles here)
        if (!viewSet) { cx = (double)-0.445f; cy = 0.0; sx = sy = (double)2.34f; }
        // the widest keyframe's scale must be one a view can hold: the view words are floats (the perturbation precisions carry their
        // scale in the orbit, whose constructor answers for it)
        const bool orbitView = precision == MC_PRECISION_PERTURB || precision == MC_PRECISION_PERTURB_BLA || precision == MC_PRECISION_PERTURB_BLA_DEEP;
        if (!orbitView && !(std::fabs(std::ldexp(sx, zoomK)) <= 3.0e38 && std::fabs(std::ldexp(sy, zoomK)) <= 3.0e38)) {
            printf("--zoom %d %d: the first keyframe's scale, --scale x 2^%d, is beyond what a view holds (3e38)\n", zoomK, zoomF, zoomK);
            return EXIT_FAILURE;
        }
        app.setZoom((uint32_t)zoomK, (uint32_t)zoomF, cx, cy, sx, sy, nullptr);
    }
    if (precision == MC_PRECISION_PERTURB || precision == MC_PRECISION_PERTURB_BLA ||
        precision == MC_PRECISION_PERTURB_BLA_DEEP) {                                    // the reference orbit, on the host: a malformed
                                                                                         // centre ends the run before a device is touched
        // a scale below 2^-960 takes the deep constructor: (mantissa, exponent) from long double text, common exponent of the smaller
        char* endx = nullptr;
        char* endy = nullptr;
        const long double lx = strtold(sxText, &endx), ly = strtold(syText, &endy);
        if (endx == sxText || *endx || endy == syText || *endy) {
            printf("--scale %s %s: not two decimal numbers\n", sxText, syText);
            return EXIT_FAILURE;
        }
        const long double lmin = fabsl(lx) < fabsl(ly) ? fabsl(lx) : fabsl(ly);
        if (precision == MC_PRECISION_PERTURB_BLA && lmin != 0.0L && lmin < ldexpl(1.0L, -960)) {
            printf("--precision perturb-bla --scale %s %s: below 2^-960 (a deep orbit renders by the rescaled loop, which has no BLA; "
                   "use --precision perturb or perturb-bla-deep)\n", sxText, syText);
            return EXIT_FAILURE;
        }
        const bool deepScale = lmin != 0.0L && lmin < ldexpl(1.0L, -960);
        int e = 0;
        (void)frexpl(lmin, &e);
        // --orbit auto: the device from kOrbitAutoLimbs limbs upward (the orbit's k + 1, from the constructors' bits = 1 - e + 96, at least
        // 64), the host below.  130: the smallest measured limb count from which the device's whole call is at least 20 % below the host's
        // (profiles/orbit_device_probe.txt: 0.78 of the host's time there, 1.04 at 106 limbs).
        constexpr long kOrbitAutoLimbs = 130;
        const long bits = 1L - e + 96 < 64 ? 64 : 1L - e + 96;
        const bool onDevice = gpus <= 1 && (orbitWhere == kOrbitDevice ||
                                            (orbitWhere == kOrbitAuto && kOrbitAutoLimbs > 0 && lmin != 0.0L && (bits + 63) / 64 + 1 >= kOrbitAutoLimbs));
        // the orbit and its tables on ctx's device (or the host: ctx == nullptr); the message the run ends with, or "" after setOrbit()
        // shift: --zoom's keyframes, the scale's exponent raised by that much (0: the view itself)
        auto message = [](const char* fmt, auto... args) {
            char buf[8192];
            snprintf(buf, sizeof buf, fmt, args...);
            return std::string(buf);
        };
        // (mantissa, exponent): exact at any depth and under any shift.  EVERY keyframe of a zoom takes this form, the last one
        // (shift 0) too: mc_mandelbrot_zoom_push compares successive scales exactly, and the plain constructor's strtod of the text
        // need not be the double this mantissa gives
        const bool expForm = deepScale || zoomSet;
        const double mantX = (double)ldexpl(lx, -e), mantY = (double)ldexpl(ly, -e);
        // the orbit on ctx's device (or the host: ctx == nullptr): the message the run ends with, or "" and the object
        auto createOrbit = [=](mc_context* ctx, int shift, mc_mandelbrot_orbit** made) -> std::string {
            const auto t0 = std::chrono::steady_clock::now();
            int rc;
            if (ctx) {
                if (expForm) rc = mc_mandelbrot_orbit_create_device(ctx, cxText, cyText, mantX, mantY, e + shift, maxIter, made);
                else rc = mc_mandelbrot_orbit_create_device(ctx, cxText, cyText, sx, sy, 0, maxIter, made);
            } else if (expForm) {
                rc = mc_mandelbrot_orbit_create_deep(cxText, cyText, mantX, mantY, e + shift, maxIter, made);
            } else {
                rc = mc_mandelbrot_orbit_create(cxText, cyText, sx, sy, maxIter, made);
            }
            const double orbitMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (rc != MC_OK)
                return message("--centre %s %s / --scale %s %s: %s (%s)", cxText, cyText, sxText, syText, mc_error_string(rc), mc_last_error_detail());
            if (orbitSet || zoomOrbitShared) {
                uint32_t obits = 0, launches = 0;
                mc_mandelbrot_orbit_info(*made, nullptr, nullptr, &obits);
                if (ctx) mc_context_last_orbit_timing(ctx, nullptr, &launches, nullptr);
                if (zoomOrbitShared)   // the dive's one orbit: its limb count is what every keyframe's table is read with
                    printf("orbit: %.3f ms (%s, %u bits, %u fractional limbs, %u launches), shared by %d keyframes\n", orbitMs,
                           ctx ? "device" : "host", obits, (obits + 63u) / 64u, launches, zoomK + 1);
                else printf("orbit: %.3f ms (%s, %u bits, %u launches)\n", orbitMs, ctx ? "device" : "host", obits, launches);
            }
            return std::string();
        };
        // the orbit's table (on the host, unless --bla-table device leaves it to the bind), then the app owns the orbit
        auto adoptOrbit = [=, &app](mc_mandelbrot_orbit* made) -> std::string {
            const auto t0 = std::chrono::steady_clock::now();
            int rc;
            if (!blaDevice && precision == MC_PRECISION_PERTURB_BLA && (rc = mc_mandelbrot_orbit_bla(made, nullptr, nullptr)) != MC_OK) {   // the table, on the host
                mc_mandelbrot_orbit_destroy(made);
                return message("mc_mandelbrot_orbit_bla: %s (%s)", mc_error_string(rc), mc_last_error_detail());
            }
            if (!blaDevice && precision == MC_PRECISION_PERTURB_BLA_DEEP && (rc = mc_mandelbrot_orbit_bla_deep(made, nullptr, nullptr)) != MC_OK) {
                mc_mandelbrot_orbit_destroy(made);
                return message("mc_mandelbrot_orbit_bla_deep: %s (%s)", mc_error_string(rc), mc_last_error_detail());
            }
            if (!blaDevice && (blaTableSet || zoomOrbitShared) && (precision == MC_PRECISION_PERTURB_BLA || precision == MC_PRECISION_PERTURB_BLA_DEEP))
                printf("table: %.3f ms (host; uploaded by the bind)\n",
                       std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            app.setOrbit(made);   // bound to the context by init(), before the warm-up thread starts
            return std::string();
        };
        // shift: --zoom's keyframes, the scale's exponent raised by that much (0: the view itself)
        auto makeOrbit = [=](mc_context* ctx, int shift) -> std::string {
            mc_mandelbrot_orbit* made = nullptr;
            const std::string err = createOrbit(ctx, shift, &made);
            return err.empty() ? adoptOrbit(made) : err;
        };
        if (blaDevice)
            app.setDeviceTables(precision == MC_PRECISION_PERTURB_BLA ? (uint32_t)MC_ORBIT_TABLE_BLA : (uint32_t)MC_ORBIT_TABLE_BLA_DEEP);
        if (zoomSet && zoomOrbitShared) {   // the deepest keyframe's orbit, made with the first keyframe; keyframe j takes its table under its own scale
            std::shared_ptr<mc_mandelbrot_orbit*> deepest(new mc_mandelbrot_orbit*(nullptr), [](mc_mandelbrot_orbit** p) {
                if (*p) mc_mandelbrot_orbit_destroy(*p);
                delete p;
            });
            app.setZoom((uint32_t)zoomK, (uint32_t)zoomF, cx, cy, sx, sy,
                        [=](mc_context* c, int shift) -> std::string {
                            if (!*deepest) {
                                const std::string err = createOrbit(onDevice ? c : nullptr, 0, deepest.get());
                                if (!err.empty()) return err;
                            }
                            mc_mandelbrot_orbit* made = nullptr;
                            const int rc = mc_mandelbrot_orbit_rescale(*deepest, mantX, mantY, e + shift, &made);
                            if (rc != MC_OK) return message("mc_mandelbrot_orbit_rescale: %s (%s)", mc_error_string(rc), mc_last_error_detail());
                            return adoptOrbit(made);
                        });
        } else if (zoomSet) {   // one orbit per keyframe, made by runZoom() as the keyframes come
            app.setZoom((uint32_t)zoomK, (uint32_t)zoomF, cx, cy, sx, sy,
                        [makeOrbit, onDevice](mc_context* c, int shift) { return makeOrbit(onDevice ? c : nullptr, shift); });
        } else if (onDevice) {
            app.setOrbitFactory([makeOrbit](mc_context* c) { return makeOrbit(c, 0); });   // needs the context: made in init(), once it exists
        } else {
            const std::string err = makeOrbit(nullptr, 0);
            if (!err.empty()) {
                printf("%s\n", err.c_str());
                return EXIT_FAILURE;
            }
        }
    }
#elif defined(PATHTRACER_MODE)
    const int32_t spp = pos.size() > 0 ? atoi(pos[0]) : 500;                           // samples per pixel
    const uint32_t resy = pos.size() > 1 ? static_cast<uint32_t>(atoi(pos[1])) : 600;  // vertical pixel resolution
    const uint32_t resx = resy * 3 / 2;                                                // horizontal pixel resolution
    PathtracerApp app = PathtracerApp(resx, resy, spp, 16, quiet);
    app.setMathMode(mathMode);
    if (largeSpheres) app.useLargeSphereWalls();
    app.setSpherePrecision(spherePrec);
    app.setDenoise(denoise);
    app.setNoiseGuided(noiseGuided);
    if (budgetSet) app.setBudget(budget);
    if (sceneFile) {   // read and checked here, before a device is touched
        const std::string err = app.loadScene(sceneFile);
        if (!err.empty()) { printf("--scene %s: %s\n", sceneFile, err.c_str()); return EXIT_FAILURE; }
    }
    if (accel) {       // the BVH is built on the host, here
        const std::string err = app.useAccel();
        if (!err.empty()) { printf("--accel bvh: %s\n", err.c_str()); return EXIT_FAILURE; }
    }
#endif
    app.setNumGpus(gpus);
    app.setQuiet(quiet);
    app.setGpuPostprocess(gpuPost);
    app.setPngThreads(pngThreads);
    app.setOverlapStart(overlapStart);
    app.setStreamedSave(streamedSave);   // this program always saves what it renders (the Mandelbrot app streams; the path tracer's first
                                         // output rows are its last storage rows, and its PNG is 3 ms beside a 14 ms kernel)
    if (referencePng && !ComputeApp::referencePngAvailable()) {   // said before anything is rendered
        printf("--reference-png: this binary was built without the reference's PNG codec; rebuild with `make REFERENCE=<checkout of "
               "pjhusky/vulkan-compute-tests>` (its src/external/lodepng is compiled where it lies)\n");
        return EXIT_FAILURE;
    }
    app.setReferencePng(referencePng);

    const auto tStart = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
    try {
        // the reference calls init()/preRun() outside its try block (main.cpp:28-29); a missing device
        // then terminates via an uncaught exception.  Kept inside here so the failure is reported.
        app.init();
        const double initMs = since(tStart);
        app.preRun();
        printf("now running app!\n");
#if defined(MANDELBROT_MODE)
        if (zoomSet) {   // keyframes, frames and files in one pass (MandelbrotApp::runZoom)
            app.runZoom(outFile ? outFile : "mandelbrot.png");
            if (!fullTeardown) {
                fflush(stdout);
                fflush(stderr);
                std::_Exit(EXIT_SUCCESS);
            }
            return EXIT_SUCCESS;
        }
#endif
        app.run();
#if defined(MANDELBROT_MODE)
        if (adaptive) app.printRefined();   // "refined R of P pixels" (mc_context_last_refined)
        if (exactCheck) app.printExactCheck((uint32_t)exactCheck, (uint32_t)exactExtraLimbs);   // "exact check: A of N equal (limbs n, T ms)"
        if (adaptiveSmooth) app.printRefinedSmooth();   // "refined R of P pixels (threshold Q)"
        if (colour == MC_MANDEL_COLOUR_DISTANCE && gpus <= 1) app.printDistanceShare();
        if (colour == MC_MANDEL_COLOUR_SMOOTH_EQUALISED && gpus <= 1 && !supersampleSmooth && !adaptiveSmooth) app.printSmoothEqualisedStats();
#endif
#if defined(PATHTRACER_MODE)
        if (budgetSet) app.printBudget();
#endif
        if (denoise && noiseGuidedSet)
            printf("denoise: %u passes, noise-guided (k_noise %g), %.3f ms device time (render in two halves + guides + noise plane + filter)\n",
                   denoise, noiseGuided, app.timing().kernelMs);
        else if (denoise) printf("denoise: %u passes, %.3f ms device time (render + guides + filter)\n", denoise, app.timing().kernelMs);
        auto t0 = std::chrono::steady_clock::now();
        if (outFile) app.saveRenderedImage(outFile);
        else app.saveRenderedImage();
        double saveMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (!quiet) printf("saveRenderedImage() finished in %.3f ms\n", saveMs);
#if defined(MANDELBROT_MODE)
        if (locate) app.printLocate(locate);   // "locate: ..." and one line per domain, each with a ready --centre X Y
#endif
        if (timingJson) {   // init = context creation (HIP start-up); alloc = the pinned storage buffer; run = the blocking render call, of
                            // which kernel + copy are device time; convert = float -> u8 (+ rotation) on the host (0: done on the device);
                            // png = encode + write; total = process wall time up to here
            const ComputeApp::Timing& t = app.timing();
            // (warmup = the warm-up call on its helper thread, warmup_wait = what run() still waited for it: computeApp.h)
            printf("{\"timing_ms\": {\"init\": %.3f, \"alloc\": %.3f, \"run\": %.3f, \"kernel\": %.3f, \"copy\": %.3f, \"convert\": %.3f, "
                   "\"png\": %.3f, \"total\": %.3f, \"warmup\": %.3f, \"warmup_wait\": %.3f, \"streamed_bands\": %d, "
                   "\"png_join\": %.3f, \"png_assemble\": %.3f, \"png_write\": %.3f}, "
                   "\"gpu_postprocess\": %s, \"gpus\": %d, \"overlap_start\": %s, \"reference_png\": %s, \"denoise\": %u, \"noise_guided\": %g, \"accel\": \"%s\", "
                   "\"main_at_ms\": %.3f, \"end_at_ms\": %.3f}\n",
                   initMs, t.allocMs, t.runMs, t.kernelMs, t.copyMs, t.convertMs, t.pngMs, since(tStart), t.warmupMs,
                   t.warmupWaitMs, t.streamedBands, t.pngJoinMs, t.pngAssembleMs, t.pngWriteMs, gpuPost ? "true" : "false", gpus, overlapStart ? "true" : "false", referencePng ? "true" : "false", denoise, noiseGuided, accel ? "bvh" : "linear",
                   // CLOCK_MONOTONIC at main()'s first timed statement and now: a parent that reads the same clock around the process
                   // gets what `total` cannot contain — loading + static initialisers before main(), teardown after it
                   std::chrono::duration<double, std::milli>(tStart.time_since_epoch()).count(),
                   std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count());
        }
    } catch (const std::runtime_error& e) {
        printf("%s\n", e.what());
        return EXIT_FAILURE;
    }

    // The picture is on disk and everything is printed.  Destroying the context, unregistering the storage buffer and the HIP runtime's
    // own exit handlers take another 45 - 50 ms (profiles/r06_init_spread_probe.txt: a third of a K2 process) to give back what the
    // operating system reclaims at exit anyway: leave at once unless asked (--full-teardown: leak checkers, sanitizers, the tests).
    if (!fullTeardown) {
        fflush(stdout);
        fflush(stderr);
        std::_Exit(EXIT_SUCCESS);
    }
    return EXIT_SUCCESS;
}
