// MandelbrotApp — mirrors src/mandelbrotApp.h:8-194 of the reference on top of ComputeApp.
#ifndef MANDELBROTAPP_H_
#define MANDELBROTAPP_H_

#include <algorithm>
#include <chrono>
#include <cmath>

#include "computeApp.h"
#include "pngWriter.h"

struct MandelbrotApp : public ComputeApp {
    // Same signature as the reference (mandelbrotApp.h:10).  workgroupSize is accepted for source
    // compatibility; the HIP kernels choose their own tiling (8x8 pixels per wave64).
    MandelbrotApp(const uint32_t resx, const uint32_t resy, const uint32_t workgroupSize = 32) {
        this->resx = resx;
        this->resy = resy;
        this->workgroupSize = workgroupSize;
        bufferSize = (uint64_t)sizeof(Pixel) * resx * resy;   // mandelbrotApp.h:16 (uint32_t there)
        mc_mandelbrot_default_params(resx, resy, &params);    // M=128, centre (-0.445,0), scale 2.34, kColor {0.1,0.7,0.6,0}
    }

    // -- additions: the reference hard-codes these in the shader (mandelbrot.comp:5-6,38,40) --
    void setMaxIter(uint32_t m) { params.max_iter = m; }
    void setView(double cx, double cy, double sx, double sy) {
        split(cx, params.centre_x_hi, params.centre_x_lo);
        split(cy, params.centre_y_hi, params.centre_y_lo);
        split(sx, params.scale_x_hi, params.scale_x_lo);
        split(sy, params.scale_y_hi, params.scale_y_lo);
    }
    void setColourFlags(uint32_t flags) { params.flags |= flags; }   // MC_MANDEL_COLOUR_EQUALISED, _SMOOTH, _DISTANCE, _SMOOTH_EQUALISED (main.cpp --colour)
    // --adaptive-smooth[=Q]: run() renders through mc_mandelbrot_render_adaptive_smooth with this threshold
    void setAdaptiveSmoothThreshold(uint32_t q) { adaptiveSmoothQ = q; }
    void setSupersample(uint32_t s) { params.flags |= MC_MANDEL_SUPERSAMPLE(s); }   // 2, 4 or 8 (main.cpp --supersample)
    void setPrecision(uint32_t precision) { params.precision = precision; }   // MC_PRECISION_F32 / _DS / _F64 (setView packs the same words)
    // MC_PRECISION_PERTURB / _BLA / _BLA_DEEP: the view is this orbit's (the app owns it; for the BLA precisions main() has built the
    // table); the params' view words are zero.  Bound in contextCreated().
    void setOrbit(mc_mandelbrot_orbit* o) {
        if (orbit) mc_mandelbrot_orbit_destroy(orbit);
        orbit = o;
        setView(0.0, 0.0, 0.0, 0.0);
    }
    // --bla-table device: the orbit carries no table; every bind builds the named ones (MC_ORBIT_TABLE_*) on the device
    // and prints how long that took.  0 (the default): the plain bind of the table main() built.
    void setDeviceTables(uint32_t tables) { deviceTables = tables; }
    // --orbit device | auto: the orbit is made on the context's device (mc_mandelbrot_orbit_create_device), so only once the context
    // exists: contextCreated() calls the factory before the bind and before the warm-up helper starts.  It calls setOrbit(), or
    // returns the message the run ends with.
    void setOrbitFactory(std::function<std::string(mc_context*)> f) { orbitFactory = std::move(f); }
    // --zoom K F: the view (cx, cy, sx, sy) is the DEEPEST of K + 1 keyframes, keyframe j at that scale x 2^(K - j).
    // keyOrbit, for the perturbation precisions: makes keyframe j's orbit (the scale's exponent shifted by K - j) and hands it to
    // setOrbit(), or returns the message the run ends with; runZoom() binds it.  The warm-up is skipped: no orbit is bound before the
    // first keyframe, and every keyframe is a render of its own.
    void setZoom(uint32_t K, uint32_t F, double cx, double cy, double sx, double sy, std::function<std::string(mc_context*, int)> keyOrbit) {
        zoomK = K; zoomF = F; zoomCx = cx; zoomCy = cy; zoomSx = sx; zoomSy = sy;
        zoomOrbit = std::move(keyOrbit);
    }
    // --zoom-keyframes counts: runZoom() keeps the keyframes as count planes (mc_mandelbrot_zoom_counts_*) and every frame
    // is coloured through one map blended from the two keyframes' maps; colours (the default): the vec4 sequence.
    void setZoomCounts(bool counts) { zoomCounts = counts; }
    // --zoom-filter area: runZoom() composes every frame through the _frame_filtered calls with
    // MC_MANDEL_ZOOM_FILTER_AREA; bilinear (the default): the unfiltered calls, as before the option existed.
    void setZoomFilter(uint32_t filter) { zoomFilter = filter; }
    // --buddhabrot SAMPLES: run() renders the orbit-density plane(s) through mc_buddhabrot_render instead of the
    // Mandelbrot set, tone-maps them into the storage buffer and the save goes on as ever.  view: --centre / --scale when given (else the
    // library's default view); maxIter: --max-iter when given (else the library's 1000); nebula: three renders of max_iter MR MG MB, one
    // per colour channel, instead of one grey plane; equalised: the rank map of each plane's histogram instead of the square-root map.
    struct Buddhabrot {
        uint64_t samples = 0;   // 0: off
        uint32_t maxIter = 0, minIter = 0, seed = 1;
        bool viewSet = false, windowSet = false, nebula = false, equalised = false;
        double view[4] = {0, 0, 0, 0}, window[4] = {0, 0, 0, 0};
        uint32_t nebulaIter[3] = {0, 0, 0};
        double whitePct = 99.9;
        // --guided[=G]: every channel through mc_buddhabrot_render_guided, one pilot per channel; 0 / unset: the
        // library's defaults (mc_buddhabrot_guide_default_params)
        bool guided = false, pilotSet = false, dilateSet = false;
        uint32_t guideLog2 = 0, dilate = 0, unbiased = 0;
        uint64_t pilot = 0;
    };
    void setBuddhabrot(const Buddhabrot& b) { buddha = b; }
    ~MandelbrotApp() { if (orbit) mc_mandelbrot_orbit_destroy(orbit); }
    MandelbrotApp(const MandelbrotApp&) = delete;
    MandelbrotApp& operator=(const MandelbrotApp&) = delete;

    virtual void preRun() override {
        if (!quiet) { printf(" * before createBuffer()\n"); fflush(stdout); }
        createBuffer(bufferSize);   // output buffer
    }

    void bindOrbit() {
        if (!deviceTables) {
            check(mc_context_bind_mandelbrot_orbit(ctx, orbit), "mc_context_bind_mandelbrot_orbit");
            return;
        }
        check(mc_context_bind_mandelbrot_orbit_tables(ctx, orbit, deviceTables), "mc_context_bind_mandelbrot_orbit_tables");
        double tableMs = 0.0;
        uint32_t launches = 0;
        check(mc_context_last_table_timing(ctx, &tableMs, &launches), "mc_context_last_table_timing");
        printf("table: %.3f ms (device, %u launches; built by the bind)\n", tableMs, launches);
    }

    // The request run() makes: push constant kColor (mandelbrotApp.h:139-141) and ONE dispatch over the whole image (:146)
    mc_mandelbrot_params request() const {
        mc_mandelbrot_params q = params;
        q.k_color[0] = 0.1f; q.k_color[1] = 0.7f; q.k_color[2] = 0.6f; q.k_color[3] = 0.0f;
        q.row_begin = 0; q.row_end = resy;
        return q;
    }
    virtual void createCommandBuffer() override { params = request(); }

    virtual void contextCreated() override {
        if (orbitFactory) {
            const std::string err = orbitFactory(ctx);
            if (!err.empty()) throw std::runtime_error(err);
        }
        if (orbit) bindOrbit();
    }

    virtual std::function<int()> warmupCall() const override {   // tables + code object of that request (bit 1: the banded render's second stream)
        if (zoomK || buddha.samples) return [] { return (int)MC_OK; };
        return [ctx = ctx, q = request(), how = (gpuPostprocess ? 1 : 0) | (streaming() ? 2 : 0)] { return mc_context_warmup_mandelbrot(ctx, &q, how); };
    }

    virtual void runCommandBuffer() override {
        if (buddha.samples) { runBuddhabrot(); return; }
        if (streaming()) { runStreamed(); return; }
        if (!multi && (params.flags & MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE)) {   // the caller's threshold: the call that takes one
            check(mc_mandelbrot_render_adaptive_smooth(ctx, &params, adaptiveSmoothQ, gpuPostprocess ? nullptr : buffer.data(),
                                                       gpuPostprocess ? rgba8.bytes() : nullptr), "mc_mandelbrot_render_adaptive_smooth");
            return;
        }
        if (gpuPostprocess) {   // render + float->u8 on the device: 4 B/pixel cross PCIe instead of 16
            if (multi) check(mc_multi_mandelbrot_render_rgba8(multi, &params, rgba8.bytes()), "mc_multi_mandelbrot_render_rgba8");
            else check(mc_mandelbrot_render_rgba8(ctx, &params, rgba8.bytes()), "mc_mandelbrot_render_rgba8");
            return;
        }
        if (!multi && (params.flags & MC_MANDEL_COLOUR_DISTANCE)) {   // the colours and D from one render (printDistanceShare reads D)
            distance.resize((size_t)resx * resy);
            check(mc_mandelbrot_render_distance(ctx, &params, buffer.data(), nullptr, nullptr, distance.data()), "mc_mandelbrot_render_distance");
            return;
        }
        if (multi) check(mc_multi_mandelbrot_render(multi, &params, buffer.data(), nullptr), "mc_multi_mandelbrot_render");
        else check(mc_mandelbrot_render(ctx, &params, buffer.data(), nullptr), "mc_mandelbrot_render");
    }

    // mandelbrotApp.h:149-170: u8 = static_cast<uint8_t>(scale * c), alpha 255.  The cast is UB out of
    // range; the reference binary on x86-64 truncates to int32 and keeps the low byte — stated explicitly.
    void getRenderedImage(std::vector<uint8_t>& image, const uint32_t resx, const uint32_t resy, float floatScaleFactor) {
        convertStorage(image, resx, resy, floatScaleFactor, false);   // the loop of :159-166, row stripes in parallel
    }

    virtual void saveRenderedImage(const char* png_filename = "mandelbrot.png") override {
        saveImage(png_filename, resx, resy, 255.0f, false, true);   // mandelbrotApp.h:172-184: scale 255, "writing" after getRenderedImage
    }

    const HostStorage& storageBuffer() const { return buffer; }

    // --zoom K F: K + 1 keyframes through mc_mandelbrot_zoom_push, K * F + 1 frames through mc_mandelbrot_zoom_frame, each saved as it
    // arrives under `out` with _%05u before its extension.  Frame 0 is keyframe 0 (composed from it alone at r = 1); once keyframe j >= 1
    // is pushed, frames (j - 1) F + 1 .. j F follow from keyframes j - 1 and j at r = mc_mandelbrot_zoom_ratio(1 .. F, F), the last of
    // them (r = 0.5) being keyframe j bit for bit.  --gpu-postprocess takes the RGBA8 form: the compose kernel writes the bytes itself.
    // --zoom-keyframes counts: the same keyframes, frames and lines through mc_mandelbrot_zoom_counts_push / _frame with (step, F).
    void runZoom(const char* out) {
        using clock = std::chrono::steady_clock;
        auto ms = [](clock::time_point t) { return std::chrono::duration<double, std::milli>(clock::now() - t).count(); };
        if (multi) throw std::runtime_error("--zoom: one GPU (the keyframes stay on the context's device)");
        createCommandBuffer();
        waitWarmup();
        const auto tStart = clock::now();
        mc_mandelbrot_zoom* z = nullptr;
        mc_mandelbrot_zoom_counts* zc = nullptr;
        if (zoomCounts) check(mc_mandelbrot_zoom_counts_create(ctx, resx, resy, &zc), "mc_mandelbrot_zoom_counts_create");
        else check(mc_mandelbrot_zoom_create(ctx, resx, resy, &z), "mc_mandelbrot_zoom_create");
        struct Guard {
            mc_mandelbrot_zoom* z;
            mc_mandelbrot_zoom_counts* zc;
            ~Guard() { mc_mandelbrot_zoom_destroy(z); mc_mandelbrot_zoom_counts_destroy(zc); }
        } guard{z, zc};
        const std::string name(out);
        size_t dot = name.find_last_of('.');
        const size_t slash = name.find_last_of('/');
        if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) dot = name.size();
        double keyMs = 0.0, composeMs = 0.0, saveMs = 0.0;
        uint32_t frames = 0;
        auto emit = [&](uint32_t step) {
            auto t = clock::now();
            float* f32 = gpuPostprocess ? nullptr : buffer.data();
            uint8_t* u8 = gpuPostprocess ? rgba8.bytes() : nullptr;
            const bool filtered = zoomFilter != MC_MANDEL_ZOOM_FILTER_BILINEAR;
            if (zoomCounts) {
                if (filtered) check(mc_mandelbrot_zoom_counts_frame_filtered(zc, step, zoomF, zoomFilter, f32, u8), "mc_mandelbrot_zoom_counts_frame_filtered");
                else check(mc_mandelbrot_zoom_counts_frame(zc, step, zoomF, f32, u8), "mc_mandelbrot_zoom_counts_frame");
            } else {
                double r = 0.0;
                check(mc_mandelbrot_zoom_ratio(step, zoomF, &r), "mc_mandelbrot_zoom_ratio");
                if (filtered) check(mc_mandelbrot_zoom_frame_filtered(z, r, zoomFilter, f32, u8), "mc_mandelbrot_zoom_frame_filtered");
                else check(mc_mandelbrot_zoom_frame(z, r, f32, u8), "mc_mandelbrot_zoom_frame");
            }
            composeMs += ms(t);
            char num[16];
            snprintf(num, sizeof num, "_%05u", frames);
            const std::string file = name.substr(0, dot) + num + name.substr(dot);
            t = clock::now();
            saveImage(file.c_str(), resx, resy, 255.0f, false, true);
            saveMs += ms(t);
            frames++;
        };
        for (uint32_t j = 0; j <= zoomK; j++) {
            const int shift = (int)(zoomK - j);
            const auto t = clock::now();
            if (zoomOrbit) {
                const std::string err = zoomOrbit(ctx, shift);
                if (!err.empty()) throw std::runtime_error(err);
                bindOrbit();
            } else {
                setView(zoomCx, zoomCy, std::ldexp(zoomSx, shift), std::ldexp(zoomSy, shift));
            }
            if (zoomCounts) check(mc_mandelbrot_zoom_counts_push(zc, &params), "mc_mandelbrot_zoom_counts_push");
            else check(mc_mandelbrot_zoom_push(z, &params), "mc_mandelbrot_zoom_push");
            const double pushMs = ms(t);
            keyMs += pushMs;
            double kernel = 0.0;
            (void)mc_context_last_timing(ctx, &kernel, nullptr);
            printf("keyframe %u of %u: the view's scale x 2^%d, %.3f ms (kernels %.3f ms)\n", j, zoomK, shift, pushMs, kernel);
            if (j == 0) {
                emit(0u);   // (r = 1: keyframe 0 alone)
            } else {
                for (uint32_t s = 1; s <= zoomF; s++) emit(s);
            }
        }
        printf("zoom: %u keyframes in %.3f ms, %u frames composed in %.3f ms and saved in %.3f ms, %.3f ms in all\n", zoomK + 1, keyMs, frames,
               composeMs, saveMs, ms(tStart));
    }

    // --adaptive: how many pixels the last render sampled s x s (the share above which plain supersampling is the faster call: DESIGN.md §3.12)
    void printRefined() {
        uint64_t refined = 0, pixels = 0;
        check(mc_context_last_refined(ctx, &refined, &pixels), "mc_context_last_refined");
        printf("refined %llu of %llu pixels\n", (unsigned long long)refined, (unsigned long long)pixels);
    }

    // --adaptive-smooth: the same report with the threshold the render used
    void printRefinedSmooth() {
        uint64_t refined = 0, pixels = 0;
        check(mc_context_last_refined(ctx, &refined, &pixels), "mc_context_last_refined");
        printf("refined %llu of %llu pixels (threshold %u)\n", (unsigned long long)refined, (unsigned long long)pixels, adaptiveSmoothQ);
    }

    // --exact-check N: N pixels of the view, the centre pixel and a fixed lattice of N - 1, iterated exactly on the
    // device (mc_mandelbrot_exact_counts_device) and compared with the render's counts.  The save keeps colours only: the count plane is
    // rendered once more, without the colouring and sampling flags.
    void printExactCheck(uint32_t n, uint32_t extraLimbs) {
        std::vector<uint32_t> gx(n), gy(n), exact(n);
        std::vector<double> dcx(n), dcy(n);
        gx[0] = resx / 2; gy[0] = resy / 2;
        uint32_t cols = 1;
        while ((uint64_t)cols * cols < n - 1u) cols++;
        const uint32_t rows = n > 1 ? (n - 1u + cols - 1u) / cols : 1u;
        for (uint32_t i = 1; i < n; i++) {
            gx[i] = (uint32_t)(((uint64_t)(2u * ((i - 1u) % cols) + 1u) * resx) / (2u * cols));
            gy[i] = (uint32_t)(((uint64_t)(2u * ((i - 1u) / cols) + 1u) * resy) / (2u * rows));
        }
        mc_mandelbrot_params q = params;
        q.flags = 0;
        std::vector<uint32_t> plane((size_t)resx * resy);
        check(mc_mandelbrot_render(ctx, &q, nullptr, plane.data()), "mc_mandelbrot_render");
        int32_t e = 0;
        check(mc_mandelbrot_exact_pixel_offsets(orbit, resx, resy, n, gx.data(), gy.data(), dcx.data(), dcy.data(), &e),
              "mc_mandelbrot_exact_pixel_offsets");
        check(mc_mandelbrot_exact_counts_device(ctx, orbit, params.max_iter, extraLimbs, n, dcx.data(), dcy.data(), e, exact.data()),
              "mc_mandelbrot_exact_counts_device");
        double ms = 0.0;
        uint32_t limbs = 0;
        check(mc_context_last_exact_timing(ctx, &ms, nullptr, &limbs, nullptr, nullptr), "mc_context_last_exact_timing");
        uint32_t equal = 0;
        for (uint32_t i = 0; i < n; i++) equal += plane[(size_t)gy[i] * resx + gx[i]] == exact[i] ? 1u : 0u;
        printf("exact check: %u of %u equal (limbs %u, %.3f ms)\n", equal, n, limbs, ms);
        uint32_t shown = 0;
        for (uint32_t i = 0; i < n && shown < 8u; i++) {
            const uint32_t r = plane[(size_t)gy[i] * resx + gx[i]];
            if (r != exact[i]) {
                printf("  pixel (%u, %u): render %u, exact %u\n", gx[i], gy[i], r, exact[i]);
                shown++;
            }
        }
    }

    // --locate[=N]: one atom render of the view (mc_mandelbrot_render_atom, at the image's own size), its domains
    // (mc_mandelbrot_atom_domains), then for each of the N periods >= 1 with the most pixels (ties: the smaller period) Newton's method
    // from the domain's best pixel (mc_mandelbrot_nucleus_refine) and the nucleus as text (mc_mandelbrot_orbit_offset_text).  F32 / F64:
    // an orbit at centre "0", "0" of the view's scale with the pixel's own c as the offset; PERTURB: the view's orbit and the pixel's dc.
    // An entry whose nucleus agrees with a smaller listed period's to 2^-40 of the scale is marked "= period q" (the minimum inside a
    // component can fall on a multiple of its period): which to dive into is left to the reader.
    void printLocate(uint32_t count) {
        using clock = std::chrono::steady_clock;
        auto ms = [](clock::time_point t) { return std::chrono::duration<double, std::milli>(clock::now() - t).count(); };
        const auto tStart = clock::now();
        const uint32_t W = resx, H = resy, M = params.max_iter;
        const bool perturb = params.precision == MC_PRECISION_PERTURB, f32 = params.precision == MC_PRECISION_F32;
        mc_mandelbrot_params q = params;
        q.flags = 0;
        std::vector<uint32_t> period((size_t)W * H), cnt((size_t)M + 1), best((size_t)M + 1);
        std::vector<double> amin((size_t)W * H), low((size_t)M + 1);
        check(mc_mandelbrot_render_atom(ctx, &q, nullptr, period.data(), amin.data()), "mc_mandelbrot_render_atom");
        const double renderMs = ms(tStart);
        check(mc_mandelbrot_atom_domains(period.data(), amin.data(), (uint64_t)W * H, M, cnt.data(), low.data(), best.data()),
              "mc_mandelbrot_atom_domains");
        // the view as the kernels read it, and the orbit Newton runs on
        double cx = 0.0, cy = 0.0, sx = 0.0, sy = 0.0;
        mc_mandelbrot_orbit* zero = nullptr;
        struct Guard {
            mc_mandelbrot_orbit*& o;
            ~Guard() { if (o) mc_mandelbrot_orbit_destroy(o); }
        } guard{zero};
        auto pixelOffset = [&](uint32_t gx, uint32_t gy, double off[2]) {
            if (perturb) {
                int32_t e = 0;
                check(mc_mandelbrot_exact_pixel_offsets(orbit, W, H, 1, &gx, &gy, &off[0], &off[1], &e), "mc_mandelbrot_exact_pixel_offsets");
            } else if (f32) {   // mandelbrot.comp:30-31,38 in fp32, then the exact conversion
                off[0] = (double)(params.centre_x_hi + ((float)gx / (float)W - 0.5f) * params.scale_x_hi);
                off[1] = (double)(params.centre_y_hi + ((float)gy / (float)H - 0.5f) * params.scale_y_hi);
            } else {
                off[0] = cx + ((double)gx / (double)W - 0.5) * sx;
                off[1] = cy + ((double)gy / (double)H - 0.5) * sy;
            }
        };
        if (perturb) {
            double corner[2];
            pixelOffset(0u, 0u, corner);   // (0 / n - 0.5) * scale, exactly
            sx = -2.0 * corner[0];
            sy = -2.0 * corner[1];
        } else {
            cx = f32 ? (double)params.centre_x_hi : (double)params.centre_x_hi + (double)params.centre_x_lo;
            cy = f32 ? (double)params.centre_y_hi : (double)params.centre_y_hi + (double)params.centre_y_lo;
            sx = f32 ? (double)params.scale_x_hi : (double)params.scale_x_hi + (double)params.scale_x_lo;
            sy = f32 ? (double)params.scale_y_hi : (double)params.scale_y_hi + (double)params.scale_y_lo;
            check(mc_mandelbrot_orbit_create("0", "0", sx, sy, M, &zero), "mc_mandelbrot_orbit_create");
        }
        const mc_mandelbrot_orbit* o = perturb ? orbit : zero;
        std::vector<uint32_t> order;
        for (uint32_t v = 1; v <= M; v++)
            if (cnt[v]) order.push_back(v);
        const size_t periods = order.size();
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cnt[a] > cnt[b]; });
        if (order.size() > count) order.resize(count);
        const double smin = std::fmin(std::fabs(sx), std::fabs(sy));
        const uint32_t digits = (uint32_t)std::fmax(0.0, std::ceil(-std::log10(smin))) + 20u;
        printf("locate: atom plane %u x %u, %zu periods, render %.3f ms; the %zu largest domains (centres with %u fractional digits):\n", W, H,
               periods, renderMs, order.size(), digits);
        struct Entry { uint32_t p; int rc; std::string why; double o[2]; uint32_t steps; double last[2]; };
        std::vector<Entry> found;
        for (uint32_t p : order) {   // every nucleus first: an entry is compared with all the others
            Entry e{p, MC_OK, "", {0.0, 0.0}, 0u, {0.0, 0.0}};
            pixelOffset(best[p] % W, best[p] / W, e.o);
            e.rc = mc_mandelbrot_nucleus_refine(o, p, 64u, e.o, &e.steps, e.last);
            if (e.rc != MC_OK) e.why = std::string(mc_error_string(e.rc)) + " (" + mc_last_error_detail() + ")";
            found.push_back(e);
        }
        std::vector<char> tx((size_t)digits + 32), ty((size_t)digits + 32);
        for (const Entry& e : found) {
            const uint32_t p = e.p;
            printf("  period %u: %u pixels, best pixel (%u, %u) amin %.6g, ", p, cnt[p], best[p] % W, best[p] / W, low[p]);
            if (e.rc != MC_OK) {
                printf("Newton failed: %s\n", e.why.c_str());
                continue;
            }
            const double px = ((e.o[0] - cx) / sx + 0.5) * (double)W, py = ((e.o[1] - cy) / sy + 0.5) * (double)H;
            const bool inside = px >= 0.0 && px < (double)W && py >= 0.0 && py < (double)H;
            const bool converged = std::fmax(std::fabs(e.last[0]), std::fabs(e.last[1])) <=
                                   std::ldexp(1.0, -52) * std::fmax(std::fabs(e.o[0]), std::fabs(e.o[1]));
            check(mc_mandelbrot_orbit_offset_text(o, e.o[0], e.o[1], digits, tx.data(), ty.data(), tx.size()), "mc_mandelbrot_orbit_offset_text");
            printf("Newton %u steps%s to pixel (%.2f, %.2f), %s", e.steps, converged ? "" : " (not converged)", px, py,
                   inside ? "inside" : "outside view");
            uint32_t same = 0;   // the smallest listed period with the same nucleus
            for (const Entry& f : found)
                if (f.rc == MC_OK && f.p < p && (same == 0u || f.p < same) && std::fabs(f.o[0] - e.o[0]) <= std::ldexp(std::fabs(sx), -40) &&
                    std::fabs(f.o[1] - e.o[1]) <= std::ldexp(std::fabs(sy), -40))
                    same = f.p;
            if (same) printf(", = period %u", same);
            printf(": --centre %s %s\n", tx.data(), ty.data());
        }
        printf("locate: %.3f ms in all\n", ms(tStart));
    }

    // --colour distance: the share of pixels whose distance estimate is below one pixel, the ones the shading darkens.  D came with the
    // colours where the storage buffer was rendered; the RGBA8 route (--gpu-postprocess) left none behind and renders the plane once more.
    void printDistanceShare() {
        if (distance.empty()) {
            distance.resize((size_t)resx * resy);
            check(mc_mandelbrot_render_distance(ctx, &params, nullptr, nullptr, nullptr, distance.data()), "mc_mandelbrot_render_distance");
        }
        uint64_t below = 0;
        for (float d : distance) below += d < 1.0f ? 1u : 0u;
        printf("distance below 1 pixel: %llu of %llu pixels (%.2f %%)\n", (unsigned long long)below, (unsigned long long)distance.size(),
               100.0 * (double)below / (double)distance.size());
    }

    // --colour smooth-equalised: how many pixels escaped and how many of the histogram's bins (integer parts of the smooth count) they
    // occupy, the knots the palette is spread over.  The image came through the whole-image calls, which keep no plane: q is rendered
    // once more.
    void printSmoothEqualisedStats() {
        std::vector<uint32_t> q((size_t)resx * resy);
        check(mc_mandelbrot_render_smooth_equalised(ctx, &params, nullptr, nullptr, q.data(), nullptr), "mc_mandelbrot_render_smooth_equalised");
        const uint32_t M = params.max_iter;
        std::vector<uint8_t> seen(M, 0);
        uint64_t escaped = 0, occupied = 0;
        for (uint32_t v : q)
            if (v < 256u * M) {
                escaped++;
                if (!seen[v >> 8]) { seen[v >> 8] = 1; occupied++; }
            }
        printf("smooth equalised: %llu of %llu pixels escaped, %llu of %u bins occupied\n", (unsigned long long)escaped,
               (unsigned long long)q.size(), (unsigned long long)occupied, M);
    }

private:
    // --buddhabrot: one render per channel, the stats line of each, the white level, the maps, the tone map, [the conversion on the device].
    // The white level L is APP POLICY, not part of the ABI: the density not exceeded by whitePct % of the non-empty bins — the smallest
    // v >= 1 with (double)#{bins: 1 <= d <= v} >= (whitePct / 100) * (double)#{bins: d >= 1} — read from ONE histogram of min(d, 2^20 - 1)
    // over all the planes; 1 when every bin is empty.  --tone equalised ranks each plane's densities among its NON-EMPTY bins (the empty
    // bin's count is dropped from the histogram before mc_mandelbrot_equalise_map, so the background does not spend the palette).
    void runBuddhabrot() {
        const uint32_t channels = buddha.nebula ? 3u : 1u;
        const size_t npix = (size_t)resx * resy;
        mc_buddhabrot_params bp;
        check(mc_buddhabrot_default_params(resx, resy, buddha.samples, &bp), "mc_buddhabrot_default_params");
        if (buddha.viewSet) { bp.view_centre_x = buddha.view[0]; bp.view_centre_y = buddha.view[1]; bp.view_scale_x = buddha.view[2]; bp.view_scale_y = buddha.view[3]; }
        if (buddha.windowSet) { bp.sample_centre_x = buddha.window[0]; bp.sample_centre_y = buddha.window[1]; bp.sample_scale_x = buddha.window[2]; bp.sample_scale_y = buddha.window[3]; }
        bp.min_iter = buddha.minIter;
        bp.seed = buddha.seed;
        std::vector<uint32_t> planes[3];
        for (uint32_t c = 0; c < channels; c++) {
            bp.max_iter = buddha.nebula ? buddha.nebulaIter[c] : (buddha.maxIter ? buddha.maxIter : bp.max_iter);
            planes[c].resize(npix);
            mc_buddhabrot_stats st;
            mc_buddhabrot_guide_info info;
            uint32_t grid = 0;
            if (buddha.guided) {
                mc_buddhabrot_guide_params gp;
                check(mc_buddhabrot_guide_default_params(&gp), "mc_buddhabrot_guide_default_params");
                if (buddha.guideLog2) gp.grid_log2 = buddha.guideLog2;
                if (buddha.pilotSet) gp.pilot_samples = buddha.pilot;
                if (buddha.dilateSet) gp.dilate = buddha.dilate;
                gp.complement_weight = buddha.unbiased;
                grid = gp.grid_log2;
                check(mc_buddhabrot_render_guided(ctx, &bp, &gp, planes[c].data(), &st, &info), "mc_buddhabrot_render_guided");
            } else {
                check(mc_buddhabrot_render(ctx, &bp, planes[c].data(), &st), "mc_buddhabrot_render");
            }
            double kernel = 0.0;
            (void)mc_context_last_timing(ctx, &kernel, nullptr);
            printf("buddhabrot: max_iter %u, min_iter %u, seed %u: samples %llu, skipped %llu, contributing %llu, points %llu, added %llu (kernel %.3f ms)\n",
                   bp.max_iter, bp.min_iter, bp.seed, (unsigned long long)st.samples, (unsigned long long)st.skipped,
                   (unsigned long long)st.contributing, (unsigned long long)st.points, (unsigned long long)st.added, kernel);
            if (buddha.guided) {
                const unsigned long long all = 1ull << (2u * grid);
                printf("guided: %u of %llu cells (%.2f %%), pilot added %llu of %llu samples", info.n_cells, all,
                       100.0 * (double)info.n_cells / (double)all, (unsigned long long)info.pilot.added, (unsigned long long)info.pilot.samples);
                if (info.complement.samples)
                    printf(", complement %u cells: samples %llu, added %llu at weight %u", info.n_complement,
                           (unsigned long long)info.complement.samples, (unsigned long long)info.complement.added, buddha.unbiased);
                printf("\n");
            }
        }
        constexpr uint32_t kCap = (1u << 20) - 1u;
        std::vector<uint64_t> hist((size_t)kCap + 1, 0);
        for (uint32_t c = 0; c < channels; c++)
            for (uint32_t d : planes[c]) hist[std::min(d, kCap)]++;
        uint64_t nonEmpty = 0;
        for (uint32_t v = 1; v <= kCap; v++) nonEmpty += hist[v];
        uint32_t L = 1;
        if (nonEmpty) {
            const double need = (buddha.whitePct / 100.0) * (double)nonEmpty;
            uint64_t run = 0;
            for (uint32_t v = 1; v <= kCap; v++) {
                run += hist[v];
                if ((double)run >= need) { L = v; break; }
            }
        }
        printf("buddhabrot: white level %u (%g %% of %llu non-empty bins), tone %s\n", L, buddha.whitePct, (unsigned long long)nonEmpty,
               buddha.equalised ? "equalised" : "sqrt");
        std::vector<uint32_t> maps[3];
        for (uint32_t c = 0; c < channels; c++) {
            maps[c].resize((size_t)L + 1);
            if (!buddha.equalised) {
                check(mc_buddhabrot_sqrt_map(L, maps[c].data()), "mc_buddhabrot_sqrt_map");
                continue;
            }
            std::vector<uint32_t> h((size_t)L + 1, 0);
            for (uint32_t d : planes[c]) h[std::min(d, L)]++;
            h[0] = 0;
            check(mc_mandelbrot_equalise_map(L, h.data(), maps[c].data()), "mc_mandelbrot_equalise_map");
        }
        const uint32_t* d[3] = {planes[0].data(), planes[channels > 1 ? 1 : 0].data(), planes[channels > 1 ? 2 : 0].data()};
        const uint32_t* m[3] = {maps[0].data(), maps[channels > 1 ? 1 : 0].data(), maps[channels > 1 ? 2 : 0].data()};
        std::vector<float> staged;   // --gpu-postprocess: the storage buffer was not allocated, only the RGBA8 image
        float* rgba = buffer.data();
        if (gpuPostprocess) { staged.resize(npix * 4); rgba = staged.data(); }
        check(mc_buddhabrot_tonemap(resx, resy, d[0], d[1], d[2], L, m[0], m[1], m[2], rgba), "mc_buddhabrot_tonemap");
        if (gpuPostprocess) check(mc_convert_rgba8(ctx, rgba, resx, resy, 255.0f, 0, rgba8.bytes()), "mc_convert_rgba8");
    }
    Buddhabrot buddha;
    // The image in row bands of kBandRows through mc_mandelbrot_render_banded: band k + 1 is launched on a second stream before band k has
    // finished, and every band is handed to the PNG workers as it arrives.  At K4 (5120 rows: 8 bands) the 50 ms of filter + deflate run
    // beside the 60 ms of rendering instead of after them.  (A blocking render per band was measured first: every band's last tiles then
    // drain on an otherwise empty device — K4's kernels 72 ms instead of 60, profiles/r06_streamed_save_probe_blocking_bands.txt.)
    static constexpr uint32_t kBandRows = 640;
    // Where streaming pays: K4 (7680 x 5120, M = 50 000: 60 ms of rendering beside 50 ms of PNG work) gains 29 ms of 204; K1 (3200 x 2400,
    // M = 1000: a 0.2 ms kernel, 2 ms of copy) LOSES 10 to the second stream's first launch (profiles/r06_streamed_save_probe.txt).  The
    // work bound W x H x M tells the two apart before anything has run; the line sits a decade above K1 and a decade below K4.
    virtual bool worthStreaming() const override { return (double)resx * (double)resy * (double)params.max_iter >= 1e11; }
    static void bandArrived(uint32_t rowsDone, void* self) { static_cast<MandelbrotApp*>(self)->progressive.rowsReady(rowsDone); }
    void runStreamed() {
        constexpr float scaleFactor = 255.0f;   // mandelbrotApp.h:174
        if (gpuPostprocess) progressive.beginOpaqueRgba8(rgba8.bytes(), resx, resy, pngThreads);   // (the device conversion writes alpha 255)
        else progressive.beginStorage(buffer.data(), resx, resy, scaleFactor, pngThreads);
        check(mc_mandelbrot_render_banded(ctx, &params, gpuPostprocess ? nullptr : buffer.data(), gpuPostprocess ? rgba8.bytes() : nullptr,
                                          kBandRows, &MandelbrotApp::bandArrived, this), "mc_mandelbrot_render_banded");
        times.streamedBands = (int)((resy + kBandRows - 1) / kBandRows);
    }
    struct Pixel { float r, g, b, a; };   // mandelbrotApp.h:187-189
    static void split(double d, float& hi, float& lo) { hi = (float)d; lo = (float)(d - (double)hi); }
    uint64_t bufferSize;
    uint32_t resx, resy;
    uint32_t workgroupSize;
    mc_mandelbrot_params params;
    mc_mandelbrot_orbit* orbit = nullptr;
    std::vector<float> distance;   // --colour distance: D of the last render
    std::function<std::string(mc_context*)> orbitFactory;
    uint32_t zoomK = 0, zoomF = 0;   // --zoom K F; 0: a still
    bool zoomCounts = false;         // --zoom-keyframes counts
    uint32_t adaptiveSmoothQ = MC_MANDEL_ADAPTIVE_SMOOTH_THRESHOLD;   // --adaptive-smooth[=Q]
    uint32_t zoomFilter = MC_MANDEL_ZOOM_FILTER_BILINEAR;   // --zoom-filter
    double zoomCx = 0.0, zoomCy = 0.0, zoomSx = 0.0, zoomSy = 0.0;
    std::function<std::string(mc_context*, int)> zoomOrbit;
    uint32_t deviceTables = 0;       // --bla-table device: MC_ORBIT_TABLE_*
};

#endif  // MANDELBROTAPP_H_
