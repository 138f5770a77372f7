// PathtracerApp — mirrors src/pathtracerApp.h:42-397 of the reference on top of ComputeApp.
#ifndef PATHTRACERAPP_H_
#define PATHTRACERAPP_H_

#include <cstdio>
#include <cstring>
#include <string>

#include "computeApp.h"
#include "pngWriter.h"

struct PathtracerApp : public ComputeApp {
    struct pushConst_t {          // pathtracerApp.h:44-47
        uint32_t imgdim[2];       // { WIDTH, HEIGHT }
        uint32_t samps[2];        // { 0, spp }
    } pushConst;

    // Same signature as the reference (pathtracerApp.h:49); `quiet` (main.cpp --quiet) only silences the constructor's
    // "in PathtracerApp ctor" line, which the reference always prints.
    PathtracerApp(const uint32_t resx, const uint32_t resy, const int32_t spp, const uint32_t workgroupSize = 16,
                  const bool quiet = false) {
        setQuiet(quiet);
        this->resx = resx;
        this->resy = resy;
        this->spp = spp;
        this->workgroupSize = workgroupSize;
        bufferSize = (uint64_t)sizeof(Pixel) * resx * resy;
        if (!quiet) printf("in PathtracerApp ctor\n");
        pushConst.imgdim[0] = resx;
        pushConst.imgdim[1] = resy;
        pushConst.samps[0] = 0;
        pushConst.samps[1] = (uint32_t)spp;
        mc_pathtrace_default_params(resx, resy, (uint32_t)spp, &params);
        const float *pl, *sp; uint32_t np, ns;
        mc_pathtrace_default_scene(&pl, &np, &sp, &ns);   // the tables of pathtracerApp.h:14-39
        planes.assign(pl, pl + 12 * np);
        spheres.assign(sp, sp + 12 * ns);
    }

    // -- additions --
    void setMathMode(uint32_t mode) { params.math_mode = mode; }   // MC_PT_MATH_STRICT / MC_PT_MATH_FAST / MC_PT_MATH_FAST_CAREFUL
    // The reference's precision experiment (pathtracerApp.h:11, emulateDouble.h.glsl:13-26), a run-time switch here:
    // which sphere-test branch of pathTracer.comp:132-256 is active, and the sphere-walled scene of :28-35.
    void setSpherePrecision(uint32_t prec) { params.flags = (params.flags & ~MC_PT_PRECISION(0xf)) | MC_PT_PRECISION(prec); }
    void useLargeSphereWalls() {
        static const float dummyPlane[12] = {1, 0, 0, 1000, 0, 0, 0, 0, 1, 1, 1, 1};   // "must have at least one plane" (:22-23)
        static const float walls[6 * 12] = {
            (float)(1e5 - 2.6), 0, 0, (float)1e5, 0, 0, 0, 0, (float).85, (float).25, (float).25, 1,    // Left
            (float)(1e5 + 2.6), 0, 0, (float)1e5, 0, 0, 0, 0, (float).25, (float).35, (float).85, 1,    // Right
            0, (float)(1e5 + 2), 0, (float)1e5, 0, 0, 0, 0, (float).75, (float).75, (float).75, 1,      // Top
            0, (float)(-1e5 - 2), 0, (float)1e5, 0, 0, 0, 0, (float).75, (float).75, (float).75, 1,     // Bottom
            0, 0, (float)(-1e5 - 2.8), (float)1e5, 0, 0, 0, 0, (float).85, (float).85, (float).25, 1,   // Back
            0, 0, (float)(1e5 + 7.9), (float)1e5, 0, 0, 0, 0, (float)0.1, (float)0.7, (float)0.7, 1,    // Front
        };
        std::vector<float> sp(walls, walls + 72);
        sp.insert(sp.end(), spheres.begin(), spheres.end());   // then mirror, glass, light (:36-38)
        planes.assign(dummyPlane, dummyPlane + 12);
        spheres.swap(sp);
    }
    // --denoise [P]: run() renders, makes the guide planes and filters on the device (mc_pathtrace_render_denoised) with the default
    // weights and P passes; 0 = off, and then run() is what it was.  One GPU (main.cpp refuses --gpus above 1).
    void setDenoise(uint32_t passes) { denoisePasses = passes; }
    // --noise-guided [K]: the denoised run() takes its colour tolerance from a measured noise plane (mc_pathtrace_render_denoised_adaptive)
    // with k_noise = K and the default radius; 0 = off.
    void setNoiseGuided(float k) { noiseK = k; }
    // --budget [L] [--noise-target T]: run() is mc_pathtrace_render_budgeted — a pilot of spp samples, then up to L doublings where the measured
    // noise is above T — with the default radius.  One GPU, no --denoise (main.cpp refuses those); with --accel bvh the accelerated chain.
    void setBudget(const mc_pathtrace_budget_params& b) { budget = b; budgeted = true; }
    // "budget: <pixels of level 0 .. L> mean <m> spp" (mc_context_last_budget), after run()
    void printBudget() const {
        uint64_t per[9];
        double mean = 0.0;
        if (mc_context_last_budget(ctx, per, &mean) != MC_OK) return;
        printf("budget:");
        for (uint32_t l = 0; l <= budget.max_level; l++) printf(" %llu", (unsigned long long)per[l]);
        printf(" mean %.4f spp\n", mean);
    }
    void setScene(const float* pl, uint32_t np, const float* sp, uint32_t ns) {
        planes.assign(pl, pl + 12 * np);
        spheres.assign(sp, sp + 12 * ns);
    }

    // --scene FILE: a text file, one object per line, `plane` or `sphere` followed by the record's 12 floats (equation.xyzw or
    // centre.xyz radius | emission.xyz 0 | colour.rgb material); blank lines and lines starting with # are skipped.  Returns "" or what is wrong.
    std::string loadScene(const char* path) {
        FILE* f = std::fopen(path, "r");
        if (!f) return "cannot open the file";
        std::vector<float> pl, sp;
        char line[1024];
        int lineNo = 0;
        std::string err;
        while (err.empty() && std::fgets(line, sizeof line, f)) {
            lineNo++;
            char kind[16] = {0};
            float v[12];
            int used = 0;
            if (std::sscanf(line, " %15s%n", kind, &used) != 1 || kind[0] == '#') continue;
            const bool plane = std::strcmp(kind, "plane") == 0;
            if (!plane && std::strcmp(kind, "sphere") != 0) { err = "line " + std::to_string(lineNo) + ": neither `plane` nor `sphere`"; break; }
            const char* at = line + used;
            int k = 0;
            for (; k < 12; k++) {
                char* end = nullptr;
                v[k] = std::strtof(at, &end);
                if (end == at) break;
                at = end;
            }
            while (*at == ' ' || *at == '\t' || *at == '\r' || *at == '\n') at++;
            if (k != 12 || *at) { err = "line " + std::to_string(lineNo) + ": 12 numbers expected after `" + kind + "`"; break; }
            (plane ? pl : sp).insert((plane ? pl : sp).end(), v, v + 12);
        }
        std::fclose(f);
        if (!err.empty()) return err;
        if ((pl.size() + sp.size()) / 12 > (1u << 20)) return "more than 2^20 objects";
        planes.swap(pl);
        spheres.swap(sp);
        return "";
    }
    // --accel bvh: run() renders through mc_pathtrace_render_accel* — the plain render, or with --denoise --noise-guided / --budget the
    // accelerated noise-guided / budgeted chain (one GPU, no plain --denoise: main.cpp refuses those).  The tree is built here, on the
    // host.  Returns "" or the library's refusal.
    std::string useAccel() {
        const int rc = mc_pathtrace_accel_create(planes.data(), (uint32_t)planes.size() / 12, spheres.data(), (uint32_t)spheres.size() / 12, &accel);
        if (rc != MC_OK) return std::string(mc_error_string(rc)) + " (" + mc_last_error_detail() + ")";
        return "";
    }

    virtual void preRun() override {
        if (!quiet) { printf(" * before createBuffer()\n"); fflush(stdout); }
        createBuffer(bufferSize);   // output buffer; the two scene SSBOs of the reference (pathtracerApp.h:129-198)
                                    // become kernel arguments, there is nothing to upload here
    }

    // The reference records spp dispatches, one push-constant update each, with no barrier in between
    // (pathtracerApp.h:361-376).  Here the whole samps.x range [0,spp) is ONE launch with the sample
    // loop fused in registers, accumulating in the barrier-serialised order s = 0..spp-1.
    mc_pathtrace_params request() const {
        mc_pathtrace_params q = params;
        q.width = pushConst.imgdim[0]; q.height = pushConst.imgdim[1];
        q.spp = pushConst.samps[1];
        q.sample_begin = 0; q.sample_end = pushConst.samps[1];
        q.row_begin = 0; q.row_end = resy;
        return q;
    }
    virtual void createCommandBuffer() override {
        if (!quiet) { printf("\n   ### recording fused spp loop: samples [0,%d) ###\n\n", spp); fflush(stdout); }
        params = request();
    }

    virtual std::function<int()> warmupCall() const override {   // what run() is going to ask for (the setters were called before init())
        if (accel) return [] { return (int)MC_OK; };   // (the plain calls' warm-up would load the linear kernels and upload the tables for nothing)
        return [ctx = ctx, q = request(), planes = planes, spheres = spheres, rgba8 = gpuPostprocess ? 1 : 0] {
            return mc_context_warmup_pathtrace(ctx, &q, planes.data(), (uint32_t)planes.size() / 12, spheres.data(),
                                               (uint32_t)spheres.size() / 12, rgba8);
        };
    }

    virtual void runCommandBuffer() override {
        const uint32_t np = (uint32_t)planes.size() / 12, ns = (uint32_t)spheres.size() / 12;
        if (accel) {
            float* f32 = gpuPostprocess ? nullptr : buffer.data();   // both routes, as the table forms below
            uint8_t* u8 = gpuPostprocess ? rgba8.bytes() : nullptr;
            if (budgeted) {
                check(mc_pathtrace_render_accel_budgeted(ctx, accel, &params, &budget, f32, u8, nullptr), "mc_pathtrace_render_accel_budgeted");
                return;
            }
            if (denoisePasses) {   // (main.cpp lets only the noise-guided chain through)
                mc_pathtrace_denoise_params d;
                mc_pathtrace_denoise_default_params(params.width, params.height, &d);
                d.passes = denoisePasses;
                float k = 0.0f;
                uint32_t radius = 0;
                mc_pathtrace_noise_default_params(&k, &radius);
                check(mc_pathtrace_render_accel_denoised_adaptive(ctx, accel, &params, &d, noiseK, radius, f32, u8),
                      "mc_pathtrace_render_accel_denoised_adaptive");
                return;
            }
            if (gpuPostprocess) check(mc_pathtrace_render_accel_rgba8(ctx, accel, &params, rgba8.bytes()), "mc_pathtrace_render_accel_rgba8");
            else check(mc_pathtrace_render_accel(ctx, accel, &params, buffer.data()), "mc_pathtrace_render_accel");
            return;
        }
        if (budgeted) {   // both routes, as the denoised calls
            check(mc_pathtrace_render_budgeted(ctx, &params, &budget, planes.data(), np, spheres.data(), ns, gpuPostprocess ? nullptr : buffer.data(),
                                               gpuPostprocess ? rgba8.bytes() : nullptr, nullptr),
                  "mc_pathtrace_render_budgeted");
            return;
        }
        if (denoisePasses) {   // both routes: the storage buffer, or (--gpu-postprocess) the RGBA8 image converted and rotated on the device
            mc_pathtrace_denoise_params d;
            mc_pathtrace_denoise_default_params(params.width, params.height, &d);
            d.passes = denoisePasses;
            if (noiseK > 0.0f) {
                float k = 0.0f;
                uint32_t radius = 0;
                mc_pathtrace_noise_default_params(&k, &radius);
                check(mc_pathtrace_render_denoised_adaptive(ctx, &params, &d, noiseK, radius, planes.data(), np, spheres.data(), ns,
                                                            gpuPostprocess ? nullptr : buffer.data(), gpuPostprocess ? rgba8.bytes() : nullptr),
                      "mc_pathtrace_render_denoised_adaptive");
                return;
            }
            check(mc_pathtrace_render_denoised(ctx, &params, &d, planes.data(), np, spheres.data(), ns, gpuPostprocess ? nullptr : buffer.data(),
                                               gpuPostprocess ? rgba8.bytes() : nullptr),
                  "mc_pathtrace_render_denoised");
            return;
        }
        if (gpuPostprocess) {   // render + float->u8 + 180-degree rotation on the device (pathtracerApp.h:202-243), 4 B/pixel copied
            if (multi) check(mc_multi_pathtrace_render_rgba8(multi, &params, planes.data(), np, spheres.data(), ns, rgba8.bytes()),
                             "mc_multi_pathtrace_render_rgba8");
            else check(mc_pathtrace_render_rgba8(ctx, &params, planes.data(), np, spheres.data(), ns, rgba8.bytes()),
                       "mc_pathtrace_render_rgba8");
            return;
        }
        if (multi) check(mc_multi_pathtrace_render(multi, &params, planes.data(), np, spheres.data(), ns, buffer.data()),
                         "mc_multi_pathtrace_render");
        else check(mc_pathtrace_render(ctx, &params, planes.data(), np, spheres.data(), ns, buffer.data()), "mc_pathtrace_render");
    }

    // pathtracerApp.h:202-223
    void getRenderedImage(std::vector<uint8_t>& image, const uint32_t resx, const uint32_t resy, float floatScaleFactor) {
        convertStorage(image, resx, resy, floatScaleFactor, false);   // the loop of :212-219, row stripes in parallel
    }

    virtual void saveRenderedImage(const char* png_filename = "pathtracer.png") override {
        // pathtracerApp.h:225-247: scale 1, then — the pinhole camera's image is upside-down and mirrored — every pixel of the left half
        // swapped with its point reflection (:235-243), applied while converting: the same bytes, incl. an odd width's middle column
        saveImage(png_filename, resx, resy, 1.0f, true, false);
    }

    const HostStorage& storageBuffer() const { return buffer; }

private:
    struct Pixel { float r, g, b, a; };
    uint64_t bufferSize;
    uint32_t resx, resy;
    int32_t spp;
    uint32_t workgroupSize;
    mc_pathtrace_params params;
    uint32_t denoisePasses = 0;
    float noiseK = 0.0f;
    bool budgeted = false;
    mc_pathtrace_budget_params budget = {0, 0.0f, 0, 0};
    mc_pathtrace_accel* accel = nullptr;   // --accel bvh (lives as long as the process: the app leaves through _Exit or its destructor-free end)
    std::vector<float> planes, spheres;
};

#endif  // PATHTRACERAPP_H_
