// Buddhabrot, host side: the checks every mc_buddhabrot_* call shares and the host-only entry points (mc_buddhabrot_default_params,
// _density, _importance, _importance_cells, _density_guided, _guide_default_params, _sqrt_map, _tonemap).
// Plain C++17, no HIP header; built with the library's floating-point flags (-ffp-contract=off), since the plane is a result.  The
// arithmetic of a sample is buddhabrot.h's, the text the kernels compile too.
#include <cmath>
#include <cstring>
#include <vector>

#include "buddhabrot.h"

namespace mc {

namespace {

int refuse(const char* who, const char* what) {
    set_error_detail(std::string(who) + ": " + what);
    return MC_ERR_INVALID_ARGUMENT;
}

}  // namespace

int buddhabrot_check(const mc_buddhabrot_params* p, const char* who) {
    if (!p) return refuse(who, "p is NULL");
    if (!p->width) return refuse(who, "width is 0");
    if (!p->height) return refuse(who, "height is 0");
    if ((uint64_t)p->width * p->height > 0xffffffffull) return refuse(who, "width * height exceeds 2^32 - 1");
    if (!p->max_iter) return refuse(who, "max_iter is 0");
    if (p->max_iter > buddha::kMaxIterLimit) return refuse(who, "max_iter exceeds 2^24");
    const struct { double v; bool scale; const char* name; } fields[8] = {
        {p->view_centre_x, false, "view_centre_x"},     {p->view_centre_y, false, "view_centre_y"},
        {p->view_scale_x, true, "view_scale_x"},        {p->view_scale_y, true, "view_scale_y"},
        {p->sample_centre_x, false, "sample_centre_x"}, {p->sample_centre_y, false, "sample_centre_y"},
        {p->sample_scale_x, true, "sample_scale_x"},    {p->sample_scale_y, true, "sample_scale_y"}};
    for (const auto& f : fields) {
        if (!std::isfinite(f.v)) return refuse(who, (std::string(f.name) + " is not finite").c_str());
        if (f.scale && f.v == 0.0) return refuse(who, (std::string(f.name) + " is zero").c_str());
    }
    if (p->sample_end < p->sample_begin) return refuse(who, "sample_end is below sample_begin");
    if (p->sample_end - p->sample_begin > buddha::kMaxSamples) return refuse(who, "sample_end - sample_begin exceeds 2^40 samples in one call");
    if (p->flags & ~(uint32_t)(MC_BUDDHA_KERNEL_PLAIN | MC_BUDDHA_KERNEL_POOLED)) return refuse(who, "flags has unknown bits");
    if ((p->flags & MC_BUDDHA_KERNEL_PLAIN) && (p->flags & MC_BUDDHA_KERNEL_POOLED))
        return refuse(who, "flags names both MC_BUDDHA_KERNEL_PLAIN and MC_BUDDHA_KERNEL_POOLED");
    return MC_OK;
}

int buddhabrot_check_grid(uint32_t grid_log2, const char* who) {
    if (!grid_log2 || grid_log2 > buddha::kMaxGridLog2) return refuse(who, "grid_log2 is outside 1 .. 12");
    return MC_OK;
}

// read_list: `cells` is a host list, every entry is checked against the grid (the async device form cannot: its caller's precondition).
int buddhabrot_check_cell_list(const uint32_t* cells, uint32_t n_cells, uint32_t grid_log2, uint32_t weight, bool read_list,
                               const char* who) {
    if (int rc = buddhabrot_check_grid(grid_log2, who)) return rc;
    if (!cells) return refuse(who, "cells is NULL");
    if (!n_cells) return refuse(who, "n_cells is 0");
    if (!weight) return refuse(who, "weight is 0");
    if (read_list) {
        const uint32_t count = 1u << (2u * grid_log2);
        for (uint32_t j = 0; j < n_cells; j++)
            if (cells[j] >= count) return refuse(who, "a cell index is outside the grid (at least G * G)");
    }
    return MC_OK;
}

int buddhabrot_check_guide(const mc_buddhabrot_guide_params* guide, const char* who) {
    if (!guide) return refuse(who, "guide is NULL");
    if (int rc = buddhabrot_check_grid(guide->grid_log2, who)) return rc;
    if (guide->pilot_samples > buddha::kMaxSamples) return refuse(who, "pilot_samples exceeds 2^40");
    if (!guide->threshold) return refuse(who, "threshold is 0");
    if (guide->dilate > buddha::kMaxDilate) return refuse(who, "dilate exceeds 8");
    return MC_OK;
}

namespace {

// The host calls' one body: the samples of a's range, uniform or (gd.cells) guided, into plane (unless null) at gd.weight per point,
// into the map (unless null) and into st.
void host_samples(const buddha::Args& a, const buddha::Guide& gd, uint32_t* plane, uint64_t (&st)[buddha::kStats]) {
    for (uint64_t k = a.begin; k < a.end; k++) {
        st[buddha::kSamples]++;
        uint32_t ux, uy;
        buddha::hash_words(a.seed, k, ux, uy);
        if (gd.cells) buddha::guided_words(gd.cells[k % gd.n_cells], gd.g, ux, uy);
        double cx, cy;
        buddha::c_of_words(a, ux, uy, cx, cy);
        if (buddha::interior(cx, cy)) {
            st[buddha::kSkipped]++;
            continue;
        }
        buddha::Orbit o;
        o.reset();
        uint32_t n = 0;
        bool escaped = false;
        for (uint32_t i = 0; i < a.max_iter; i++)
            if (o.advance(cx, cy) > 4.0) {
                n = i;
                escaped = true;
                break;
            }
        if (!escaped || n < a.min_iter) continue;
        st[buddha::kContributing]++;
        st[buddha::kPoints] += n;
        o.reset();
        uint32_t added = 0;
        for (uint32_t i = 0; i < n; i++) {
            o.advance(cx, cy);
            uint32_t bin;
            if (buddha::bin_of(a, o.zx, o.zy, bin)) {
                if (plane) plane[bin] += gd.weight;   // (wraps modulo 2^32)
                added++;
            }
        }
        st[buddha::kAdded] += added;
        if (gd.map && added) gd.map[buddha::cell_of(ux, uy, gd.g)] += added;   // (wraps too)
    }
}

void add_stats(mc_buddhabrot_stats* stats, const uint64_t (&st)[buddha::kStats]) {
    if (!stats) return;
    stats->samples += st[buddha::kSamples];
    stats->skipped += st[buddha::kSkipped];
    stats->contributing += st[buddha::kContributing];
    stats->points += st[buddha::kPoints];
    stats->added += st[buddha::kAdded];
}

}  // namespace

int buddhabrot_check_levels(uint32_t levels, const char* who) {
    if (!levels || levels > buddha::kMaxLevels) return refuse(who, "levels is outside 1 .. 2^20");
    return MC_OK;
}

int buddhabrot_check_maps(uint32_t levels, const uint32_t* m0, const uint32_t* m1, const uint32_t* m2, const char* who) {
    const uint32_t* maps[3] = {m0, m1, m2};
    for (int c = 0; c < 3; c++) {
        if (c && maps[c] == maps[c - 1]) continue;   // (grey: one map three times is checked once)
        for (uint32_t j = 0; j <= levels; j++)
            if (maps[c][j] > levels) return refuse(who, "a map entry exceeds levels");
    }
    return MC_OK;
}

void buddhabrot_tone_table(uint32_t levels, const uint32_t* m0, const uint32_t* m1, const uint32_t* m2, float* table) {
    const uint32_t* maps[3] = {m0, m1, m2};
    const size_t entries = (size_t)levels + 1;
    const float lf = (float)levels;
    for (int c = 0; c < 3; c++)
        for (size_t j = 0; j < entries; j++) table[c * entries + j] = (float)maps[c][j] / lf;
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_buddhabrot_default_params(uint32_t width, uint32_t height, uint64_t samples, mc_buddhabrot_params* out) {
    if (!out) {
        set_error_detail("mc_buddhabrot_default_params: out is NULL");
        return MC_ERR_INVALID_ARGUMENT;
    }
    std::memset(out, 0, sizeof(*out));
    out->view_centre_x = -0.5; out->view_centre_y = 0.0;
    out->view_scale_x = 3.0;
    out->view_scale_y = width ? (3.0 * (double)height) / (double)width : 3.0;
    out->sample_centre_x = -0.5; out->sample_centre_y = 0.0;
    out->sample_scale_x = 4.0; out->sample_scale_y = 4.0;
    out->sample_begin = 0; out->sample_end = samples;
    out->width = width; out->height = height;
    out->max_iter = 1000; out->min_iter = 0;
    out->seed = 1; out->flags = 0;
    return MC_OK;
}

int mc_buddhabrot_density(const mc_buddhabrot_params* p, uint32_t* plane, mc_buddhabrot_stats* stats) {
    const char* who = "mc_buddhabrot_density";
    if (int rc = buddhabrot_check(p, who)) return rc;
    if (!plane) {
        set_error_detail(std::string(who) + ": plane is NULL");
        return MC_ERR_INVALID_ARGUMENT;
    }
    buddha::Guide gd{};
    gd.weight = 1u;
    uint64_t st[buddha::kStats] = {0, 0, 0, 0, 0};
    host_samples(buddha::make_args(p), gd, plane, st);
    add_stats(stats, st);
    return MC_OK;
}

int mc_buddhabrot_importance(const mc_buddhabrot_params* p, uint32_t grid_log2, uint32_t* map, uint32_t* plane,
                             mc_buddhabrot_stats* stats) {
    const char* who = "mc_buddhabrot_importance";
    if (int rc = buddhabrot_check(p, who)) return rc;
    if (int rc = buddhabrot_check_grid(grid_log2, who)) return rc;
    if (!map) return refuse(who, "map is NULL");
    buddha::Guide gd{};
    gd.map = map;
    gd.g = grid_log2;
    gd.weight = 1u;
    uint64_t st[buddha::kStats] = {0, 0, 0, 0, 0};
    host_samples(buddha::make_args(p), gd, plane, st);
    add_stats(stats, st);
    return MC_OK;
}

int mc_buddhabrot_importance_cells(uint32_t grid_log2, const uint32_t* map, uint32_t threshold, uint32_t dilate, uint32_t flags,
                                   uint32_t* cells_out, uint32_t* n_cells) {
    const char* who = "mc_buddhabrot_importance_cells";
    if (int rc = buddhabrot_check_grid(grid_log2, who)) return rc;
    if (!map) return refuse(who, "map is NULL");
    if (!n_cells) return refuse(who, "n_cells is NULL");
    if (!threshold) return refuse(who, "threshold is 0");
    if (dilate > buddha::kMaxDilate) return refuse(who, "dilate exceeds 8");
    if (flags & ~(uint32_t)MC_BUDDHA_CELLS_COMPLEMENT) return refuse(who, "flags has unknown bits");
    const size_t G = (size_t)1 << grid_log2;
    std::vector<uint8_t> in(G * G), row(G * G);
    for (size_t c = 0; c < G * G; c++) in[c] = map[c] >= threshold;
    // one ring of the 8-neighbourhood = the 3-wide maximum along the rows, then along the columns, clipped at the edges
    for (uint32_t ring = 0; ring < dilate; ring++) {
        for (size_t y = 0; y < G; y++)
            for (size_t x = 0; x < G; x++)
                row[y * G + x] = in[y * G + x] | (x ? in[y * G + x - 1] : 0) | (x + 1 < G ? in[y * G + x + 1] : 0);
        for (size_t y = 0; y < G; y++)
            for (size_t x = 0; x < G; x++)
                in[y * G + x] = row[y * G + x] | (y ? row[(y - 1) * G + x] : 0) | (y + 1 < G ? row[(y + 1) * G + x] : 0);
    }
    const uint8_t want = (flags & MC_BUDDHA_CELLS_COMPLEMENT) ? 0 : 1;
    uint32_t n = 0;
    for (size_t c = 0; c < G * G; c++)
        if (in[c] == want) {
            if (cells_out) cells_out[n] = (uint32_t)c;
            n++;
        }
    *n_cells = n;
    return MC_OK;
}

int mc_buddhabrot_density_guided(const mc_buddhabrot_params* p, const uint32_t* cells, uint32_t n_cells, uint32_t grid_log2,
                                 uint32_t weight, uint32_t* plane, mc_buddhabrot_stats* stats) {
    const char* who = "mc_buddhabrot_density_guided";
    if (int rc = buddhabrot_check(p, who)) return rc;
    if (int rc = buddhabrot_check_cell_list(cells, n_cells, grid_log2, weight, true, who)) return rc;
    if (!plane) return refuse(who, "plane is NULL");
    buddha::Guide gd{};
    gd.cells = cells;
    gd.n_cells = n_cells;
    gd.g = grid_log2;
    gd.weight = weight;
    uint64_t st[buddha::kStats] = {0, 0, 0, 0, 0};
    host_samples(buddha::make_args(p), gd, plane, st);
    add_stats(stats, st);
    return MC_OK;
}

int mc_buddhabrot_guide_default_params(mc_buddhabrot_guide_params* out) {
    if (!out) return refuse("mc_buddhabrot_guide_default_params", "out is NULL");
    std::memset(out, 0, sizeof(*out));
    out->grid_log2 = 8;
    out->pilot_samples = 1ull << 24;
    out->threshold = 1;
    out->dilate = 1;
    out->complement_weight = 0;
    return MC_OK;
}

int mc_buddhabrot_sqrt_map(uint32_t levels, uint32_t* map) {
    const char* who = "mc_buddhabrot_sqrt_map";
    if (int rc = buddhabrot_check_levels(levels, who)) return rc;
    if (!map) {
        set_error_detail(std::string(who) + ": map is NULL");
        return MC_ERR_INVALID_ARGUMENT;
    }
    const double lf = (double)levels;
    for (uint32_t j = 0; j <= levels; j++) {
        const uint32_t v = (uint32_t)(lf * std::sqrt((double)j / lf));
        map[j] = v > levels ? levels : v;
    }
    return MC_OK;
}

int mc_buddhabrot_tonemap(uint32_t width, uint32_t height, const uint32_t* d0, const uint32_t* d1, const uint32_t* d2, uint32_t levels,
                          const uint32_t* m0, const uint32_t* m1, const uint32_t* m2, float* out) {
    const char* who = "mc_buddhabrot_tonemap";
    if (!d0 || !d1 || !d2 || !m0 || !m1 || !m2 || !out) {
        set_error_detail(std::string(who) + ": a pointer is NULL");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (!width || !height || (uint64_t)width * height > 0xffffffffull) {
        set_error_detail(std::string(who) + ": width or height is 0, or width * height exceeds 2^32 - 1");
        return MC_ERR_INVALID_ARGUMENT;
    }
    if (int rc = buddhabrot_check_levels(levels, who)) return rc;
    if (int rc = buddhabrot_check_maps(levels, m0, m1, m2, who)) return rc;
    const uint32_t* planes[3] = {d0, d1, d2};
    const uint32_t* maps[3] = {m0, m1, m2};
    const float lf = (float)levels;
    const size_t npix = (size_t)width * height;
    for (size_t i = 0; i < npix; i++) {
        for (int c = 0; c < 3; c++) {
            const uint32_t d = planes[c][i];
            out[4 * i + c] = (float)maps[c][d > levels ? levels : d] / lf;
        }
        out[4 * i + 3] = 1.0f;
    }
    return MC_OK;
}

}  // extern "C"
