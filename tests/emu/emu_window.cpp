// emu_window.cpp — TEST-ONLY CPU emulation of the window kernel (csrc/window_band.hpp): the product's planner and every workgroup
// of the launch grid, phase by phase.  Built by tests/test_window_emulation.py (g++, the flags of tests/emu/Makefile).
#include "hip_shim.hpp"
#include <string>
#include <vector>
#include "../../jpeg-decoder_amd/csrc/host_common.hpp"
#include "../../jpeg-decoder_amd/csrc/window_band.hpp"

using namespace jpgpu;

static int plan(const jpgpu_image_desc *desc, const uint32_t win[4], uint8_t *out, ImageJob &job, WindowGeom &g, size_t *len, char *why, size_t why_cap) {
    size_t out_len = 0;
    std::string err;
    uint8_t *no_planes[4] = {nullptr, nullptr, nullptr, nullptr};
    int rc = build_image_job(desc->components, desc->ncomp, no_planes, desc->out_w, desc->out_h, desc->color_transform, out, job, out_len, err);
    if (rc) return rc;
    const char *reason = "";
    if (!window_geom_from_job(desc->components, desc->ncomp, job, win[0], win[1], win[2], win[3], g, reason)) {
        if (why && why_cap) snprintf(why, why_cap, "%s", reason);
        return -1;
    }
    if (len) *len = (size_t)win[2] * win[3] * desc->ncomp;
    return 0;
}

extern "C" {
// The planner alone: the WindowGeom as uint32 words (geom_words: capacity in words).  Returns -1 if it refused the window, else the
// status of build_image_job.
int emu_window_plan(const jpgpu_image_desc *desc, const uint32_t *win, uint32_t *geom, uint32_t geom_words, char *why, size_t why_cap) {
    ImageJob job;
    WindowGeom g;
    int rc = plan(desc, win, nullptr, job, g, nullptr, why, why_cap);
    if (rc) return rc;
    const size_t n = sizeof(WindowGeom) / 4 < geom_words ? sizeof(WindowGeom) / 4 : geom_words;
    memcpy(geom, &g, n * 4);
    return 0;
}
// The block rectangle of component `comp` that tile (tile, band) transforms, ring included: rect = {bx0, by0, bx1, by1}.
int emu_window_tile_blocks(const jpgpu_image_desc *desc, const uint32_t *win, uint32_t tile, uint32_t band, uint32_t comp, int32_t *rect) {
    ImageJob job;
    WindowGeom g;
    int rc = plan(desc, win, nullptr, job, g, nullptr, nullptr, 0);
    if (rc) return rc;
    window_tile_blocks(g, comp, tile, band, rect[0], rect[1], rect[2], rect[3]);
    return 0;
}
// The window kernel over the whole launch grid: `out` receives the window's bytes (*len of them).
int emu_window_decode(const jpgpu_image_desc *desc, const int16_t *const *coefs, const uint32_t *win, uint8_t *out, size_t *len) {
    ImageJob job;
    WindowGeom g;
    int rc = plan(desc, win, out, job, g, len, nullptr, 0);
    if (rc) return rc;
    PlaneJob pj[4];
    memset(pj, 0, sizeof(pj));
    for (uint32_t c = 0; c < desc->ncomp; c++) {
        pj[c].coefs = coefs[c];
        pj[c].qt = desc->quantization_tables[c];
        pj[c].block_w = desc->components[c].block_width;
        pj[c].n_blocks = (uint32_t)desc->components[c].block_width * desc->components[c].block_height;
        pj[c].scale = desc->components[c].dct_scale;
    }
    std::vector<uint8_t> lds(g.lds_bytes + 64);
    for (uint32_t band = 0; band < g.bands; band++)
        for (uint32_t tile = 0; tile < g.tiles_x; tile++) {
            memset(lds.data(), 0xCD, lds.size());  // garbage, like real LDS
#define RUNW(S)                                                                                      \
    {                                                                                                \
        for (uint32_t t = 0; t < WB_NT; t++) WBand<S>::transform(g, pj, tile, band, t, lds.data());  \
        for (uint32_t t = 0; t < WB_NT; t++) WBand<S>::pixels(g, job, tile, band, t, lds.data());    \
    }
            if (g.scale == 8) RUNW(8) else if (g.scale == 4) RUNW(4) else if (g.scale == 2) RUNW(2) else RUNW(1)
#undef RUNW
        }
    return 0;
}
}
