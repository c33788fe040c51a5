// emu_batch_output.cpp — TEST-ONLY: the fixed-output stage of a batch as csrc/batch_output.hpp states it — the options record, the rules,
// the placement normalisation, the bytes per image and the route — on the CPU.  Built by tests/test_batch_output.py (g++, the flags of
// tests/emu/Makefile); batch_output_asan.cpp runs the same functions as a stand-alone program under the sanitizers.
#include "hip_shim.hpp"
#include <string>
#include <vector>
#include "../../jpeg-decoder_amd/csrc/batch_output.hpp"

using namespace jpgpu;

extern "C" {
// OutputSpec with plain fields (ctypes mirrors it: tests/test_batch_output.py)
struct EmuSpec {
    uint32_t w, h, filter, rgb, tensor;
    jpgpu_tensor_format tn;
    uint8_t fill[4];
    uint32_t warp;
    jpgpu_warp_options wp;
};
}

static OutputSpec spec_of(const EmuSpec &e) {
    OutputSpec s;
    s.w = e.w, s.h = e.h, s.filter = e.filter, s.rgb = e.rgb != 0, s.tensor = e.tensor != 0, s.tn = e.tn, s.warp = e.warp != 0, s.wp = e.wp;
    memcpy(s.fill, e.fill, 4);
    return s;
}

extern "C" {
uint32_t emu_cc_none() { return CC_NONE; }
uint32_t emu_rs_max_out() { return RS_MAX_OUT; }

int emu_output_rule(const EmuSpec *e, char *why, uint32_t cap) {
    std::string text;
    const int rc = output_rule(spec_of(*e), text);
    snprintf(why, cap, "%s", text.c_str());
    return rc;
}
int emu_output_image_rule(const EmuSpec *e, uint32_t ncomp, uint32_t color_fn, char *why, uint32_t cap) {
    std::string text;
    const int rc = output_image_rule(spec_of(*e), ncomp, color_fn, text);
    snprintf(why, cap, "%s", text.c_str());
    return rc;
}
int emu_spec_equal(const EmuSpec *a, const EmuSpec *b) { return spec_of(*a) == spec_of(*b) ? 1 : 0; }
// What a default-constructed OutputSpec compares equal to: every option absent
int emu_spec_is_default(const EmuSpec *a) { return spec_of(*a) == OutputSpec{} ? 1 : 0; }

// out: n placements; returns n, or the first image that shows no pixel
uint32_t emu_normalise_placements(const jpgpu_placement *pls, uint32_t n, uint32_t w, uint32_t h, jpgpu_placement *out, uint32_t *placed) {
    std::vector<jpgpu_placement> norm;
    bool any = false;
    const uint32_t k = normalise_placements(pls, n, w, h, norm, any);
    for (uint32_t i = 0; i < n; i++) out[i] = norm[i];
    *placed = any;
    return k;
}
// placed_axis (csrc/placed_band.hpp): out3 = {first, count, v0}; returns whether the axis shows a pixel
int emu_placed_axis(uint32_t r, int32_t at, uint32_t out, uint32_t *out3) { return placed_axis(r, at, out, out3[0], out3[1], out3[2]) ? 1 : 0; }

size_t emu_output_image_bytes(const EmuSpec *e, uint32_t ncomp, int u8) { return output_image_bytes(spec_of(*e), ncomp, u8 != 0); }
size_t emu_output_arena(const EmuSpec *e, const uint32_t *ncomps, uint32_t n, int u8, size_t *off, size_t *len) {
    std::vector<jpgpu_image_desc> descs(n);
    for (uint32_t i = 0; i < n; i++) descs[i].ncomp = ncomps[i];
    std::vector<size_t> o, l;
    const size_t bytes = output_arena(spec_of(*e), descs, u8 != 0, o, l);
    for (uint32_t i = 0; i < n; i++) off[i] = o[i], len[i] = l[i];
    return bytes;
}

// out4 = {resample (0 none, 1 band, 2 tensor, 3 placed, 4 placed tensor), runs, warp, tensor_jobs}
void emu_output_route(const EmuSpec *e, int placed, uint32_t max_runs, uint32_t *out4) {
    const OutputRoute r = output_route(spec_of(*e), placed != 0, max_runs);
    out4[0] = (uint32_t)r.resample, out4[1] = r.runs, out4[2] = r.warp, out4[3] = r.tensor_jobs();
}
}
