// emu_batch_layout.cpp — TEST-ONLY: the window rule, the output layout and the headroom rule of a batch (csrc/batch_layout.hpp) on the
// CPU, and a window group planned and rewindowed with them the way batch_create and batch_rewindow (csrc/batch.cpp) do it.
// Built by tests/test_batch_layout.py (g++, the flags of tests/emu/Makefile).
#include "hip_shim.hpp"
#include <string>
#include <vector>
#include "../../jpeg-decoder_amd/csrc/batch_layout.hpp"

using namespace jpgpu;

namespace {
struct Plan {  // what a batch keeps of its window group and its output arena
    std::vector<jpgpu_image_desc> descs;
    std::vector<uint32_t> ids;
    std::vector<WindowGeom> geoms;
    std::vector<size_t> full_len, off, len;
    size_t bytes = 0;
    void number() {  // (BandGroup::set_geoms)
        uint32_t pj = 0;
        for (size_t k = 0; k < ids.size(); k++) geoms[k].first_plane_job = pj, pj += descs[ids[k]].ncomp;
    }
};
}  // namespace

extern "C" {
uint32_t emu_window_geom_words() { return (uint32_t)(sizeof(WindowGeom) / 4); }

// out = {windowed, gw, gh}; the reason text in `why`
int emu_window_rule(const jpgpu_image_desc *d, const jpgpu_window *wn, uint32_t *out, char *why, uint32_t why_cap) {
    bool windowed = false;
    WindowGeom wg;
    std::string text;
    const int rc = window_rule(*d, *wn, windowed, out[1], out[2], wg, text);
    out[0] = windowed;
    snprintf(why, why_cap, "%s", text.c_str());
    return rc;
}

size_t emu_arena_layout(const size_t *lens, uint32_t n, size_t *off, size_t *len) {
    std::vector<size_t> o, l;
    const size_t bytes = arena_layout(std::vector<size_t>(lens, lens + n), o, l);
    for (uint32_t i = 0; i < n; i++) off[i] = o[i], len[i] = l[i];
    return bytes;
}
size_t emu_arena_headroom(size_t need, size_t full) { return arena_headroom(need, full); }

// batch_create's part: the rule per image, the group in image order, the layout.  *status: the rule's or build_image_job's.
void *emu_plan_create(const jpgpu_image_desc *descs, const jpgpu_window *windows, uint32_t n, int *status) {
    Plan *p = new Plan();
    p->descs.assign(descs, descs + n);
    p->full_len.assign(n, 0);
    std::vector<size_t> lens(n, 0);
    *status = JPGPU_OK;
    for (uint32_t i = 0; i < n && *status == JPGPU_OK; i++) {
        uint8_t *dummy[4] = {nullptr, nullptr, nullptr, nullptr};
        ImageJob ij;
        std::string why;
        if ((*status = build_image_job(descs[i].components, descs[i].ncomp, dummy, descs[i].out_w, descs[i].out_h, descs[i].color_transform, nullptr, ij, lens[i], why))) break;
        p->full_len[i] = lens[i];
        bool windowed = false;
        uint32_t gw = 0, gh = 0;
        WindowGeom wg;
        if ((*status = window_rule(descs[i], windows[i], windowed, gw, gh, wg, why)) || !windowed) continue;
        p->ids.push_back(i);
        p->geoms.push_back(wg);
        lens[i] = (size_t)wg.ww * wg.wh * descs[i].ncomp;
    }
    p->number();
    p->bytes = arena_layout(lens, p->off, p->len);
    return p;
}
// batch_rewindow's part: refused with nothing changed, or the new geometries and the new layout
int emu_plan_rewindow(void *plan, const jpgpu_window *windows) {
    Plan *p = static_cast<Plan *>(plan);
    std::vector<WindowGeom> geoms;
    std::vector<size_t> lens;
    const int rc = window_rule_rewindow(p->descs, p->ids, p->full_len, windows, geoms, lens);
    if (rc) return rc;
    p->bytes = arena_layout(lens, p->off, p->len);
    p->geoms = geoms;
    p->number();
    return JPGPU_OK;
}
uint32_t emu_plan_members(const void *plan) { return (uint32_t)static_cast<const Plan *>(plan)->ids.size(); }
// ids / geoms: per member; off / len / full_len: per image; returns the arena's bytes
size_t emu_plan_read(const void *plan, uint32_t *ids, uint32_t *geoms, size_t *off, size_t *len, size_t *full_len) {
    const Plan *p = static_cast<const Plan *>(plan);
    for (size_t k = 0; k < p->ids.size(); k++) ids[k] = p->ids[k];
    memcpy(geoms, p->geoms.data(), p->geoms.size() * sizeof(WindowGeom));
    for (size_t i = 0; i < p->descs.size(); i++) off[i] = p->off[i], len[i] = p->len[i], full_len[i] = p->full_len[i];
    return p->bytes;
}
void emu_plan_destroy(void *plan) { delete static_cast<Plan *>(plan); }
}
