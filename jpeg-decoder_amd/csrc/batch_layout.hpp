// batch_layout.hpp — what a batch makes of its windows and where its images lie in an arena, stated once: the window rule
// (batch_create, batch_check_window, batch_rewindow), the output layout (the output, the intermediate and the rewindowed arena)
// and the headroom rule.  No HIP dependency (tests/emu/emu_batch_layout.cpp runs it on the CPU).
#pragma once
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "host_common.hpp"
#include "window_band.hpp"

namespace jpgpu {

// The window rule.  What window `wn` is on an image of descriptor `d`: JPGPU_OK with `windowed` (false: an empty window or one that
// covers the gw x gh output grid — no window) and the window's geometry in `wg`; JPGPU_ERR_FORMAT for a window outside the grid,
// JPGPU_ERR_UNSUPPORTED for a descriptor the window planner refuses (the reason in `why`).
// whole_grid_geom: plan "no window" as a window over the whole grid (batch_rewindow keeps such a member in its group).
inline int window_rule(const jpgpu_image_desc &d, const jpgpu_window &wn, bool &windowed, uint32_t &gw, uint32_t &gh, WindowGeom &wg, std::string &why,
                       bool whole_grid_geom = false) {
    windowed = false;
    window_grid(d.components, d.ncomp, d.out_w, d.out_h, gw, gh);
    uint32_t x = wn.x, y = wn.y, w = wn.w, h = wn.h;
    char msg[200];
    if (w != 0 && h != 0) {
        if (x + w > gw || y + h > gh) {
            snprintf(msg, sizeof(msg), "window (%u, %u) %ux%u outside the %ux%u image", x, y, w, h, gw, gh);
            why = msg;
            return JPGPU_ERR_FORMAT;
        }
        windowed = x != 0 || y != 0 || w != gw || h != gh;
    }
    if (!windowed) {
        if (!whole_grid_geom) return JPGPU_OK;
        x = y = 0, w = gw, h = gh;
    }
    uint8_t *dummy[4] = {nullptr, nullptr, nullptr, nullptr};
    ImageJob ij;
    size_t out_len = 0;
    int rc = build_image_job(d.components, d.ncomp, dummy, d.out_w, d.out_h, d.color_transform, nullptr, ij, out_len, why);
    if (rc) return rc;
    const char *reason = "";
    if (!window_geom_from_job(d.components, d.ncomp, ij, x, y, w, h, wg, reason)) {
        snprintf(msg, sizeof(msg), "no window kernel for this descriptor: %s", reason);
        why = msg;
        return JPGPU_ERR_UNSUPPORTED;
    }
    return JPGPU_OK;
}

// The rule for other windows on a batch whose window group is `ids` (in image order): the members' geometries and every image's
// output bytes (`full_len`: those of a whole image).  JPGPU_ERR_UNSUPPORTED — the caller creates a new batch — when another set of
// images would be windowed or a window lies outside its image.  A member whose new window is the whole image — one in a thousand of
// a loader's random crops — stays in the group: the window kernel decodes the whole grid to the same bytes.
inline int window_rule_rewindow(const std::vector<jpgpu_image_desc> &descs, const std::vector<uint32_t> &ids, const std::vector<size_t> &full_len,
                                const jpgpu_window *windows, std::vector<WindowGeom> &geoms, std::vector<size_t> &lens) {
    geoms.assign(ids.size(), WindowGeom{});
    lens = full_len;
    size_t k = 0;
    for (uint32_t i = 0; i < (uint32_t)descs.size(); i++) {
        const bool member = k < ids.size() && ids[k] == i;
        bool windowed = false;
        uint32_t gw = 0, gh = 0;
        WindowGeom wg;
        std::string why;
        if (window_rule(descs[i], windows[i], windowed, gw, gh, wg, why, member) != JPGPU_OK || (windowed && !member)) return JPGPU_ERR_UNSUPPORTED;
        if (!member) continue;
        lens[i] = (size_t)wg.ww * wg.wh * descs[i].ncomp;
        geoms[k++] = wg;
    }
    return JPGPU_OK;
}

// The output layout: images in order at 256-byte-aligned running offsets, an arena of at least 256 bytes.  Returns the arena's bytes.
inline size_t arena_layout(const std::vector<size_t> &lens, std::vector<size_t> &off, std::vector<size_t> &len) {
    size_t oo = 0;
    off.resize(lens.size());
    for (size_t i = 0; i < lens.size(); i++) {
        off[i] = oo;
        oo += align_up(lens[i], 256);
    }
    len = lens;
    return std::max<size_t>(oo, 256);
}
inline size_t arena_layout(const std::vector<size_t> &lens) {  // (the bytes alone)
    std::vector<size_t> off, len;
    return arena_layout(lens, off, len);
}

// A quarter more than asked for: what buffers that grow on demand and arenas with headroom allocate.
inline size_t quarter_more(size_t need) { return need + need / 4; }
// The headroom rule of arenas that hold windows (`full`: what the whole images take): a quarter more than these windows need, at most
// `full` — the totals of a loader's random crops differ little from call to call, and batch_rewindow sets other windows in place.
inline size_t arena_headroom(size_t need, size_t full) { return std::max(need, std::min(std::max<size_t>(full, 256), quarter_more(need))); }

}  // namespace jpgpu
