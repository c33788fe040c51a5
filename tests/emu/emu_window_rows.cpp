// emu_window_rows.cpp — TEST-ONLY: the rows of coefficient blocks the device entropy route keeps for a windowed image
// (window_kept_rows / window_kept_mcu_rows, csrc/window_band.hpp) against every block the window kernel's tiles enumerate
// (window_tile_blocks).  Built by tests/test_pipeline_windows_abi.py (g++, the flags of tests/emu/Makefile).
#include "hip_shim.hpp"
#include <string>
#include "../../jpeg-decoder_amd/csrc/host_common.hpp"
#include "../../jpeg-decoder_amd/csrc/window_band.hpp"

using namespace jpgpu;

extern "C" {
// rows[c] = {r0, r1} per component, mcu = {my0, my1}, counts = {tiles visited, blocks rows outside [r0, r1), component rows outside the
// MCU rows kept, rows kept that no tile touches}.  Returns -1 if the planner refused the window, else the status of build_image_job.
int emu_window_rows(const jpgpu_image_desc *desc, const uint32_t *win, uint32_t *rows, uint32_t *mcu, uint32_t *counts) {
    size_t out_len = 0;
    std::string err;
    uint8_t *no_planes[4] = {nullptr, nullptr, nullptr, nullptr};
    ImageJob job;
    int rc = build_image_job(desc->components, desc->ncomp, no_planes, desc->out_w, desc->out_h, desc->color_transform, nullptr, job, out_len, err);
    if (rc) return rc;
    WindowGeom g;
    const char *reason = "";
    if (!window_geom_from_job(desc->components, desc->ncomp, job, win[0], win[1], win[2], win[3], g, reason)) return -1;
    window_kept_mcu_rows(g, mcu[0], mcu[1]);
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    for (uint32_t c = 0; c < g.ncomp; c++) {
        uint32_t r0, r1;
        window_kept_rows(g, c, r0, r1);
        rows[2 * c] = r0, rows[2 * c + 1] = r1;
        if (r0 < mcu[0] * g.v[c] || r1 > mcu[1] * g.v[c] || r1 > g.block_h[c] || r0 >= r1) counts[2]++;
        int32_t lo = 0x7fffffff, hi = -1;
        for (uint32_t band = 0; band < g.bands; band++)
            for (uint32_t tile = 0; tile < g.tiles_x; tile++) {
                int32_t bx0, by0, bx1, by1;
                window_tile_blocks(g, c, tile, band, bx0, by0, bx1, by1);
                counts[0]++;
                if (by0 < (int32_t)r0 || by1 > (int32_t)r1) counts[1]++;
                lo = by0 < lo ? by0 : lo, hi = by1 > hi ? by1 : hi;
            }
        if (lo != (int32_t)r0 || hi != (int32_t)r1) counts[3]++;
    }
    return 0;
}
}
