// emu_warp.cpp — TEST-ONLY CPU emulation of the warp kernels (csrc/warp_band.hpp, csrc/warp.hip): the product's job builder (the
// fixed-point coefficients, the N-sep tables) and every workgroup of the launch grid, lane by lane.  Built by tests/test_warp.py (g++,
// -ffp-contract=off) and, with its own main, by the stand-alone sanitizer program tests/emu/warp_asan.cpp.
#include "hip_shim.hpp"
#include <vector>
#include "../../jpeg-decoder_amd/csrc/tensor_band.hpp"
#include "../../jpeg-decoder_amd/csrc/warp_band.hpp"

using namespace jpgpu;

extern "C" {

// One image of w x h x nc bytes at `src` through matrix m under `filter` into dst: es == 0: h x w x nc bytes; es == 2 / 4: nc planes of
// w x h elements looked up in ttab (nc x 256 elements).  kind_out: the body the job builder chose.  0, or -1 for a refused matrix.
int emu_warp(const uint8_t *src, uint32_t w, uint32_t h, uint32_t nc, uint32_t flip, uint32_t filter, const double *m, const uint8_t *fill, void *dst, uint32_t es,
             const void *ttab, uint32_t *kind_out) {
    if (!warp_check(m, w, h)) return -1;
    // (as the batch lays the launch out: two images, the second one the job under test, so that WarpJob::tab is no zero)
    std::vector<int32_t> tabs(2u * ((size_t)w + h), 0x7fffffff);
    WarpJob j{};
    j.src = src, j.dst = dst;
    j.w = w, j.h = h, j.nc = nc, j.flip = flip;
    j.fill = (uint32_t)fill[0] | ((uint32_t)fill[1] << 8) | ((uint32_t)fill[2] << 16) | ((uint32_t)fill[3] << 24);
    j.plane = w * h;
    j.tab = w + h;
    warp_job_matrix(j, m, filter, tabs.data() + j.tab);
    if (kind_out) *kind_out = j.kind;
    const uint32_t tiles = AffBand::tiles_of(w, h);
    for (uint32_t tile = 0; tile < tiles; tile++)
        for (uint32_t tid = 0; tid < WP_NT; tid++) {
            if (es == 0u) AffBand::lane_u8(j, tabs.data(), tile, tid);
            else if (es == 4u) AffBand::lane_tensor<uint32_t>(j, tabs.data(), (const uint32_t *)ttab, tile, tid);
            else AffBand::lane_tensor<uint16_t>(j, tabs.data(), (const uint16_t *)ttab, tile, tid);
        }
    return 0;
}

int emu_warp_check(const double *m, uint32_t w, uint32_t h) { return warp_check(m, w, h) ? 0 : -1; }

}  // extern "C"
