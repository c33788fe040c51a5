// emu_resample.cpp — TEST-ONLY CPU emulation of the resample kernel (csrc/resample_band.hpp): the product's tables, planner and every
// workgroup of the launch grid through the product's own walk (band_walk of csrc/band_walk.hpp under the lanes of band_lanes.hpp: the
// walk's barriers are the phase boundaries).  Built by tests/test_resample_emulation.py (g++, the flags of tests/emu/Makefile).
#include "hip_shim.hpp"
#include "band_lanes.hpp"

using namespace jpgpu;

extern "C" {
// `src` (any alignment): in_h rows of in_w * nc bytes; `dst` (4-byte aligned): out_h * out_w * nc bytes.  lds_cap / rb_cap: the
// planner's budget (small ones force the chunked vertical path / short bands).  info = {rb, bands, cap_rows, most chunks of a band,
// lds_bytes}.  Returns 0, or -1 when the planner refuses.
int emu_resample(const uint8_t *src, uint32_t in_w, uint32_t in_h, uint32_t nc, uint32_t out_w, uint32_t out_h, uint8_t *dst, uint32_t lds_cap, uint32_t rb_cap,
                 uint32_t *info) {
    ResampleJob j{};
    j.src = src, j.dst = dst;
    j.in_w = in_w, j.in_h = in_h, j.nc = nc, j.out_w = out_w, j.out_h = out_h;
    j.hks = resample_ksize(in_w, out_w), j.vks = resample_ksize(in_h, out_h);
    j.hb = 0, j.hk = j.hb + 2u * out_w, j.vb = j.hk + out_w * j.hks, j.vk = j.vb + 2u * out_h;
    std::vector<int32_t> tab((size_t)j.vk + (size_t)out_h * j.vks);
    resample_coefficients(in_w, out_w, tab.data() + j.hb, tab.data() + j.hk, j.hks);
    resample_coefficients(in_h, out_h, tab.data() + j.vb, tab.data() + j.vk, j.vks);
    if (!resample_plan(j, tab.data(), lds_cap, rb_cap)) return -1;
    uint32_t most = 0;
    emu_launch_u8(j, tab.data(), most);
    if (info) info[0] = j.rb, info[1] = j.bands, info[2] = j.cap_rows, info[3] = most, info[4] = j.lds_bytes;
    return 0;
}
// resample_coefficients alone (what jpgpu_resample_coefficients wraps)
uint32_t emu_resample_ksize(uint32_t in_size, uint32_t out_size) { return resample_ksize(in_size, out_size); }
void emu_resample_coefficients(uint32_t in_size, uint32_t out_size, int32_t *bounds, int32_t *coefs, uint32_t ksize) {
    resample_coefficients(in_size, out_size, bounds, coefs, ksize);
}
}
