// emu_tensor.cpp — TEST-ONLY CPU emulation of the tensor kernel (csrc/tensor_band.hpp, resample_tensor_kernel of csrc/resample.hip): the
// product's tables, planner and every workgroup of the launch grid through the product's own walk (band_walk of csrc/band_walk.hpp
// under the lanes of band_lanes.hpp: the walk's barriers are the phase boundaries).  Built by tests/test_tensor_emulation.py (g++, the
// flags of tests/emu/Makefile).
#include "hip_shim.hpp"
#include "band_lanes.hpp"

using namespace jpgpu;

extern "C" {
// `src` (any alignment): in_h rows of in_w * nc bytes; `dst` (16-byte aligned): nc planes of `plane` elements (0: out_h * out_w), the
// first out_h * out_w of each written.  dtype 1 / 2 / 3 = f32 / f16 / bf16, table from mean / std.  lds_cap / rb_cap: the planner's
// budget.  info = {rb, bands, cap_rows, most chunks of a band, lds_bytes}.  Returns 0, -1 when the planner refuses, -2 for a
// refused format.
int emu_tensor(const uint8_t *src, uint32_t in_w, uint32_t in_h, uint32_t nc, uint32_t out_w, uint32_t out_h, uint8_t *dst, uint32_t plane, uint32_t flip,
               uint32_t dtype, const float *mean, const float *std_, uint32_t lds_cap, uint32_t rb_cap, uint32_t *info) {
    const char *why = nullptr;
    if (!tensor_format_ok(dtype, 0, mean, std_, nc, why)) return -2;
    TensorJob t{};
    ResampleJob &j = t.r;
    j.src = src, j.dst = dst;
    j.in_w = in_w, j.in_h = in_h, j.nc = nc, j.out_w = out_w, j.out_h = out_h;
    j.hks = resample_ksize(in_w, out_w), j.vks = resample_ksize(in_h, out_h);
    j.hb = 0, j.hk = j.hb + 2u * out_w, j.vb = j.hk + out_w * j.hks, j.vk = j.vb + 2u * out_h;
    std::vector<int32_t> tab((size_t)j.vk + (size_t)out_h * j.vks);
    resample_coefficients(in_w, out_w, tab.data() + j.hb, tab.data() + j.hk, j.hks);
    resample_coefficients(in_h, out_h, tab.data() + j.vb, tab.data() + j.vk, j.vks);
    if (!resample_plan(j, tab.data(), lds_cap, rb_cap)) return -1;
    t.plane = plane ? plane : out_w * out_h;
    t.flip = flip;
    std::vector<uint32_t> ttab(4 * 256, 0xDEADBEEFu);
    tensor_table(dtype, mean, std_, nc, ttab.data());
    uint32_t most = 0;
    if (tensor_elem_bytes(dtype) == 4u) emu_launch_tensor<uint32_t>(t, tab.data(), ttab.data(), most);
    else emu_launch_tensor<uint16_t>(t, tab.data(), ttab.data(), most);
    if (info) info[0] = j.rb, info[1] = j.bands, info[2] = j.cap_rows, info[3] = most, info[4] = j.lds_bytes;
    return 0;
}
// tensor_table alone (what jpgpu_tensor_table wraps); 0, or -2 for a refused format
int emu_tensor_table(uint32_t dtype, uint32_t reserved, const float *mean, const float *std_, uint32_t nc, void *table) {
    const char *why = nullptr;
    if (!tensor_format_ok(dtype, reserved, mean, std_, nc, why)) return -2;
    tensor_table(dtype, mean, std_, nc, table);
    return 0;
}
}
