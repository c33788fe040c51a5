// emu_rgb.cpp — TEST-ONLY CPU emulation of the RGB-output kernels (resample_band_rgb_kernel / resample_tensor_rgb_kernel of
// csrc/resample.hip): the product's tables, planner and every workgroup of the launch grid through the product's own walk
// (band_walk of csrc/band_walk.hpp under the lanes of band_lanes.hpp: the walk's barriers are the phase boundaries), the horizontal
// pass chosen by the job's src_nc as the kernels choose it.
// Built by tests/test_rgb_emulation.py (g++, the flags of tests/emu/Makefile).
#include "hip_shim.hpp"
#include "band_lanes.hpp"

using namespace jpgpu;

// the job of an image of `snc` source channels in a batch with RGB output, as output_retable (csrc/batch_output.cpp) makes it
static bool make_job(ResampleJob &j, std::vector<int32_t> &tab, const uint8_t *src, uint32_t in_w, uint32_t in_h, uint32_t snc, uint32_t out_w, uint32_t out_h,
                     uint8_t *dst, uint32_t lds_cap, uint32_t rb_cap) {
    j.src = src, j.dst = dst;
    j.in_w = in_w, j.in_h = in_h, j.nc = 3u, j.out_w = out_w, j.out_h = out_h;
    j.src_nc = snc == 3u ? 0u : snc;
    j.hks = resample_ksize(in_w, out_w), j.vks = resample_ksize(in_h, out_h);
    j.hb = 0, j.hk = j.hb + 2u * out_w, j.vb = j.hk + out_w * j.hks, j.vk = j.vb + 2u * out_h;
    tab.assign((size_t)j.vk + (size_t)out_h * j.vks, 0);
    resample_coefficients(in_w, out_w, tab.data() + j.hb, tab.data() + j.hk, j.hks);
    resample_coefficients(in_h, out_h, tab.data() + j.vb, tab.data() + j.vk, j.vks);
    return resample_plan(j, tab.data(), lds_cap, rb_cap);
}

extern "C" {
// `src`: in_h rows of in_w * snc bytes (snc = 1: any alignment; 4: 4-byte aligned; 3: any); `dst` (4-byte aligned): out_h * out_w * 3
// bytes.  lds_cap / rb_cap: the planner's budget.  info = {rb, bands, cap_rows, most chunks of a band, lds_bytes, pitch}.  Returns 0,
// or -1 when the planner refuses.
int emu_rgb_resample(const uint8_t *src, uint32_t in_w, uint32_t in_h, uint32_t snc, uint32_t out_w, uint32_t out_h, uint8_t *dst, uint32_t lds_cap,
                     uint32_t rb_cap, uint32_t *info) {
    ResampleJob j{};
    std::vector<int32_t> tabv;
    if (!make_job(j, tabv, src, in_w, in_h, snc, out_w, out_h, dst, lds_cap, rb_cap)) return -1;
    const int32_t *tab = tabv.data();
    uint32_t most = 0;
    emu_launch_u8(j, tab, most);
    if (info) info[0] = j.rb, info[1] = j.bands, info[2] = j.cap_rows, info[3] = most, info[4] = j.lds_bytes, info[5] = j.pitch;
    return 0;
}
// The same source into a tensor: `dst` (16-byte aligned) 3 planes of out_h * out_w elements.  dtype 1 / 2 / 3 = f32 / f16 / bf16, the
// table of three channels from mean / std.  Returns 0, -1 when the planner refuses, -2 for a refused format.
int emu_rgb_tensor(const uint8_t *src, uint32_t in_w, uint32_t in_h, uint32_t snc, uint32_t out_w, uint32_t out_h, uint8_t *dst, uint32_t flip, uint32_t dtype,
                   const float *mean, const float *std_, uint32_t lds_cap, uint32_t rb_cap, uint32_t *info) {
    const char *why = nullptr;
    if (!tensor_format_ok(dtype, 0, mean, std_, 3u, why)) return -2;
    TensorJob t{};
    std::vector<int32_t> tabv;
    if (!make_job(t.r, tabv, src, in_w, in_h, snc, out_w, out_h, dst, lds_cap, rb_cap)) return -1;
    t.plane = out_w * out_h;
    t.flip = flip;
    std::vector<uint32_t> ttab(4 * 256, 0xDEADBEEFu);
    tensor_table(dtype, mean, std_, 3u, ttab.data());
    uint32_t most = 0;
    if (tensor_elem_bytes(dtype) == 4u) emu_launch_tensor<uint32_t>(t, tabv.data(), ttab.data(), most);
    else emu_launch_tensor<uint16_t>(t, tabv.data(), ttab.data(), most);
    if (info) info[0] = t.r.rb, info[1] = t.r.bands, info[2] = t.r.cap_rows, info[3] = most, info[4] = t.r.lds_bytes, info[5] = t.r.pitch;
    return 0;
}
// what the planner says to a job whose src_nc does not go with its nc (1: planned, 0: refused)
int emu_rgb_plan_ok(uint32_t nc, uint32_t src_nc) {
    ResampleJob j{};
    j.in_w = j.in_h = j.out_w = j.out_h = 4u, j.nc = nc, j.src_nc = src_nc;
    j.hks = j.vks = resample_ksize(4u, 4u);
    j.hb = 0, j.hk = 8u, j.vb = j.hk + 4u * j.hks, j.vk = j.vb + 8u;
    std::vector<int32_t> tab((size_t)j.vk + 4u * j.vks);
    resample_coefficients(4u, 4u, tab.data() + j.hb, tab.data() + j.hk, j.hks);
    resample_coefficients(4u, 4u, tab.data() + j.vb, tab.data() + j.vk, j.vks);
    return resample_plan(j, tab.data()) ? 1 : 0;
}
}
