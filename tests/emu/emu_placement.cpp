// emu_placement.cpp — TEST-ONLY CPU emulation of the placed kernels (csrc/placed_band.hpp, csrc/placed.hip): the product's range tables,
// planner and every workgroup of the launch grid through the product's own walk (band_walk of csrc/band_walk.hpp under the lanes of
// band_lanes.hpp: the walk's barriers are the phase boundaries).
// Built by tests/test_placement_emulation.py (g++, the flags of tests/emu/Makefile) and, with its own main, by the stand-alone
// sanitizer program tests/emu/placement_asan.cpp.
#include "hip_shim.hpp"
#include "band_lanes.hpp"

using namespace jpgpu;

namespace {

// the job of the visible rectangle and its place: tables of the visible ranges into `tab`.  0, -1 planner refusal, -3 nothing visible
int plan(ResampleJob &j, Place &p, std::vector<int32_t> &tab, uint32_t in_w, uint32_t in_h, uint32_t nc, uint32_t kind, uint32_t cw, uint32_t ch, uint32_t rw,
         uint32_t rh, int32_t x, int32_t y, const uint8_t *fill, uint32_t lds_cap, uint32_t rb_cap) {
    uint32_t fx, fy;
    j.in_w = in_w, j.in_h = in_h, j.nc = kind ? 3u : nc, j.src_nc = kind;
    if (!placed_axis(rw, x, cw, fx, j.out_w, p.vx) || !placed_axis(rh, y, ch, fy, j.out_h, p.vy)) return -3;
    p.cw = cw, p.ch = ch;
    p.fill = (uint32_t)fill[0] | ((uint32_t)fill[1] << 8) | ((uint32_t)fill[2] << 16) | ((uint32_t)fill[3] << 24);
    j.hks = resample_ksize(in_w, rw), j.vks = resample_ksize(in_h, rh);
    j.hb = 0, j.hk = j.hb + 2u * j.out_w, j.vb = j.hk + j.out_w * j.hks, j.vk = j.vb + 2u * j.out_h;
    tab.assign((size_t)j.vk + (size_t)j.out_h * j.vks, 0);
    resample_coefficients_range(in_w, rw, fx, j.out_w, tab.data() + j.hb, tab.data() + j.hk, j.hks);
    resample_coefficients_range(in_h, rh, fy, j.out_h, tab.data() + j.vb, tab.data() + j.vk, j.vks);
    return placed_plan(j, p, tab.data(), lds_cap, rb_cap) ? 0 : -1;
}

// info: rb, the job's bands, cap_rows, most chunks of a band, lds_bytes, canvas bands, bands above the first visible one, bands without a
// visible row, bands whose first AND last dword are shared with a neighbour, visible width, visible height, shift
void fill_info(uint32_t *info, const ResampleJob &j, const Place &p, uint32_t most, uint32_t fill_bands, uint32_t shared) {
    if (!info) return;
    info[0] = j.rb, info[1] = j.bands, info[2] = j.cap_rows, info[3] = most, info[4] = j.lds_bytes, info[5] = p.bands, info[6] = p.pre;
    info[7] = fill_bands, info[8] = shared, info[9] = j.out_w, info[10] = j.out_h, info[11] = p.shift;
}

}  // namespace

extern "C" {
// `src` (any alignment): in_h rows of in_w * nc bytes (kind 1 / 4: a gray / CMYK source converted, nc is 1 / 4 then and the canvas has
// three channels); `dst` (4-byte aligned): the canvas, ch rows of cw * channels bytes.  lds_cap / rb_cap: the planner's budget.
// Returns 0, -1 when the planner refuses, -3 when the placement shows no pixel.
int emu_placed(const uint8_t *src, uint32_t in_w, uint32_t in_h, uint32_t nc, uint32_t kind, uint32_t cw, uint32_t ch, uint32_t rw, uint32_t rh, int32_t x,
               int32_t y, const uint8_t *fill, uint8_t *dst, uint32_t lds_cap, uint32_t rb_cap, uint32_t *info) {
    PlacedJob pj{};
    ResampleJob &j = pj.r;
    std::vector<int32_t> tab;
    int rc = plan(j, pj.p, tab, in_w, in_h, nc, kind, cw, ch, rw, rh, x, y, fill, lds_cap, rb_cap);
    if (rc) return rc;
    j.src = src, j.dst = dst;
    uint32_t most = 0, fill_bands = 0, shared = 0;
    for (uint32_t band = 0; band < pj.p.bands; band++) {
        uint32_t a, b, q0, q1;
        PBand::run_of(j, pj.p, band, a, b, q0, q1);
        if ((a & 3u) && (b & 3u) && q1 - q0 >= 2u) shared++;
    }
    emu_launch_placed(pj, tab.data(), most, fill_bands);
    fill_info(info, j, pj.p, most, fill_bands, shared);
    return 0;
}
// the tensor kernels: `dst` (16-byte aligned) channels planes of `plane` elements (0: ch * cw).  dtype 1 / 2 / 3 = f32 / f16 / bf16.
// -2 for a refused format.
int emu_placed_tensor(const uint8_t *src, uint32_t in_w, uint32_t in_h, uint32_t nc, uint32_t kind, uint32_t cw, uint32_t ch, uint32_t rw, uint32_t rh,
                      int32_t x, int32_t y, const uint8_t *fill, uint8_t *dst, uint32_t plane, uint32_t flip, uint32_t dtype, const float *mean,
                      const float *std_, uint32_t lds_cap, uint32_t rb_cap, uint32_t *info) {
    const char *why = nullptr;
    const uint32_t onc = kind ? 3u : nc;
    if (!tensor_format_ok(dtype, 0, mean, std_, onc, why)) return -2;
    PlacedTensorJob t{};
    ResampleJob &j = t.t.r;
    std::vector<int32_t> tab;
    int rc = plan(j, t.p, tab, in_w, in_h, nc, kind, cw, ch, rw, rh, x, y, fill, lds_cap, rb_cap);
    if (rc) return rc;
    j.src = src, j.dst = dst;
    t.t.plane = plane ? plane : cw * ch;
    t.t.flip = flip;
    std::vector<uint32_t> ttab(4 * 256, 0xDEADBEEFu);
    tensor_table(dtype, mean, std_, onc, ttab.data());
    uint32_t most = 0, fill_bands = 0;
    if (tensor_elem_bytes(dtype) == 4u) emu_launch_placed_tensor<uint32_t>(t, tab.data(), ttab.data(), most, fill_bands);
    else emu_launch_placed_tensor<uint16_t>(t, tab.data(), ttab.data(), most, fill_bands);
    fill_info(info, j, t.p, most, fill_bands, 0);
    return 0;
}
// resample_coefficients_range alone (what jpgpu_resample_coefficients_range wraps)
void emu_placed_range(uint32_t in_size, uint32_t out_size, uint32_t first, uint32_t count, int32_t *bounds, int32_t *coefs, uint32_t ksize) {
    resample_coefficients_range(in_size, out_size, first, count, bounds, coefs, ksize);
}
// fit_placement alone (what jpgpu_fit_placement wraps): out = {rw, rh, x, y}; 0, or -1 for a refused rule
int emu_placed_fit(uint32_t mode, uint32_t size, uint32_t src_w, uint32_t src_h, uint32_t out_w, uint32_t out_h, int32_t *out) {
    uint32_t rw, rh;
    int32_t x, y;
    if (!fit_placement(mode, size, src_w, src_h, out_w, out_h, rw, rh, x, y)) return -1;
    out[0] = (int32_t)rw, out[1] = (int32_t)rh, out[2] = x, out[3] = y;
    return 0;
}
}
