// emu_resample.cpp — TEST-ONLY CPU emulation of the resample kernel (csrc/resample_band.hpp): the product's tables, planner and every
// workgroup of the launch grid, lane by lane and phase by phase (the kernel's barriers are the phase boundaries).  Built by
// tests/test_resample_emulation.py (g++, the flags of tests/emu/Makefile).
#include "hip_shim.hpp"
#include <vector>
#include "../../jpeg-decoder_amd/csrc/resample_band.hpp"

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
    std::vector<uint8_t> lds_store(j.lds_bytes + 16);
    uint8_t *lds = lds_store.data() + ((16 - ((uintptr_t)lds_store.data() & 15)) & 15);
    std::vector<int32_t> acc(RS_NT * 4);
    uint32_t most = 0;
    for (uint32_t band = 0; band < j.bands; band++) {
        const uint32_t chunks = RBand::chunks_of(j, tab.data(), band);
        most = chunks > most ? chunks : most;
        memset(lds, 0xCD, j.lds_bytes);  // garbage, like real LDS
        if (chunks == 1u) {
            for (uint32_t t = 0; t < RS_NT; t++) RBand::hpass(j, tab.data(), band, 0u, 0u, j.out_w, t, lds);
            for (uint32_t t = 0; t < RS_NT; t++) RBand::vstore(j, tab.data(), band, t, lds);
            continue;
        }
        const uint32_t groups = RBand::groups_of(j, band);
        for (uint32_t group = 0; group < groups; group++) {
            uint32_t x0, x1;
            RBand::group_columns(j, band, group, x0, x1);
            std::fill(acc.begin(), acc.end(), 0);
            for (uint32_t chunk = 0; chunk < chunks; chunk++) {
                memset(lds, 0xCD, j.lds_bytes);
                for (uint32_t t = 0; t < RS_NT; t++) RBand::hpass(j, tab.data(), band, chunk, x0, x1, t, lds);
                for (uint32_t t = 0; t < RS_NT; t++) RBand::vacc(j, tab.data(), band, chunk, group, t, lds, *reinterpret_cast<int32_t(*)[4]>(&acc[4 * t]));
            }
            for (uint32_t t = 0; t < RS_NT; t++) RBand::vput(j, band, group, t, *reinterpret_cast<int32_t(*)[4]>(&acc[4 * t]));
        }
    }
    if (info) info[0] = j.rb, info[1] = j.bands, info[2] = j.cap_rows, info[3] = most, info[4] = j.lds_bytes;
    return 0;
}
// resample_coefficients alone (what jpgpu_resample_coefficients wraps)
uint32_t emu_resample_ksize(uint32_t in_size, uint32_t out_size) { return resample_ksize(in_size, out_size); }
void emu_resample_coefficients(uint32_t in_size, uint32_t out_size, int32_t *bounds, int32_t *coefs, uint32_t ksize) {
    resample_coefficients(in_size, out_size, bounds, coefs, ksize);
}
}
