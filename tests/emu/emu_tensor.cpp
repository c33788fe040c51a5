// emu_tensor.cpp — TEST-ONLY CPU emulation of the tensor kernel (csrc/tensor_band.hpp, resample_tensor_kernel of csrc/resample.hip): the
// product's tables, planner and every workgroup of the launch grid, lane by lane and phase by phase (the kernel's barriers are the
// phase boundaries).  Built by tests/test_tensor_emulation.py (g++, the flags of tests/emu/Makefile).
#include "hip_shim.hpp"
#include <vector>
#include "../../jpeg-decoder_amd/csrc/tensor_band.hpp"

using namespace jpgpu;

template <class E>
static void run_bands(const TensorJob &t, const int32_t *tab, const uint32_t *ttab, uint8_t *lds, uint32_t lds_total, uint32_t &most) {
    typedef int32_t Sum[16];
    std::vector<int32_t> acc(RS_NT * 16);
    for (uint32_t band = 0; band < t.r.bands; band++) {
        const uint32_t chunks = RBand::chunks_of(t.r, tab, band);
        most = chunks > most ? chunks : most;
        memset(lds, 0xCD, lds_total);  // garbage, like real LDS
        for (uint32_t tid = 0; tid < RS_NT; tid++) TBand<E>::load_table(t, ttab, tid, lds);
        if (chunks == 1u) {
            for (uint32_t tid = 0; tid < RS_NT; tid++) RBand::hpass(t.r, tab, band, 0u, 0u, t.r.out_w, tid, lds);
            for (uint32_t tid = 0; tid < RS_NT; tid++) TBand<E>::vstore(t, tab, band, tid, lds);
            continue;
        }
        const uint32_t groups = TBand<E>::groups_of(t, band);
        for (uint32_t group = 0; group < groups; group++) {
            uint32_t x0, x1;
            TBand<E>::group_columns(t, band, group, x0, x1);
            std::fill(acc.begin(), acc.end(), 0);
            for (uint32_t chunk = 0; chunk < chunks; chunk++) {
                memset(lds, 0xCD, t.r.lds_bytes);  // (the rows only: the table stays)
                for (uint32_t tid = 0; tid < RS_NT; tid++) RBand::hpass(t.r, tab, band, chunk, x0, x1, tid, lds);
                for (uint32_t tid = 0; tid < RS_NT; tid++) TBand<E>::vacc(t, tab, band, chunk, group, tid, lds, *reinterpret_cast<Sum *>(&acc[16 * tid]));
            }
            for (uint32_t tid = 0; tid < RS_NT; tid++) TBand<E>::vput(t, band, group, tid, *reinterpret_cast<Sum *>(&acc[16 * tid]), lds);
        }
    }
}

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
    const uint32_t lds_total = ((j.lds_bytes + 15u) & ~15u) + TN_TABLE_MAX;
    std::vector<uint8_t> lds_store(lds_total + 16);
    uint8_t *lds = lds_store.data() + ((16 - ((uintptr_t)lds_store.data() & 15)) & 15);
    uint32_t most = 0;
    if (tensor_elem_bytes(dtype) == 4u) run_bands<uint32_t>(t, tab.data(), ttab.data(), lds, lds_total, most);
    else run_bands<uint16_t>(t, tab.data(), ttab.data(), lds, lds_total, most);
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
