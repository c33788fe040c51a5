// emu_orient.cpp — TEST-ONLY CPU emulation of the orientation kernel (csrc/orient_band.hpp, csrc/orient.hip): every workgroup of the
// launch grid, lane by lane, with the kernel's one barrier — every lane loads into LDS poisoned beforehand, then every lane stores.
// The stores go through a policy that counts them per destination byte.  Built by tests/test_orient_emulation.py (g++).
#include "hip_shim.hpp"
#include <vector>
#include "../../jpeg-decoder_amd/csrc/orient_band.hpp"

using namespace jpgpu;

namespace {
struct CountingStores {
    uint8_t *base;
    size_t bytes;
    uint32_t *count;  // per byte of [base, base + bytes + pad)
    uint32_t *outside;
    void put(uintptr_t p, uint8_t v) const {
        if (p < (uintptr_t)base || p >= (uintptr_t)base + bytes) return (void)++*outside;
        *reinterpret_cast<uint8_t *>(p) = v;
        count[p - (uintptr_t)base]++;
    }
    void dword(uintptr_t p, uint32_t v) const {
        if (p & 3u) ++*outside;  // (an unaligned dword store)
        for (uint32_t b = 0; b < 4u; b++) put(p + b, (uint8_t)(v >> (8u * b)));
    }
    void byte(uintptr_t p, uint8_t v) const { put(p, v); }
};

template <uint32_t NC>
void run_tile(const OrientJob &j, uint32_t tile, uint32_t *lds, const CountingStores &st) {
    memset(lds, 0xCD, OR_LDS_DW * 4u);  // garbage, like real LDS
    for (uint32_t tid = 0; tid < OR_NT; tid++) OBand<NC>::load(j, tile, tid, lds);
    for (uint32_t tid = 0; tid < OR_NT; tid++) OBand<NC>::store(j, tile, tid, lds, st);
}
}  // namespace

extern "C" {

// S of h x w x nc bytes at `src` under orientation o into dst (h * w * nc bytes); count: the stores every destination byte received;
// returns the stores that fell outside dst or were unaligned dwords.  src and dst must be 4-byte aligned and src readable up to the
// next multiple of 4 (the arena's contract).
uint32_t emu_orient(const uint8_t *src, uint32_t w, uint32_t h, uint32_t nc, uint32_t o, uint8_t *dst, uint32_t *count) {
    OrientJob j{};
    j.src = src, j.dst = dst, j.w = w, j.h = h, j.nc = nc, j.o = o;
    orient_job_tiles(j);
    std::vector<uint32_t> lds(OR_LDS_DW);
    uint32_t outside = 0;
    const CountingStores st{dst, orient_bytes(w, h, nc), count, &outside};
    for (uint32_t tile = 0; tile < j.tiles; tile++) {
        if (nc == 3u) run_tile<3u>(j, tile, lds.data(), st);
        else if (nc == 1u) run_tile<1u>(j, tile, lds.data(), st);
        else run_tile<4u>(j, tile, lds.data(), st);
    }
    return outside;
}
uint32_t emu_orient_tile() { return OR_T; }
// orient_source_window and oriented_size (out: sx, sy, sw, sh, ow, oh); 0, or -1 for a window outside O
int emu_orient_window(uint32_t o, uint32_t w, uint32_t h, uint32_t x, uint32_t y, uint32_t ww, uint32_t wh, uint32_t *out) {
    oriented_size(o, w, h, out[4], out[5]);
    return orient_source_window(o, w, h, x, y, ww, wh, out[0], out[1], out[2], out[3]) ? 0 : -1;
}

}  // extern "C"
