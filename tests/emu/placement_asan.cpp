// placement_asan.cpp — TEST-ONLY stand-alone program: the placement planner, the range tables, the fit rules and every emulated workgroup of
// the placed kernels (emu_placement.cpp) under AddressSanitizer + UBSan, over small cases that reach every path: crop, pad, bands of
// fill, shared dwords, the chunked path, one visible pixel at every corner, both tensor item forms with and without a flip, the
// converting horizontal passes.  Built and run by tests/test_placement.py:
//   g++ -fsanitize=address,undefined ... -include hip_shim.hpp placement_asan.cpp      exit code 0 = no report and every check held
#include "emu_placement.cpp"

#include <cstdio>
#include <cstdlib>

namespace {

int failures = 0;
#define CHECK(cond, ...)                              \
    do {                                              \
        if (!(cond)) {                                \
            failures++;                               \
            fprintf(stderr, "FAILED %s: ", #cond);    \
            fprintf(stderr, __VA_ARGS__);             \
            fprintf(stderr, "\n");                    \
        }                                             \
    } while (0)

struct Case {
    uint32_t in_w, in_h, cw, ch, rw, rh;
    int32_t x, y;
    uint32_t lds_cap, rb_cap;
};
const Case kCases[] = {
    {100, 75, 56, 56, 85, 64, -15, -3, RS_MAX_LDS, 64}, {9, 17, 37, 53, 27, 51, 5, 1, RS_MAX_LDS, 3},   {50, 34, 37, 53, 61, 20, -11, 17, RS_MAX_LDS, 5},
    {161, 97, 16, 200, 5, 8, 6, 150, RS_MAX_LDS, 64},   {24, 1100, 7, 7, 2, 1, 1, 3, 64, 64},           {20, 300, 9, 6, 7, 2, 1, 3, 48, 64},
    {131, 97, 3, 3, 61, 45, -60, -44, RS_MAX_LDS, 64},  {131, 97, 3, 3, 61, 45, 2, -44, RS_MAX_LDS, 64}, {131, 97, 3, 3, 61, 45, -60, 2, RS_MAX_LDS, 64},
    {131, 97, 3, 3, 61, 45, 2, 2, RS_MAX_LDS, 64},      {34, 50, 2048, 3, 102, 150, 1000, -70, RS_MAX_LDS, 64}, {50, 34, 224, 224, 150, 102, 38, -3, RS_MAX_LDS, 64},
    {100, 75, 64, 8, 85, 64, -15, -3, RS_MAX_LDS, 64},  {16, 1200, 2048, 2, 2500, 1, -200, 1, RS_MAX_LDS, 64}, {8, 8, 8, 8, 8, 8, 0, 0, RS_MAX_LDS, 64},
};

// the source in a buffer with the slack of the product's arenas (the horizontal pass reads the aligned dwords that hold its bytes)
struct Source {
    std::vector<uint8_t> store;
    const uint8_t *p;
    Source(uint32_t w, uint32_t h, uint32_t nc, uint32_t off) : store((size_t)w * h * nc + 32 + off) {
        uint32_t s = 12345u + w * 7u + h;
        for (uint8_t &b : store) b = (uint8_t)((s = s * 1664525u + 1013904223u) >> 24);
        p = store.data() + 16 + off;
    }
};

bool visible(const Case &c, uint32_t X, uint32_t Y) {
    return (int64_t)X >= c.x && (int64_t)X < (int64_t)c.x + c.rw && (int64_t)Y >= c.y && (int64_t)Y < (int64_t)c.y + c.rh;
}

void run_u8(const Case &c, uint32_t nc, uint32_t kind) {
    const uint8_t fill[4] = {114, 7, 200, 33};
    const uint32_t onc = kind ? 3u : nc;
    const size_t n = (size_t)c.cw * c.ch * onc;
    Source src(c.in_w, c.in_h, nc, nc & 3u);
    uint8_t *dst = (uint8_t *)malloc(n);  // (exactly the canvas: a byte beyond it is a report)
    memset(dst, 0x5A, n);
    uint32_t info[16] = {0};
    const int rc = emu_placed(src.p, c.in_w, c.in_h, nc, kind, c.cw, c.ch, c.rw, c.rh, c.x, c.y, fill, dst, c.lds_cap, c.rb_cap, info);
    CHECK(rc == 0, "emu_placed rc %d", rc);
    for (uint32_t Y = 0; Y < c.ch && rc == 0; Y++)
        for (uint32_t X = 0; X < c.cw; X++)
            if (!visible(c, X, Y))
                for (uint32_t ch = 0; ch < onc; ch++)
                    CHECK(dst[((size_t)Y * c.cw + X) * onc + ch] == fill[ch], "fill at (%u, %u, %u) of %ux%u", X, Y, ch, c.cw, c.ch);
    free(dst);
}

void run_tensor(const Case &c, uint32_t nc, uint32_t dtype, uint32_t flip) {
    const uint8_t fill[4] = {114, 7, 200, 33};
    const float mean[4] = {0.485f, 0.456f, 0.406f, 0.f}, std_[4] = {0.229f, 0.224f, 0.225f, 1.f};
    const uint32_t es = tensor_elem_bytes(dtype);
    const size_t n = (size_t)c.cw * c.ch * nc * es;
    Source src(c.in_w, c.in_h, nc, 1);
    void *dst = nullptr;
    if (posix_memalign(&dst, 16, (n + 15) & ~(size_t)15)) abort();
    memset(dst, 0x5A, (n + 15) & ~(size_t)15);
    uint32_t info[16] = {0};
    const int rc = emu_placed_tensor(src.p, c.in_w, c.in_h, nc, 0, c.cw, c.ch, c.rw, c.rh, c.x, c.y, fill, (uint8_t *)dst, 0, flip, dtype, mean, std_, c.lds_cap,
                                     c.rb_cap, info);
    CHECK(rc == 0, "emu_placed_tensor rc %d", rc);
    std::vector<uint32_t> table(4 * 256);
    tensor_table(dtype, mean, std_, nc, table.data());
    for (uint32_t ch = 0; ch < nc && rc == 0; ch++)
        for (uint32_t Y = 0; Y < c.ch; Y++)
            for (uint32_t X = 0; X < c.cw; X++) {
                if (visible(c, flip ? c.cw - 1 - X : X, Y)) continue;
                const size_t e = ((size_t)ch * c.ch + Y) * c.cw + X, t = (size_t)ch * 256 + fill[ch];
                const bool same = es == 4 ? ((uint32_t *)dst)[e] == table[t] : ((uint16_t *)dst)[e] == ((uint16_t *)table.data())[t];
                CHECK(same, "filled element (%u, %u, %u) of %ux%u flip %u", ch, Y, X, c.cw, c.ch, flip);
            }
    for (size_t i = n; i < ((n + 15) & ~(size_t)15); i++) CHECK(((uint8_t *)dst)[i] == 0x5A, "byte %zu behind the tensor", i - n);
    free(dst);
}

void range_tables() {
    const uint32_t pairs[][2] = {{1, 65535}, {65535, 1}, {1080, 455}, {375, 256}, {13, 997}};
    for (auto &pr : pairs) {
        const uint32_t in = pr[0], out = pr[1], ks = resample_ksize(in, out);
        std::vector<int32_t> b(2 * (size_t)out), k((size_t)out * ks);
        resample_coefficients(in, out, b.data(), k.data(), ks);
        const uint32_t spans[][2] = {{0, out < 300 ? out : 300}, {out - 1, 1}, {out / 2, out - out / 2 < 77 ? out - out / 2 : 77}};
        for (auto &sp : spans) {
            std::vector<int32_t> rb(2 * (size_t)sp[1]), rk((size_t)sp[1] * ks);  // (exactly `count` entries)
            resample_coefficients_range(in, out, sp[0], sp[1], rb.data(), rk.data(), ks);
            CHECK(memcmp(rb.data(), b.data() + 2 * (size_t)sp[0], rb.size() * 4) == 0 && memcmp(rk.data(), k.data() + (size_t)sp[0] * ks, rk.size() * 4) == 0,
                  "range [%u, +%u) of (%u, %u)", sp[0], sp[1], in, out);
        }
    }
}

void fits() {
    int32_t o[4];
    CHECK(emu_placed_fit(1, 256, 500, 375, 224, 224, o) == 0 && o[0] == 341 && o[1] == 256 && o[2] == -58 && o[3] == -16, "500x375");
    CHECK(emu_placed_fit(1, 256, 1920, 1080, 224, 224, o) == 0 && o[0] == 455 && o[2] == -116, "1920x1080");
    CHECK(emu_placed_fit(2, 0, 333, 500, 640, 640, o) == 0 && o[0] == 426 && o[1] == 640 && o[2] == 107 && o[3] == 0, "letterbox 333x500");
    CHECK(emu_placed_fit(1, 256, 8, 4000, 224, 224, o) != 0, "a side above 65535");
    CHECK(emu_placed_fit(1, 65535, 65535, 1, 1, 1, o) != 0, "overflowing sides");
    CHECK(emu_placed_fit(2, 0, 65535, 1, 2048, 2048, o) == 0 && o[1] == 1, "letterbox of a line");
}

}  // namespace

int main() {
    range_tables();
    fits();
    for (const Case &c : kCases) {
        for (uint32_t nc : {1u, 3u, 4u}) run_u8(c, nc, 0);
        run_u8(c, 1, 1);
        run_u8(c, 4, 4);
        for (uint32_t flip = 0; flip < 2; flip++) {
            run_tensor(c, 3, 1, flip);
            run_tensor(c, 1, 3, flip);
            run_tensor(c, 4, 2, flip);
        }
    }
    if (failures) fprintf(stderr, "%d checks failed\n", failures);
    else printf("placement_asan: ok\n");
    return failures ? 1 : 0;
}
