// warp_asan.cpp — TEST-ONLY stand-alone program: the warp's job builder, its host functions and every emulated workgroup of the warp
// kernels (emu_warp.cpp) under AddressSanitizer + UBSan, over small cases that reach every body (N, N-sep, B), u8 and tensor stores of
// every channel count, flips, matrices at the refusal bounds and sizes of one pixel and of one tile and a bit.  Built and run by
// tests/test_warp.py:
//   g++ -fsanitize=address,undefined ... -ffp-contract=off -include hip_shim.hpp warp_asan.cpp      exit code 0 = no report, every check held
#include "emu_warp.cpp"

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

struct Mat {
    double m[6];
};
const uint32_t kSizes[][2] = {{1, 1}, {33, 21}, {16, 16}, {257, 1}, {3, 300}, {2048, 2}};
const Mat kMats[] = {{{1, 0, 0, 0, 1, 0}},         {{1, 0, 3.3, 0, 1, -2.7}},        {{0.5, 0, 0, 0, 0.5, 0}},         {{-1, 0, 33, 0, 1, 0}},
                     {{0.9659258262890683, -0.25881904510252074, 4.1, 0.25881904510252074, 0.9659258262890683, -3.2}},
                     {{0, 1, 0, -1, 0, 21}},       {{1, 0.3, -4, 0, 1, 0}},          {{1, 0, 5000, 0, 1, 5000}},       {{0.01, 0.002, 10, -0.003, 0.01, 7}},
                     {{1, 0, -31000, 0, 1, 31000}}, {{-15.5, 0, 32000, 0, -9.25, 300}}, {{7.5, -3.25, -100, 2.125, 9, -250}}};

void run(uint32_t w, uint32_t h, uint32_t nc, uint32_t flip, uint32_t filter, const Mat &mt, uint32_t es) {
    const uint8_t fill[4] = {114, 7, 200, 33};
    uint8_t *src = (uint8_t *)malloc((size_t)w * h * nc);  // (exactly the image: a byte beyond it is a report)
    uint32_t s = 99u + w * 7u + h + nc;
    for (size_t i = 0; i < (size_t)w * h * nc; i++) src[i] = (uint8_t)((s = s * 1664525u + 1013904223u) >> 24);
    const size_t n = (size_t)w * h * nc * (es ? es : 1u);
    void *dst = malloc(n);
    memset(dst, 0x5A, n);
    std::vector<uint32_t> table(4 * 256);
    const float mean[4] = {0.485f, 0.456f, 0.406f, 0.f}, std_[4] = {0.229f, 0.224f, 0.225f, 1.f};
    if (es) tensor_table(es == 4u ? TN_F32 : TN_F16, mean, std_, nc, table.data());
    uint32_t kind = 9;
    const int rc = emu_warp(src, w, h, nc, flip, filter, mt.m, fill, dst, es, table.data(), &kind);
    if (rc != 0) {  // (refused for this size: nothing written)
        CHECK(((uint8_t *)dst)[0] == 0x5A, "a refused matrix wrote");
    } else {
        CHECK(kind == (filter ? WP_KIND_B : ((mt.m[1] == 0 && mt.m[3] == 0) ? WP_KIND_NSEP : WP_KIND_N)), "kind %u", kind);
        const bool identity = &mt == &kMats[0], outside = &mt == &kMats[7];
        for (uint32_t Y = 0; Y < h && (identity || outside); Y++)
            for (uint32_t X = 0; X < w; X++)
                for (uint32_t c = 0; c < nc; c++) {
                    const uint32_t want = outside ? fill[c] : src[((size_t)Y * w + (flip ? w - 1 - X : X)) * nc + c];
                    const size_t e = ((size_t)c * h + Y) * w + X, t = (size_t)c * 256 + want;
                    const bool same = es == 0 ? ((uint8_t *)dst)[((size_t)Y * w + X) * nc + c] == want
                                              : (es == 4 ? ((uint32_t *)dst)[e] == table[t] : ((uint16_t *)dst)[e] == ((uint16_t *)table.data())[t]);
                    CHECK(same, "(%u, %u, %u) of %ux%u filter %u flip %u es %u", X, Y, c, w, h, filter, flip, es);
                }
    }
    free(dst);
    free(src);
}

void host_functions() {
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    const Mat bad[] = {{{nan, 0, 0, 0, 1, 0}}, {{1, 0, inf, 0, 1, 0}}, {{16000.5, 0, 0, 0, 1, 0}}, {{1, 0, 0, -16001, 1, 0}}, {{1, 0, 32000.5, 0, 1, 0}}, {{1, 0, 0, 0, 1, -32001}},
                       {{100, 0, 0, 0, 1, 0}}};
    for (const Mat &b : bad) CHECK(emu_warp_check(b.m, 400, 300) != 0, "accepted (%g ...)", b.m[0]);
    CHECK(emu_warp_check(kMats[0].m, 2048, 2048) == 0, "identity");
    int32_t idx[8];
    warp_nearest_axis(1e300, -1.0, 8, idx);  // (positions no int holds)
    CHECK(idx[0] == 2147483647, "huge %d", idx[0]);
    warp_nearest_axis(nan, 0.0, 8, idx);
    CHECK(idx[3] == -1, "nan %d", idx[3]);
    warp_nearest_axis(-1e300, 5.0, 8, idx);
    CHECK(idx[7] == -1, "negative %d", idx[7]);
}

}  // namespace

int main() {
    host_functions();
    for (auto &sz : kSizes)
        for (const Mat &mt : kMats)
            for (uint32_t filter = 0; filter < 2; filter++) {
                for (uint32_t nc : {1u, 3u, 4u}) run(sz[0], sz[1], nc, (nc + filter) & 1u, filter, mt, 0);
                run(sz[0], sz[1], 3, 1, filter, mt, 4);
                run(sz[0], sz[1], 1, 0, filter, mt, 2);
                run(sz[0], sz[1], 4, 0, filter, mt, 4);
                run(sz[0], sz[1], 2, 1, filter, mt, 0);
            }
    if (failures) fprintf(stderr, "%d checks failed\n", failures);
    else printf("warp_asan: ok\n");
    return failures ? 1 : 0;
}
