// batch_output_asan.cpp — TEST-ONLY stand-alone program: csrc/batch_output.hpp under AddressSanitizer + UBSan.  The rule function over the
// whole cross of options, the per-image rule, spec equality, the placement normalisation at the edges of int32 and uint16, the bytes
// per image at the largest output, and the route table.  Built and run by tests/test_batch_output.py:
//   g++ -fsanitize=address,undefined ... -include hip_shim.hpp batch_output_asan.cpp      exit code 0 = no report and every check held
#include "emu_batch_output.cpp"

#include <climits>
#include <cstdio>

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
}  // namespace

int main() {
    const uint32_t sizes[4][2] = {{0, 0}, {8, 8}, {0, 8}, {2049, 8}}, filters[3] = {0, 3, 9}, dtypes[3] = {1, 2, 0}, wfilters[3] = {0, 1, 2};
    char why[300];
    int cells = 0;
    for (const auto &sz : sizes)
        for (uint32_t f : filters)
            for (uint32_t rgb = 0; rgb < 2; rgb++)
                for (uint32_t t = 0; t < 3; t++)      // none, f16, dtype 0
                    for (uint32_t wp = 0; wp < 3; wp++) {  // none, bilinear, filter 2
                        EmuSpec e{};
                        e.w = sz[0], e.h = sz[1], e.filter = f, e.rgb = rgb, e.tensor = t != 0, e.tn.dtype = dtypes[t], e.warp = wp != 0, e.wp.filter = wfilters[wp];
                        for (int c = 0; c < 4; c++) e.tn.std[c] = 1.0f;
                        const int rc = emu_output_rule(&e, why, sizeof why);
                        CHECK(rc == JPGPU_OK || rc == JPGPU_ERR_FORMAT || rc == JPGPU_ERR_UNSUPPORTED, "status %d", rc);
                        CHECK((rc == JPGPU_OK) == (why[0] == 0), "status %d with the reason '%s'", rc, why);
                        CHECK(emu_spec_equal(&e, &e) == 1, "a spec differs from itself");
                        for (uint32_t nc = 0; nc <= 5; nc++) (void)emu_output_image_rule(&e, nc, nc & 1 ? emu_cc_none() : 0u, why, sizeof why);
                        uint32_t r4[4];
                        for (int placed = 0; placed < 2; placed++) emu_output_route(&e, placed, wp, r4);
                        if (rc == JPGPU_OK && e.w) {
                            size_t off[3], len[3];
                            const uint32_t ncomps[3] = {1, 3, 4};
                            CHECK(emu_output_arena(&e, ncomps, 3, 0, off, len) >= len[0] + len[1] + len[2], "arena below its images");
                        }
                        cells++;
                    }
    CHECK(cells == 4 * 3 * 2 * 3 * 3, "%d cells", cells);
    // placements at the edges of what the fields hold
    const jpgpu_placement pls[] = {{0, 0, 0, 0},           {8, 8, 0, 0},       {65535, 65535, INT32_MIN, INT32_MIN}, {65535, 65535, INT32_MAX, INT32_MAX},
                                   {65535, 1, -65534, 7},  {1, 1, 7, 7},       {1, 1, 8, 0},                         {1, 1, -1, 0},
                                   {65535, 65535, -65535, 0}, {3, 0, 100, 100}};
    const uint32_t n = sizeof pls / sizeof pls[0];
    for (uint32_t first = 0; first < n; first++) {
        jpgpu_placement out[n];
        uint32_t placed = 0;
        const uint32_t k = emu_normalise_placements(pls + first, n - first, 8, 8, out, &placed);
        for (uint32_t i = 0; i < n - first; i++) {
            uint32_t a[3], b[3];
            const bool visible = emu_placed_axis(out[i].rw, out[i].x, 8, a) && emu_placed_axis(out[i].rh, out[i].y, 8, b);
            CHECK(i >= k || visible, "placement %u of the list from %u passed and shows nothing", i, first);
            CHECK(i != k || !visible, "placement %u of the list from %u refused and shows a pixel", i, first);
            if (i < k && visible) CHECK(a[2] + a[1] <= 8 && b[2] + b[1] <= 8, "visible range beyond the output");
        }
    }
    // the largest output in every element size
    EmuSpec big{};
    big.w = big.h = emu_rs_max_out(), big.tensor = 1, big.tn.dtype = 1, big.rgb = 1;
    CHECK(emu_output_image_bytes(&big, 1, 0) == (size_t)2048 * 2048 * 3 * 4, "f32 rgb bytes");
    CHECK(emu_output_image_bytes(&big, 4, 1) == (size_t)2048 * 2048 * 3, "u8 rgb bytes");
    if (failures) return fprintf(stderr, "batch_output_asan: %d check(s) failed\n", failures), 1;
    printf("batch_output_asan: ok\n");
    return 0;
}
