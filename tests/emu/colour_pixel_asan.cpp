// colour_pixel_asan.cpp — TEST-ONLY stand-alone program: the colour stage's job builder, its refusal rule and the emulated workgroup of
// the colour kernel with HUE and SHARPNESS (emu_colour_pixel.cpp) under AddressSanitizer + UBSan.  Strips of K = 1, 2, 3 rows and of as
// many as LDS holds; heights K, K + 1, 2 K and 2 K + 1 (a last strip that is whole, one row, or the image's last row alone) beside
// heights below 3; widths 1, 2, 3, 5, 33 and a few whose rows start on every byte of a dword; both operations alone and in programs with
// the table operations, at three lane counts.  The image is allocated exactly: a byte beyond it is a report; so is a dword beyond the
// strip ring.  Built and run by tests/test_workgroup_colour_pixel.py:
//   g++ -fsanitize=address,undefined ... -ffp-contract=off -include hip_shim.hpp colour_pixel_asan.cpp     exit code 0 = no report, every check held
#include "emu_colour_pixel.cpp"

#include <cmath>
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

const uint32_t kLanes[] = {CL_NT, 64u, 192u};

ColourProgram program(std::initializer_list<ColourOp> ops) {
    ColourProgram p{};
    for (const ColourOp &o : ops) p.ops[p.n++] = o;
    return p;
}

// a scalar statement of the operations, pixel by pixel out of a copy, from the header's value functions; the table operations through
// the emulated kernel of their own (colour_asan.cpp compares that one with a statement of its own)
void reference(std::vector<uint8_t> &px, uint32_t w, uint32_t h, const ColourProgram &p) {
    for (uint32_t k = 0; k < p.n; k++) {
        const ColourOp o = p.ops[k];
        const std::vector<uint8_t> src(px);
        if (o.op == CL_HUE) {
            for (uint32_t i = 0; i < w * h; i++) {
                const uint32_t c = cl_hue_pixel(src[3 * i], src[3 * i + 1], src[3 * i + 2], (uint32_t)o.value);
                px[3 * i] = (uint8_t)c, px[3 * i + 1] = (uint8_t)(c >> 8), px[3 * i + 2] = (uint8_t)(c >> 16);
            }
        } else if (o.op == CL_SHARPNESS) {
            for (uint32_t y = 1; y + 1 < h; y++)
                for (uint32_t x = 1; x + 1 < w; x++)
                    for (uint32_t c = 0; c < 3; c++) {
                        uint32_t t[3][3];
                        for (uint32_t r = 0; r < 3; r++)  // (rows y + 1, y, y - 1)
                            for (uint32_t q = 0; q < 3; q++) t[r][q] = src[((size_t)(y + 1 - r) * w + (x + q - 1)) * 3 + c];
                        px[((size_t)y * w + x) * 3 + c] = (uint8_t)cl_blend(cl_smooth_value(t[0], t[1], t[2]), t[1][1], o.value);
                    }
        } else {
            const ColourProgram one = program({o});
            ColourJob j{};
            colour_job(j, px.data(), w, h, &one);
            double scale[256];
            colour_scale_table(scale);
            emu_pixel_workgroup<64u>(j, scale, 0u);
        }
    }
}

void run(uint32_t w, uint32_t h, const ColourProgram &p, uint32_t lanes, uint32_t strip_rows, uint32_t kind) {
    const size_t n = (size_t)w * h * 3;
    uint8_t *pix = (uint8_t *)malloc(n);  // (exactly the image)
    uint32_t s = 11u + w * 31u + h + kind;
    for (size_t i = 0; i < n; i++) {
        s = s * 1664525u + 1013904223u;
        const uint32_t x = (uint32_t)(i / 3u) % w, y = (uint32_t)(i / 3u) / w;
        pix[i] = kind == 0 ? (uint8_t)(s >> 24) : kind == 1 ? (uint8_t)(((x + y) & 1u) * 255u) : (uint8_t)(i % 3u == 0 ? 9u : 200u);  // (random, checkerboard, constant)
    }
    std::vector<uint8_t> want(pix, pix + n);
    reference(want, w, h, p);
    const int rc = emu_colour_pixel(pix, w, h, &p, lanes, strip_rows);
    CHECK(rc == 0, "refused");
    size_t bad = 0;
    for (size_t i = 0; i < n; i++) bad += pix[i] != want[i];
    CHECK(bad == 0, "%zu bytes differ: %ux%u lanes %u rows %u kind %u, first op %u of %u", bad, w, h, lanes, strip_rows, kind, p.ops[0].op, p.n);
    free(pix);
}

void refusals() {
    const float nan = std::nanf(""), inf = INFINITY;
    const ColourOp bad[] = {{9u, 0.f},  {10u, 0.f},        {15u, 1.f},           {18u, 1.f},         {255u, 0.f},           {CL_HUE, 255.5f},      {CL_HUE, 256.f},
                            {CL_HUE, -1.f}, {CL_HUE, nan}, {CL_HUE, inf},        {CL_SHARPNESS, nan}, {CL_SHARPNESS, 256.5f}, {CL_SHARPNESS, -0.5f}, {CL_SHARPNESS, inf}};
    for (const ColourOp &o : bad) {
        const ColourProgram p = program({{CL_INVERT, 0.f}, o});
        CHECK(emu_colour_pixel_check(&p) != 0, "accepted op %u value %g", o.op, o.value);
        uint8_t px[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
        CHECK(emu_colour_pixel(px, 2, 2, &p, CL_NT, 0u) != 0 && px[0] == 1, "a refused program wrote");
    }
    const ColourProgram ok = program({{CL_HUE, 0.f}, {CL_HUE, 255.f}, {CL_SHARPNESS, 0.f}, {CL_SHARPNESS, 256.f}});
    CHECK(emu_colour_pixel_check(&ok) == 0, "the bounds refused");
    // the strip rule: what LDS holds, at least 6 rows up to the greatest width; a forced count is clamped by it
    for (uint32_t w = 1; w <= CL_MAX_SIDE; w++) {
        const uint32_t K = cl_strip_rows(w, 0u);
        CHECK(K >= 6u && (size_t)(K + 2u) * cl_row_pitch(w) <= CL_STRIP_BYTES, "width %u: %u rows", w, K);
        CHECK(cl_strip_rows(w, 1u) == 1u && cl_strip_rows(w, 100000u) == K, "width %u: forced", w);
    }
    CHECK(sizeof(ColourLds) + sizeof(ColourStripLds) < 64u * 1024u, "LDS");
    CHECK(sharp_steps(2, 9, 3) == 0 && sharp_steps(9, 2, 3) == 0 && sharp_steps(3, 3, 3) == 2 && sharp_steps(3, 7, 3) == 6, "step counts");
}

}  // namespace

int main() {
    refusals();
    std::vector<ColourProgram> programs;
    for (float f : {0.f, 0.37f, 1.f, 1.9f, 256.f}) programs.push_back(program({{CL_SHARPNESS, f}}));
    for (float n : {0.f, 1.f, 43.f, 128.f, 255.f}) programs.push_back(program({{CL_HUE, n}}));
    programs.push_back(program({{CL_SHARPNESS, 1.9f}, {CL_CONTRAST, 1.9f}}));
    programs.push_back(program({{CL_HUE, 43.f}, {CL_EQUALIZE, 0.f}}));
    programs.push_back(program({{CL_BRIGHTNESS, 1.2f}, {CL_CONTRAST, 0.8f}, {CL_COLOR, 1.3f}, {CL_HUE, 213.f}}));
    programs.push_back(program({{CL_HUE, 213.f}, {CL_COLOR, 1.3f}, {CL_BRIGHTNESS, 1.2f}, {CL_CONTRAST, 0.8f}}));
    programs.push_back(program({{CL_SHARPNESS, 0.37f}, {CL_SHARPNESS, 1.9f}, {CL_HUE, 1.f}, {CL_SHARPNESS, 256.f}}));
    const uint32_t widths[] = {1, 2, 3, 5, 33, 4, 6, 7, 64};
    size_t runs = 0;
    for (uint32_t rows : {1u, 2u, 3u, 0u})
        for (uint32_t w : widths) {
            const uint32_t K = rows ? rows : 5u;  // (as many as LDS holds: every one of these images is one strip)
            for (uint32_t h : {K, K + 1u, 2u * K, 2u * K + 1u, 3u * K + 2u})
                for (size_t k = 0; k < programs.size(); k++) run(w, h, programs[k], kLanes[(k + h + runs++) % 3], rows, (uint32_t)((k + w) % 3));
        }
    // rows longer than a turn of the lanes, and the widest image in strips of as many rows as LDS holds (six) and of four
    for (uint32_t k = 0; k < 3; k++) run(400, 9, programs[k], kLanes[k], k, k);
    run(CL_MAX_SIDE, 15, programs[3], CL_NT, 0u, 0u);
    run(CL_MAX_SIDE, 9, programs[10], 192u, 4u, 1u);
    if (failures) fprintf(stderr, "%d checks failed\n", failures);
    else printf("colour_pixel_asan: ok\n");
    return failures ? 1 : 0;
}
