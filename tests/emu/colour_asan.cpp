// colour_asan.cpp — TEST-ONLY stand-alone program: the colour stage's job builder, its refusal rule and the emulated workgroup of the
// colour kernel (emu_colour.cpp) under AddressSanitizer + UBSan, over small images whose byte counts leave every remainder behind the
// whole dwords and the groups of four pixels, every operation alone and programs of up to four, at three lane counts.  The image is
// allocated exactly: a byte beyond it is a report.  Built and run by tests/test_workgroup_colour.py:
//   g++ -fsanitize=address,undefined ... -ffp-contract=off -include hip_shim.hpp colour_asan.cpp      exit code 0 = no report, every check held
#include "emu_colour.cpp"

#include <cmath>
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

const uint32_t kSizes[][2] = {{1, 1}, {2, 1}, {3, 1}, {1, 5}, {7, 1}, {16, 16}, {33, 17}, {8, 8}, {2048, 2}, {5, 300}, {64, 65}};
const uint32_t kLanes[] = {CL_NT, 64u, 192u};

ColourProgram program(std::initializer_list<ColourOp> ops) {
    ColourProgram p{};
    for (const ColourOp &o : ops) p.ops[p.n++] = o;
    return p;
}

// a scalar statement of the operations, pixel by pixel, out of the header's value functions
void reference(std::vector<uint8_t> &px, uint32_t w, uint32_t h, const ColourProgram &p) {
    const uint32_t npx = w * h;
    double scale[256];
    colour_scale_table(scale);
    for (uint32_t k = 0; k < p.n; k++) {
        const ColourOp o = p.ops[k];
        uint32_t hist[3][256] = {};
        uint32_t sum = 0;
        for (uint32_t i = 0; i < npx; i++) {
            for (uint32_t c = 0; c < 3; c++) hist[c][px[3 * i + c]]++;
            sum += cl_luma(px[3 * i], px[3 * i + 1], px[3 * i + 2]);
        }
        for (uint32_t i = 0; i < npx; i++) {
            const uint32_t y = cl_luma(px[3 * i], px[3 * i + 1], px[3 * i + 2]);
            for (uint32_t c = 0; c < 3; c++) {
                const uint32_t v = px[3 * i + c];
                uint32_t lo, hi, out;
                if (o.op == CL_COLOR) out = cl_blend(y, v, o.value);
                else if (o.op == CL_AUTOCONTRAST) cl_hist_range(hist[c], lo, hi), out = cl_autocontrast_value(lo, hi, hi > lo ? scale[hi - lo] : 0.0, v);
                else if (o.op == CL_EQUALIZE) out = cl_equalize_value(hist[c], v);
                else out = cl_point_value(o.op, o.value, cl_mean(sum, npx), v);
                px[3 * i + c] = (uint8_t)out;
            }
        }
    }
}

void run(uint32_t w, uint32_t h, const ColourProgram &p, uint32_t lanes, uint32_t kind) {
    const size_t n = (size_t)w * h * 3;
    uint8_t *pix = (uint8_t *)malloc(n);  // (exactly the image)
    uint32_t s = 7u + w * 31u + h + kind;
    for (size_t i = 0; i < n; i++) {
        s = s * 1664525u + 1013904223u;
        pix[i] = kind == 0 ? (uint8_t)(s >> 24) : kind == 1 ? (uint8_t)(40u + ((s >> 24) % 90u)) : (uint8_t)(i % 3u == 0 ? 9u : 200u);  // (random, narrow, constant)
    }
    std::vector<uint8_t> want(pix, pix + n);
    reference(want, w, h, p);
    const int rc = emu_colour(pix, w, h, &p, lanes);
    CHECK(rc == 0, "refused");
    size_t bad = 0;
    for (size_t i = 0; i < n; i++) bad += pix[i] != want[i];
    CHECK(bad == 0, "%zu bytes differ: %ux%u lanes %u kind %u, first op %u of %u", bad, w, h, lanes, kind, p.ops[0].op, p.n);
    free(pix);
}

void refusals() {
    const float nan = std::nanf(""), inf = INFINITY;
    const ColourOp bad[] = {{9u, 0.f},          {CL_BRIGHTNESS, nan}, {CL_CONTRAST, inf},   {CL_COLOR, -0.5f},     {CL_BRIGHTNESS, 256.5f}, {CL_SOLARIZE, 1.5f},
                            {CL_SOLARIZE, 257.f}, {CL_SOLARIZE, -1.f},  {CL_POSTERIZE, 0.f},  {CL_POSTERIZE, 9.f},   {CL_POSTERIZE, 2.5f},    {CL_POSTERIZE, nan}};
    for (const ColourOp &o : bad) {
        const ColourProgram p = program({{CL_INVERT, 0.f}, o});
        CHECK(emu_colour_check(&p) != 0, "accepted op %u value %g", o.op, o.value);
        uint8_t px[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
        CHECK(emu_colour(px, 2, 2, &p, CL_NT) != 0 && px[0] == 1, "a refused program wrote");
    }
    ColourProgram five = program({{CL_INVERT, 0.f}, {CL_INVERT, 0.f}, {CL_INVERT, 0.f}, {CL_INVERT, 0.f}});
    five.n = 5;
    CHECK(emu_colour_check(&five) != 0, "five operations accepted");
    const ColourProgram ok = program({{CL_BRIGHTNESS, 256.f}, {CL_SOLARIZE, 256.f}, {CL_POSTERIZE, 8.f}, {CL_AUTOCONTRAST, nan}});
    CHECK(emu_colour_check(&ok) == 0, "the bounds refused");
    CHECK(emu_colour_check(nullptr) != 0, "no program accepted");
}

}  // namespace

int main() {
    refusals();
    std::vector<ColourProgram> programs;
    for (uint32_t op = 0; op < CL_OPS; op++)
        for (float v : {0.f, 1.f, 0.37f, 1.9f, 8.f, 128.f, 256.f})
            if (colour_op_check(op, v)) programs.push_back(program({{op, v}}));
    programs.push_back(program({}));
    programs.push_back(program({{CL_BRIGHTNESS, 1.9f}, {CL_AUTOCONTRAST, 0.f}}));
    programs.push_back(program({{CL_COLOR, 0.37f}, {CL_EQUALIZE, 0.f}, {CL_CONTRAST, 1.9f}}));
    programs.push_back(program({{CL_SOLARIZE, 128.f}, {CL_CONTRAST, 0.37f}, {CL_COLOR, 0.f}, {CL_AUTOCONTRAST, 0.f}}));
    programs.push_back(program({{CL_EQUALIZE, 0.f}, {CL_INVERT, 0.f}, {CL_EQUALIZE, 0.f}, {CL_COLOR, 1.9f}}));
    for (auto &sz : kSizes)
        for (size_t k = 0; k < programs.size(); k++)
            for (uint32_t kind = 0; kind < 3; kind++) run(sz[0], sz[1], programs[k], kLanes[(k + kind) % 3], kind);
    if (failures) fprintf(stderr, "%d checks failed\n", failures);
    else printf("colour_asan: ok\n");
    return failures ? 1 : 0;
}
