// emu_colour_pixel.cpp — TEST-ONLY CPU emulation of the colour kernel with the operations that are not tables
// (csrc/colour_pixel_band.hpp, csrc/colour.hip): the product's job builder and the workgroup of one image, step by step as the kernel
// walks them — every lane's share of a step, then the barrier — lane by lane.  The strip ring is allocated exactly, on the heap: a read
// or a write beyond it is a report under AddressSanitizer.  Built by tests/test_workgroup_colour_pixel.py (g++, -ffp-contract=off) and,
// with its own main, by the stand-alone sanitizer program tests/emu/colour_pixel_asan.cpp.
#include "hip_shim.hpp"
#include <cstdlib>
#include <vector>
#include "../../jpeg-decoder_amd/csrc/colour_pixel_band.hpp"

using namespace jpgpu;

template <uint32_t NT>
static void emu_pixel_workgroup(const ColourJob &j, const double *scale, uint32_t strip_rows) {
    ColourLds lds;
    ColourStripLds *strip = (ColourStripLds *)malloc(sizeof(ColourStripLds));
    memset(&lds, 0xA5, sizeof lds);  // (LDS holds anything at launch)
    memset(strip, 0xA5, sizeof *strip);
    const uint32_t n = min(j.prog.n, CL_MAX_OPS), K = cl_strip_rows(j.w, strip_rows);
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t steps = cl_op_steps(j.prog.ops[k].op, j.w, j.h, K);
        for (uint32_t step = 0; step < steps; step++)
            for (uint32_t tid = 0; tid < NT; tid++) CPixelBand<NT>::step(j, k, step, K, scale, tid, lds, *strip);  // (the barrier: the loop's end)
    }
    free(strip);
}

extern "C" {

// The image of w x h x 3 bytes at `pix` (4-byte aligned) through `prog`, in place, by a workgroup of `lanes` lanes (CL_NT, or 64 and
// 192: other strides through the same bodies), SHARPNESS in strips of `strip_rows` rows (0: as many as LDS holds).  0, or -1 for a
// refused program, size or lane count.
int emu_colour_pixel(uint8_t *pix, uint32_t w, uint32_t h, const ColourProgram *prog, uint32_t lanes, uint32_t strip_rows) {
    if (!prog || !colour_program_check(*prog) || w == 0 || h == 0 || w > CL_MAX_SIDE || h > CL_MAX_SIDE) return -1;
    ColourJob j{};
    colour_job(j, pix, w, h, prog);
    double scale[256];
    colour_scale_table(scale);
    if (lanes == CL_NT) emu_pixel_workgroup<CL_NT>(j, scale, strip_rows);
    else if (lanes == 64u) emu_pixel_workgroup<64u>(j, scale, strip_rows);
    else if (lanes == 192u) emu_pixel_workgroup<192u>(j, scale, strip_rows);
    else return -1;
    return 0;
}

int emu_colour_pixel_check(const ColourProgram *prog) { return prog && colour_program_check(*prog) ? 0 : -1; }
uint32_t emu_colour_strip_rows(uint32_t w, uint32_t forced) { return cl_strip_rows(w, forced); }
uint32_t emu_colour_sharp_steps(uint32_t w, uint32_t h, uint32_t K) { return sharp_steps(w, h, K); }
// one pixel through HUE -> r | g << 8 | b << 16 (the C++ statement of the float and double arithmetic, alone)
uint32_t emu_colour_hue_pixel(uint32_t r, uint32_t g, uint32_t b, uint32_t shift) { return cl_hue_pixel(r, g, b, shift); }

}  // extern "C"
