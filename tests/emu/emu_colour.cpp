// emu_colour.cpp — TEST-ONLY CPU emulation of the colour kernel (csrc/colour_band.hpp, csrc/colour.hip): the product's job builder and
// the workgroup of one image, phase by phase as the kernel walks them — every lane's share of a phase, then the barrier — lane by lane.
// Built by tests/test_workgroup_colour.py (g++, -ffp-contract=off) and, with its own main, by the stand-alone sanitizer program
// tests/emu/colour_asan.cpp.
#include "hip_shim.hpp"
#include <vector>
#include "../../jpeg-decoder_amd/csrc/colour_band.hpp"

using namespace jpgpu;

template <uint32_t NT>
static void emu_workgroup(const ColourJob &j, const double *scale) {
    ColourLds lds;
    memset(&lds, 0xA5, sizeof lds);  // (LDS holds anything at launch)
    const uint32_t n = min(j.prog.n, CL_MAX_OPS);
    for (uint32_t k = 0; k < n; k++)
        for (uint32_t phase = 0; phase < CL_PHASES; phase++)
            for (uint32_t tid = 0; tid < NT; tid++) CBand<NT>::phase(j, k, phase, scale, tid, lds);  // (the barrier: the loop's end)
}

extern "C" {

// The image of w x h x 3 bytes at `pix` (4-byte aligned) through `prog`, in place, by a workgroup of `lanes` lanes (CL_NT, or 64 and
// 192: other strides through the same bodies).  0, or -1 for a refused program or lane count.
int emu_colour(uint8_t *pix, uint32_t w, uint32_t h, const ColourProgram *prog, uint32_t lanes) {
    if (!prog || !colour_program_check(*prog)) return -1;
    ColourJob j{};
    colour_job(j, pix, w, h, prog);
    double scale[256];
    colour_scale_table(scale);
    if (lanes == CL_NT) emu_workgroup<CL_NT>(j, scale);
    else if (lanes == 64u) emu_workgroup<64u>(j, scale);
    else if (lanes == 192u) emu_workgroup<192u>(j, scale);
    else return -1;
    return 0;
}

int emu_colour_check(const ColourProgram *prog) { return prog && colour_program_check(*prog) ? 0 : -1; }

}  // extern "C"
