// batch_output.hpp — the fixed-output stage of a batch stated once: its options as one record, the rules that
// refuse a combination, the placement normalisation, the bytes an image takes in the stage's arenas, and the route — which launches
// run.  batch.cpp, batch_output.cpp and pipeline.cpp share it.  No HIP dependency (tests/emu/emu_batch_output.cpp runs it on the CPU).
#pragma once
#include <string.h>

#include "batch_layout.hpp"
#include "colour_band.hpp"
#include "orient_band.hpp"
#include "placed_band.hpp"
#include "resample_band.hpp"
#include "tensor_band.hpp"
#include "warp_band.hpp"

namespace jpgpu {

// What a batch is created with beyond its images, windows and placements.  An absent option holds its zero value.
struct OutputSpec {
    uint32_t w = 0, h = 0;              // the output size (0 x 0: none)
    uint32_t filter = 0;                // JPGPU_FILTER_* (0: bilinear)
    bool rgb = false;                   // JPGPU_BATCH_RGB_OUTPUT
    bool tensor = false;                // a tensor format ...
    jpgpu_tensor_format tn{};           // ... and which
    uint8_t fill[4] = {0, 0, 0, 0};     // what a placement leaves uncovered
    bool warp = false;                  // warp options ...
    jpgpu_warp_options wp{};            // ... and which
    bool orient = false;                // some image has an EXIF orientation other than 1 (jpgpu_batch_create_oriented)
    bool colour = false;                // colour options (jpgpu_batch_create_coloured): a program of colour operations per image
    bool sized() const { return w != 0 || h != 0; }
    uint32_t elem_bytes() const { return tensor ? tensor_elem_bytes(tn.dtype) : 1u; }
    uint32_t channels(uint32_t ncomp) const { return rgb ? 3u : ncomp; }
};
inline bool operator==(const OutputSpec &a, const OutputSpec &b) {
    return a.w == b.w && a.h == b.h && a.filter == b.filter && a.rgb == b.rgb && a.tensor == b.tensor && a.tn.dtype == b.tn.dtype &&
           a.tn.reserved == b.tn.reserved && memcmp(a.tn.mean, b.tn.mean, sizeof a.tn.mean) == 0 && memcmp(a.tn.std, b.tn.std, sizeof a.tn.std) == 0 &&
           memcmp(a.fill, b.fill, 4) == 0 && a.warp == b.warp && a.wp.filter == b.wp.filter && memcmp(a.wp.fill, b.wp.fill, 4) == 0 &&
           a.wp.reserved == b.wp.reserved && a.orient == b.orient && a.colour == b.colour;
}
inline uint32_t pack_fill(const uint8_t f[4]) { return (uint32_t)f[0] | ((uint32_t)f[1] << 8) | ((uint32_t)f[2] << 16) | ((uint32_t)f[3] << 24); }

// The rules of the options among themselves, before a device is touched.  A filter or RGB output without an output size is
// JPGPU_ERR_UNSUPPORTED, everything else JPGPU_ERR_FORMAT; the reason in `why`.
inline int output_rule(const OutputSpec &s, std::string &why) {
    char msg[240];
    const auto no = [&](int code, const char *fmt, uint32_t a, uint32_t b, uint32_t c = 0) { return snprintf(msg, sizeof msg, fmt, a, b, c), why = msg, code; };
    if (s.sized() && (s.w == 0 || s.h == 0 || s.w > RS_MAX_OUT || s.h > RS_MAX_OUT))
        return no(JPGPU_ERR_FORMAT, "output size %ux%u: width and height must be 1..%u", s.w, s.h, RS_MAX_OUT);
    if (s.filter >= RS_FILTERS) return no(JPGPU_ERR_FORMAT, "resample filter %u: the ids are 0..%u (JPGPU_FILTER_*)", s.filter, RS_FILTERS - 1u);
    if (s.filter && !s.sized()) return why = std::string("a resample filter (") + resample_filter_name(s.filter) + ") needs an output size", JPGPU_ERR_UNSUPPORTED;
    if (s.rgb && !s.sized()) return why = "RGB output (JPGPU_BATCH_RGB_OUTPUT) needs an output size", JPGPU_ERR_UNSUPPORTED;
    if (s.orient && !s.sized()) return why = "EXIF orientations need an output size", JPGPU_ERR_UNSUPPORTED;
    if (s.colour && !s.sized()) return why = "colour operations need an output size", JPGPU_ERR_UNSUPPORTED;
    if (s.warp && !s.sized()) return why = "a warp needs an output size", JPGPU_ERR_FORMAT;
    if (s.warp && (s.wp.filter > WP_BILINEAR || s.wp.reserved != 0))
        return no(JPGPU_ERR_FORMAT, "warp options: filter %u, reserved %u (JPGPU_WARP_NEAREST or JPGPU_WARP_BILINEAR, reserved 0)", s.wp.filter, s.wp.reserved);
    if (s.tensor && !s.sized()) return why = "a tensor format needs an output size", JPGPU_ERR_FORMAT;
    if (s.tensor && (tensor_elem_bytes(s.tn.dtype) == 0 || s.tn.reserved != 0))
        return no(JPGPU_ERR_FORMAT, "tensor format: dtype %u, reserved %u (dtype must be 1..3, reserved 0)", s.tn.dtype, s.tn.reserved);
    return JPGPU_OK;
}
// The rules of the options against one image of `ncomp` components.  Its tensor format's means and stds against its channels (no device
// is needed for that: batch_create asks first); then all of them, under the colour function `color_fn` (ImageJob::color_fn).
inline int output_tensor_rule(const OutputSpec &s, uint32_t ncomp, std::string &why) {
    const char *bad = nullptr;
    if (s.tensor && !tensor_format_ok(s.tn.dtype, s.tn.reserved, s.tn.mean, s.tn.std, s.channels(ncomp), bad)) return why = std::string("tensor format: ") + bad, JPGPU_ERR_FORMAT;
    return JPGPU_OK;
}
inline int output_image_rule(const OutputSpec &s, uint32_t ncomp, uint32_t color_fn, std::string &why) {
    if (s.sized() && color_fn == CC_NONE && ncomp > 1)
        return why = "no output size for planar output (ColorTransform None with more than one component)", JPGPU_ERR_UNSUPPORTED;
    if (s.rgb && ncomp != 1 && ncomp != 3 && ncomp != 4) return why = "no RGB output for " + std::to_string(ncomp) + " components", JPGPU_ERR_UNSUPPORTED;
    return output_tensor_rule(s, ncomp, why);
}

// Placements as a batch keeps them: "none" (rw == 0 or rh == 0) written out as the whole w x h output; `placed`: one differs from the
// whole output.  Returns n, or the index of the first image whose placement shows no pixel (`out` is then of no use).
inline uint32_t normalise_placements(const jpgpu_placement *pls, uint32_t n, uint32_t w, uint32_t h, std::vector<jpgpu_placement> &out, bool &placed) {
    out.assign(pls, pls + n);
    placed = false;
    for (uint32_t i = 0; i < n; i++) {
        jpgpu_placement &pl = out[i];
        if (pl.rw == 0 || pl.rh == 0) pl = jpgpu_placement{(uint16_t)w, (uint16_t)h, 0, 0};
        uint32_t first, count, v0;
        if (!placed_axis(pl.rw, pl.x, w, first, count, v0) || !placed_axis(pl.rh, pl.y, h, first, count, v0)) return i;
        placed = placed || pl.rw != w || pl.rh != h || pl.x != 0 || pl.y != 0;
    }
    return n;
}

// The orientations of a call (NULL: none) against the rule: n, or the index of the first value outside 1..8; `any`: one is not 1.
inline uint32_t check_orientations(const uint8_t *o, uint32_t n, bool &any) {
    any = false;
    for (uint32_t i = 0; o && i < n; i++) {
        if (!orient_valid(o[i])) return i;
        any = any || o[i] != 1u;
    }
    return n;
}
// The window `wn` of image d's ORIENTED output under orientation o, as the window of its output that the pixel routes decode.
// JPGPU_ERR_FORMAT with the reason in `why` for one outside the oriented image.
inline int orient_window_rule(const jpgpu_image_desc &d, uint32_t o, jpgpu_window &wn, std::string &why) {
    uint32_t gw = 0, gh = 0, sx, sy, sw, sh;
    window_grid(d.components, d.ncomp, d.out_w, d.out_h, gw, gh);
    if (!orient_source_window(o, gw, gh, wn.x, wn.y, wn.w, wn.h, sx, sy, sw, sh)) {
        char msg[200];
        snprintf(msg, sizeof msg, "window (%u, %u) %ux%u outside the oriented %ux%u image (orientation %u)", wn.x, wn.y, wn.w, wn.h, orient_swaps(o) ? gh : gw,
                 orient_swaps(o) ? gw : gh, o);
        return why = msg, JPGPU_ERR_FORMAT;
    }
    wn = jpgpu_window{(uint16_t)sx, (uint16_t)sy, (uint16_t)sw, (uint16_t)sh};
    return JPGPU_OK;
}

// Bytes of one image of `ncomp` components in the output arena, or (`u8`) in the arena a warp reads: what the u8 batch's output would be.
inline size_t output_image_bytes(const OutputSpec &s, uint32_t ncomp, bool u8 = false) {
    return (size_t)s.w * s.h * s.channels(ncomp) * (u8 ? 1u : s.elem_bytes());
}
// ... of every image, laid out as an arena (batch_layout.hpp).  The intermediate arena is what the batch lays out without an output size.
inline size_t output_arena(const OutputSpec &s, const std::vector<jpgpu_image_desc> &descs, bool u8, std::vector<size_t> &off, std::vector<size_t> &len) {
    std::vector<size_t> lens(descs.size());
    for (size_t i = 0; i < descs.size(); i++) lens[i] = output_image_bytes(s, descs[i].ncomp, u8);
    return arena_layout(lens, off, len);
}

// The C ABI's program as the kernels' record (the same layout, field by field)
inline ColourProgram as_program(const jpgpu_colour_program &p) {
    ColourProgram q{};
    q.n = p.n;
    for (uint32_t k = 0; k < CL_MAX_OPS && k < p.n; k++) q.ops[k] = ColourOp{p.ops[k].op, p.ops[k].value};
    return q;
}
// A colour program against the image it is meant for: a refused program (colour_program_check) is JPGPU_ERR_FORMAT, a non-empty one on
// an image whose output has another channel count than three JPGPU_ERR_UNSUPPORTED; the reason in `why`.
inline int colour_program_rule(const OutputSpec &s, uint32_t ncomp, const ColourProgram &p, std::string &why) {
    if (!colour_program_check(p))
        return why = "colour program refused (at most 4 operations; factors 0..256; SOLARIZE 0..256, POSTERIZE 1..8 and HUE 0..255 in integers: jpgpu_colour_check)", JPGPU_ERR_FORMAT;
    if (p.n != 0 && s.channels(ncomp) != 3u)
        return why = "colour operations need three output channels (this image has " + std::to_string(s.channels(ncomp)) + "; RGB output gives three)", JPGPU_ERR_UNSUPPORTED;
    return JPGPU_OK;
}

// The route: whether the orientation launch runs in front, which resample launch runs, whether the launch of runs of bands goes beside
// it, whether the colour launch follows, whether a warp launch finishes.  Allocation, job upload and launch switch on it.  A coloured
// batch always finishes through the warp launch — with identity matrices when it has no warp options (rule N-sep copies exactly and
// applies the flip and the tensor table).
enum class Resample : uint8_t { None, Band, Tensor, Placed, PlacedTensor };
struct OutputRoute {
    Resample resample = Resample::None;
    bool orient = false, runs = false, colour = false, warp = false;
    bool tensor_jobs() const { return resample == Resample::Tensor || resample == Resample::PlacedTensor; }
};
inline OutputRoute output_route(const OutputSpec &s, bool placed, uint32_t max_runs) {
    OutputRoute r;
    if (!s.sized()) return r;
    r.colour = s.colour, r.warp = s.warp || s.colour, r.orient = s.orient;
    const bool tensor = s.tensor && !s.warp && !s.colour;  // (a warped or coloured batch resamples to u8, whatever it writes in the end)
    r.resample = placed ? (tensor ? Resample::PlacedTensor : Resample::Placed) : (tensor ? Resample::Tensor : Resample::Band);
    r.runs = max_runs != 0 && !placed;
    return r;
}

}  // namespace jpgpu
