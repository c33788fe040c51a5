// colour_pixel_band.hpp — the colour operations that are not tables: HUE and SHARPNESS, ids from CL_PIXEL_OPS on, in
// the same program walk as the table operations of colour_band.hpp, in place on the image's u8 pixels.
//   HUE        value: a shift 0..255.  Per pixel (h, s, v) = rgb2hsv(r, g, b); h = (h + shift) & 255; hsv2rgb — Pillow's convert("HSV") and
//              back, torchvision's adjust_hue on a PIL image.  Shift 0 is the lossy round trip, not the identity.  The arithmetic is
//              Pillow's mix of float32 and double, every written operation rounded once (cl_hue_pixel below states it).
//   SHARPNESS  value: a factor 0..256.  blend(SMOOTH(P), P, f) per channel byte (ImageEnhance.Sharpness): SMOOTH is the 3 x 3 filter
//              (1 1 1, 1 5 1, 1 1 1) / 13 in float32, the outermost row and column on every side copied — an image with w < 3 or h < 3
//              stays as it is.
// HUE is one pass shaped like COLOR's (three dwords: four pixels; the pixels behind the last whole group are lane 0's).  SHARPNESS reads
// neighbours, so it cannot run in place pixel by pixel: the workgroup walks the image in strips of K rows through LDS.  The strip buffer
// is a ring of K + 2 rows (row y in slot y mod (K + 2), a pitch of whole dwords): "load strip s" brings the ORIGINAL bytes of the rows the
// ring does not hold yet — the rows behind the strip's first down to the row below its last, which nothing has overwritten in global
// memory yet; the strip's first row and the row above it are still there from strip s - 1, whose stores have overwritten them in global
// memory — and "compute strip s" writes the strip's rows from LDS over the image.  Every step count depends on w, h and K alone, and
// the caller puts a barrier behind every step, as behind the phases of a table operation.
//
// Lanes read LDS in aligned dwords, consecutive lanes consecutive dwords (three per row of the neighbourhood: the bytes c - 3 .. c + 6
// of the four outputs at c .. c + 3), and write the image in whole dwords where the row starts on one (3 w a multiple of 4: 224, 2048),
// else byte by byte.
#pragma once
#include "colour_band.hpp"

namespace jpgpu {

constexpr uint32_t CL_STRIP_BYTES = 48u * 1024u;  // the strip ring of SHARPNESS in LDS
constexpr uint32_t CL_MAX_SIDE = 2048u;           // the greatest width and height of an image of the colour launch

// Rows of a strip: as many as the ring holds beside the row above and the row below, at least 1; `forced` (JPGPU_CL_STRIP_ROWS; 0: none)
// takes fewer.  w <= CL_MAX_SIDE: K >= 6.
JP_CL_BOTH inline uint32_t cl_row_pitch(uint32_t w) { return (3u * w + 3u) & ~3u; }
JP_CL_BOTH inline uint32_t cl_strip_rows(uint32_t w, uint32_t forced) {
    const uint32_t fit = CL_STRIP_BYTES / cl_row_pitch(w), most = fit > 3u ? fit - 2u : 1u;
    return forced && forced < most ? forced : most;
}
// Steps of SHARPNESS: a load and a compute per strip; none for an image without an interior
JP_CL_BOTH inline uint32_t sharp_steps(uint32_t w, uint32_t h, uint32_t K) { return (w < 3u || h < 3u) ? 0u : 2u * ((h + K - 1u) / K); }
// Steps of operation `op` of a program: the four phases of a table operation, HUE's one pass, SHARPNESS's strips
JP_CL_BOTH inline uint32_t cl_op_steps(uint32_t op, uint32_t w, uint32_t h, uint32_t K) {
    return op == CL_HUE ? 1u : op == CL_SHARPNESS ? sharp_steps(w, h, K) : CL_PHASES;
}

JP_CL_BOTH inline uint32_t cl_clip8(int32_t v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// Pillow's rgb2hsv (Convert.c): h and s of a pixel, v = max(r, g, b).  "f32": rounded to float32 once per operation; the divisions are
// IEEE's, correctly rounded (hipcc's default for a / b on the device: v_div_scale / v_div_fmas / v_div_fixup).
JP_CL_BOTH inline void cl_rgb2hsv(uint32_t r, uint32_t g, uint32_t b, uint32_t &h, uint32_t &s, uint32_t &v) {
    const uint32_t mx = r > g ? (r > b ? r : b) : (g > b ? g : b), mn = r < g ? (r < b ? r : b) : (g < b ? g : b);
    v = mx, h = 0u, s = 0u;
    if (mx == mn) return;
    const float cr = (float)(mx - mn);
    const float fs = cr / (float)mx;
    const float rc = (float)(mx - r) / cr, gc = (float)(mx - g) / cr, bc = (float)(mx - b) / cr;
    float hh;
    if (r == mx) hh = cl_addf(bc, -gc);
    else if (g == mx) hh = (float)cl_addd(cl_addd(2.0, (double)rc), -(double)bc);
    else hh = (float)cl_addd(cl_addd(4.0, (double)gc), -(double)rc);
    const double x = cl_addd((double)hh / 6.0, 1.0);  // in [5/6, 11/6]: fmod(x, 1.0) is x - floor(x), exact
    hh = (float)cl_addd(x, -floor(x));
    h = cl_clip8((int32_t)cl_muld((double)hh, 255.0));
    s = cl_clip8((int32_t)cl_muld((double)fs, 255.0));
}
// C's round for x >= 0: halves away from zero (x - floor(x) is exact)
JP_CL_BOTH inline int32_t cl_round_pos(double x) {
    const double fl = floor(x);
    return (int32_t)fl + (cl_addd(x, -fl) >= 0.5 ? 1 : 0);
}
// Pillow's hsv2rgb -> r | g << 8 | b << 16
JP_CL_BOTH inline uint32_t cl_hsv2rgb(uint32_t h, uint32_t s, uint32_t v) {
    if (s == 0u) return v * 0x010101u;
    const double x = cl_muld((double)(float)h, 6.0) / 255.0;
    const double fl = floor(x);
    const uint32_t i = (uint32_t)(int32_t)fl;
    const float f = (float)cl_addd(x, -(double)(float)fl);
    const float fs = (float)((double)(float)s / 255.0);
    const double vd = (double)v;
    const uint32_t p = cl_clip8(cl_round_pos(cl_muld(vd, cl_addd(1.0, -(double)fs))));
    const uint32_t q = cl_clip8(cl_round_pos(cl_muld(vd, cl_addd(1.0, -(double)cl_mulf(fs, f)))));
    const uint32_t t = cl_clip8(cl_round_pos(cl_muld(vd, cl_addd(1.0, -cl_muld((double)fs, cl_addd(1.0, -(double)f))))));
    switch (i % 6u) {
    case 0: return v | (t << 8) | (p << 16);
    case 1: return q | (v << 8) | (p << 16);
    case 2: return p | (v << 8) | (t << 16);
    case 3: return p | (q << 8) | (v << 16);
    case 4: return t | (p << 8) | (v << 16);
    default: return v | (p << 8) | (q << 16);
    }
}
// HUE of one pixel -> r | g << 8 | b << 16
JP_CL_BOTH inline uint32_t cl_hue_pixel(uint32_t r, uint32_t g, uint32_t b, uint32_t shift) {
    uint32_t h, s, v;
    cl_rgb2hsv(r, g, b, h, s, v);
    return cl_hsv2rgb((h + shift) & 255u, s, v);
}

// SMOOTH at an interior byte: its row below (a), its own row (m), its row above (b), each the left, the middle and the right pixel's
// value of the channel; Pillow's order of the float32 sums
JP_CL_BOTH inline uint32_t cl_smooth_value(const uint32_t a[3], const uint32_t m[3], const uint32_t b[3]) {
    const float k1 = (float)(1.0 / 13), k5 = (float)(5.0 / 13);
    float ss = 0.5f;
    ss = cl_addf(ss, cl_addf(cl_addf(cl_mulf((float)a[0], k1), cl_mulf((float)a[1], k1)), cl_mulf((float)a[2], k1)));
    ss = cl_addf(ss, cl_addf(cl_addf(cl_mulf((float)m[0], k1), cl_mulf((float)m[1], k5)), cl_mulf((float)m[2], k1)));
    ss = cl_addf(ss, cl_addf(cl_addf(cl_mulf((float)b[0], k1), cl_mulf((float)b[1], k1)), cl_mulf((float)b[2], k1)));
    return cl_clip8((int32_t)ss);
}

#ifdef JPGPU_CL_DEVICE_BODY
// What a workgroup keeps in LDS beside ColourLds: the strip ring of SHARPNESS
struct ColourStripLds {
    uint32_t ring[CL_STRIP_BYTES / 4u];
};

template <uint32_t NT>
struct CPixelBand {
    typedef CBand<NT> B;

    // HUE: the image through the round trip, four pixels in three dwords per lane and turn
    static __device__ __forceinline__ void hue(const ColourJob &j, const ColourOp &o, uint32_t tid) {
        const uint32_t npx = j.w * j.h, shift = (uint32_t)o.value & 255u;
        JP_GLOBAL uint8_t *pb = (JP_GLOBAL uint8_t *)j.pix;
        JP_GLOBAL uint32_t *pd = (JP_GLOBAL uint32_t *)j.pix;
        for (uint32_t g = tid; g < npx / 4u; g += NT) {
            const uint32_t d[3] = {pd[3u * g], pd[3u * g + 1u], pd[3u * g + 2u]};
            uint64_t lo = 0u, hi = 0u;  // (bytes 0..7 and 4..11 of the twelve)
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) {
                uint32_t r, gg, b;
                B::unpack4(d, k, r, gg, b);
                const uint64_t p = (uint64_t)cl_hue_pixel(r, gg, b, shift);
                if (k < 2u) lo |= p << (24u * k);
                else hi |= p << (24u * k - 32u);
            }
            pd[3u * g] = (uint32_t)lo;
            pd[3u * g + 1u] = (uint32_t)(lo >> 32) | (uint32_t)hi;
            pd[3u * g + 2u] = (uint32_t)(hi >> 32);
        }
        if (tid == 0u)
            for (uint32_t p = npx & ~3u; p < npx; p++) {
                const uint32_t c = cl_hue_pixel(pb[3u * p], pb[3u * p + 1u], pb[3u * p + 2u], shift);
                pb[3u * p] = (uint8_t)c, pb[3u * p + 1u] = (uint8_t)(c >> 8), pb[3u * p + 2u] = (uint8_t)(c >> 16);
            }
    }

    // SHARPNESS, "load strip s": the original bytes of rows lo .. hi (the rows the ring does not hold yet) out of the image
    static __device__ __forceinline__ void sharp_load(const ColourJob &j, uint32_t s, uint32_t K, uint32_t tid, ColourStripLds &sl) {
        const uint32_t rb = 3u * j.w, pd4 = cl_row_pitch(j.w) / 4u, R = K + 2u;
        const uint32_t lo = s == 0u ? 0u : s * K + 1u, hi = min(s * K + K, j.h - 1u);
        if (lo > hi) return;
        const JP_GLOBAL uint8_t *pb = (const JP_GLOBAL uint8_t *)j.pix;
        const JP_GLOBAL uint32_t *pd = (const JP_GLOBAL uint32_t *)j.pix;
        const uint32_t items = (hi - lo + 1u) * pd4;
        for (uint32_t i = tid; i < items; i += NT) {
            const uint32_t y = lo + i / pd4, q = i % pd4, c = 4u * q, g = rb * y + c;
            uint32_t d = 0u;
            if ((g & 3u) == 0u && c + 4u <= rb) {
                d = pd[g >> 2];
            } else {
#pragma unroll
                for (uint32_t b = 0; b < 4u; b++)
                    if (c + b < rb) d |= (uint32_t)pb[g + b] << (8u * b);
            }
            sl.ring[(y % R) * pd4 + q] = d;
        }
    }

    // SHARPNESS, "compute and store strip s": rows s K .. s K + K - 1 of the image from the ring.  The first and the last row of the
    // image stay as they are; so do the first and the last pixel of every row.
    static __device__ __forceinline__ void sharp_compute(const ColourJob &j, const ColourOp &o, uint32_t s, uint32_t K, uint32_t tid, const ColourStripLds &sl) {
        const uint32_t rb = 3u * j.w, pd4 = cl_row_pitch(j.w) / 4u, R = K + 2u;
        const uint32_t lo = max(s * K, 1u), hi = min(s * K + K, j.h - 1u);  // (rows lo .. hi - 1)
        if (lo >= hi) return;
        const float f = o.value;
        JP_GLOBAL uint8_t *pb = (JP_GLOBAL uint8_t *)j.pix;
        JP_GLOBAL uint32_t *pd = (JP_GLOBAL uint32_t *)j.pix;
        const uint32_t items = (hi - lo) * pd4;
        for (uint32_t i = tid; i < items; i += NT) {
            const uint32_t y = lo + i / pd4, q = i % pd4, c = 4u * q, g = rb * y + c;
            const uint32_t qm = q ? q - 1u : 0u, qp = q + 1u < pd4 ? q + 1u : q;  // (their bytes are read for interior bytes alone)
            // rows y + 1, y, y - 1: the twelve bytes c - 4 .. c + 7 of each
            uint32_t n[3][3];
#pragma unroll
            for (uint32_t k = 0; k < 3u; k++) {
                const uint32_t base = ((y + 1u - k) % R) * pd4;
                n[k][0] = sl.ring[base + qm], n[k][1] = sl.ring[base + q], n[k][2] = sl.ring[base + qp];
            }
            uint32_t out = 0u;
#pragma unroll
            for (uint32_t b = 0; b < 4u; b++) {
                const uint32_t mid = B::byte_of(n[1][1], b);
                uint32_t v = mid;
                if (c + b >= 3u && c + b + 3u < rb) {  // (neither the row's first pixel nor its last)
                    uint32_t t[3][3];
#pragma unroll
                    for (uint32_t k = 0; k < 3u; k++) {  // (byte e of the twelve: byte e & 3 of dword e >> 2; left b + 1, middle b + 4, right b + 7)
                        t[k][0] = B::byte_of(n[k][(b + 1u) >> 2], (b + 1u) & 3u);
                        t[k][1] = B::byte_of(n[k][1], b);
                        t[k][2] = B::byte_of(n[k][(b + 7u) >> 2], (b + 7u) & 3u);
                    }
                    v = cl_blend(cl_smooth_value(t[0], t[1], t[2]), mid, f);
                }
                out |= v << (8u * b);
            }
            if ((g & 3u) == 0u && c + 4u <= rb) {
                pd[g >> 2] = out;
            } else {
#pragma unroll
                for (uint32_t b = 0; b < 4u; b++)
                    if (c + b < rb) pb[g + b] = (uint8_t)(out >> (8u * b));
            }
        }
    }

    // Lane tid's share of step `step` (of cl_op_steps) of operation k of the job; K: cl_strip_rows.  The caller puts a barrier behind
    // every step.  A table operation's steps are CBand's phases.
    static __device__ __forceinline__ void step(const ColourJob &j, uint32_t k, uint32_t step, uint32_t K, const JP_GLOBAL double *scale, uint32_t tid, ColourLds &l,
                                                ColourStripLds &sl) {
        const uint32_t op = j.prog.ops[k].op;
        if (op == CL_HUE) hue(j, j.prog.ops[k], tid);
        else if (op == CL_SHARPNESS) {
            if (step & 1u) sharp_compute(j, j.prog.ops[k], step >> 1, K, tid, sl);
            else sharp_load(j, step >> 1, K, tid, sl);
        } else B::phase(j, k, step, scale, tid, l);
    }
};
#endif  // JPGPU_CL_DEVICE_BODY

}  // namespace jpgpu
