// colour_band.hpp — the colour operations behind the fixed output size (jpgpu_batch_create_coloured): every image's u8
// result R of out_w x out_h x 3, as the same batch without colour writes it, goes through a program of at most four Pillow operations, in
// place, before the warp and the tensor table:
//     C = op_{k-1}( ... op_1( op_0( R ) ) )
// Every operation but COLOR is a table of 3 x 256 bytes looked up per channel value, some after a pass of statistics over the CURRENT
// image (CONTRAST: the sum of L; AUTOCONTRAST, EQUALIZE: the histograms); COLOR blends every pixel with its own L.  The arithmetic is
// Pillow's, stated here once for the device, the host functions and the CPU emulation (HUE and SHARPNESS, the operations from id 16 on
// that are not tables, walk the same program by steps of their own: colour_pixel_band.hpp):
//   blend(a, b, f)   IEEE float32, the product and the sum rounded once each (cl_mulf / cl_addf: no fused multiply-add):
//                    t = (float)a + f * (float)(b - a); 0 <= f <= 1: (uint8)(int)t; else t <= 0: 0, t >= 255: 255, else (uint8)(int)t.
//   L(px)            (R 19595 + G 38470 + B 7471 + 0x8000) >> 16                                        (convert("L"))
//   mean             (2 s + n) / (2 n) in integers, s the sum of L over the n pixels                    (int(s / n + 0.5) for n <= 2048^2)
//   AUTOCONTRAST     lo / hi the least / greatest value present; hi <= lo: identity; else in IEEE double, each operation rounded once:
//                    scale = 255.0 / (hi - lo) (a table made on the host), offset = -lo * scale, clamp((int)(i * scale + offset), 0, 255).
//   EQUALIZE         nz the non-zero counts; fewer than two: identity; step = (sum(nz) - nz[last]) / 255; step == 0: identity; else
//                    lut[i] = min((step / 2 + h[0] + .. + h[i-1]) / step, 255).
//
// The kernel: one workgroup of CL_NT lanes per image walks the image's program.  Every operation is four phases with a barrier behind
// each — zero the statistics, accumulate them (LDS atomics), build the table (a lane per entry), apply — and a phase with nothing to do
// for an operation is empty.  Lanes read and write whole dwords of their own (the image's base is 256-byte aligned; COLOR takes three
// dwords: four pixels); the bytes and pixels behind the last whole group are lane 0's.  Counts and sums fit 32 bits up to 2048 x 2048.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__) || defined(JPGPU_HOST_EMULATION)
#define JPGPU_CL_DEVICE_BODY 1
#include "pixel_math.hpp"
#endif

#if defined(__HIP__)
#define JP_CL_BOTH __host__ __device__
#else
#define JP_CL_BOTH
#endif

namespace jpgpu {

// JPGPU_COLOUR_*
constexpr uint32_t CL_IDENTITY = 0, CL_BRIGHTNESS = 1, CL_CONTRAST = 2, CL_COLOR = 3, CL_SOLARIZE = 4, CL_POSTERIZE = 5, CL_INVERT = 6, CL_AUTOCONTRAST = 7,
                   CL_EQUALIZE = 8, CL_OPS = 9;
// Operations from 16 on are not tables (colour_pixel_band.hpp): ids 9..15 and from 18 on are refused
constexpr uint32_t CL_PIXEL_OPS = 16, CL_HUE = 16, CL_SHARPNESS = 17, CL_PIXEL_OPS_END = 18;
constexpr uint32_t CL_MAX_OPS = 4;        // operations of a program
constexpr uint32_t CL_NT = 1024;          // lanes of a workgroup
constexpr uint32_t CL_PHASES = 4;         // zero, accumulate, table, apply
constexpr float CL_MAX_FACTOR = 256.0f;   // the greatest factor admitted: every blend then fits an int

struct ColourOp {  // (jpgpu_colour_op)
    uint32_t op;
    float value;
};
struct ColourProgram {  // (jpgpu_colour_program)
    uint32_t n;
    ColourOp ops[CL_MAX_OPS];
};
// One image of the launch: h x w x 3 bytes at pix, 256-byte aligned, rewritten in place.
struct ColourJob {
    uint8_t *pix;
    uint32_t w, h;
    ColourProgram prog;
};
// What a workgroup keeps in LDS
struct ColourLds {
    uint32_t hist[3 * 256];
    uint32_t sum;
    uint8_t lut[3 * 256];
};

// The refusal rule of one operation: an unknown id; a factor that is not finite, negative or above 256; a SOLARIZE value that is no
// integer in 0..256; a POSTERIZE value that is no integer in 1..8; a HUE shift that is no integer in 0..255; a SHARPNESS factor as the
// other factors.  The other operations ignore their value.
inline bool colour_op_check(uint32_t op, float value) {
    if (op == CL_HUE) return value >= 0.0f && value <= 255.0f && value == floorf(value);
    if (op == CL_SHARPNESS) return value >= 0.0f && value <= CL_MAX_FACTOR;
    if (op >= CL_OPS) return false;
    if (op == CL_BRIGHTNESS || op == CL_CONTRAST || op == CL_COLOR) return value >= 0.0f && value <= CL_MAX_FACTOR;  // (NaN compares false)
    if (op == CL_SOLARIZE) return value >= 0.0f && value <= 256.0f && value == floorf(value);
    if (op == CL_POSTERIZE) return value >= 1.0f && value <= 8.0f && value == floorf(value);
    return true;
}
inline bool colour_program_check(const ColourProgram &p) {
    if (p.n > CL_MAX_OPS) return false;
    for (uint32_t k = 0; k < p.n; k++)
        if (!colour_op_check(p.ops[k].op, p.ops[k].value)) return false;
    return true;
}
// The job of one image (the caller has checked the program; NULL: the empty one)
inline void colour_job(ColourJob &j, uint8_t *pix, uint32_t w, uint32_t h, const ColourProgram *p) {
    j.pix = pix, j.w = w, j.h = h;
    j.prog = ColourProgram{};
    if (!p) return;
    j.prog.n = p->n;
    for (uint32_t k = 0; k < p->n && k < CL_MAX_OPS; k++) j.prog.ops[k] = p->ops[k];
}
// 255.0 / d for d = 1..255 (t[0] is not read): made on the host, so that no device division is involved
inline void colour_scale_table(double t[256]) {
    t[0] = 0.0;
    for (uint32_t d = 1; d < 256u; d++) t[d] = 255.0 / (double)d;
}

// IEEE float32 / double, rounded once per operation.  hipcc contracts a + f * d into a fused multiply-add by default, across statements:
// the pragma takes the permission from the operation itself (warp_band.hpp: wp_mul), and the kernel's disassembly must show no v_fma /
// v_fmac in these paths (profiles/colour/; the divisions of HUE are the only fused operations of the kernel:
// colour_pixel_kernel_resources.txt).  The host's versions store the result before it is used.
JP_CL_BOTH static inline float cl_mulf(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
    return a * b;
#else
    volatile float r = a * b;
    return r;
#endif
}
JP_CL_BOTH static inline float cl_addf(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
    return a + b;
#else
    volatile float r = a + b;
    return r;
#endif
}
JP_CL_BOTH static inline double cl_muld(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
    return a * b;
#else
    volatile double r = a * b;
    return r;
#endif
}
JP_CL_BOTH static inline double cl_addd(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
    return a + b;
#else
    volatile double r = a + b;
    return r;
#endif
}

// blend(a, b, f) of two channel values; |t| <= 255 + 256 * 255 fits an int
JP_CL_BOTH inline uint32_t cl_blend(uint32_t a, uint32_t b, float f) {
    const float d = (float)((int32_t)b - (int32_t)a);
    const float t = cl_addf((float)a, cl_mulf(f, d));
    if (f >= 0.0f && f <= 1.0f) return (uint32_t)(int32_t)t & 255u;  // (t lies between a and b)
    return t <= 0.0f ? 0u : (t >= 255.0f ? 255u : (uint32_t)(int32_t)t);
}
JP_CL_BOTH inline uint32_t cl_luma(uint32_t r, uint32_t g, uint32_t b) { return (r * 19595u + g * 38470u + b * 7471u + 0x8000u) >> 16; }
// the mean of CONTRAST from the sum s of L over n pixels, n <= 2048 x 2048: 2 s + n < 2^32
JP_CL_BOTH inline uint32_t cl_mean(uint32_t s, uint32_t n) { return (2u * s + n) / (2u * n); }

// Entry v of the table of a point operation (IDENTITY and the operations with tables of their own: v)
JP_CL_BOTH inline uint32_t cl_point_value(uint32_t op, float value, uint32_t mean, uint32_t v) {
    switch (op) {
    case CL_BRIGHTNESS: return cl_blend(0u, v, value);
    case CL_CONTRAST: return cl_blend(mean, v, value);
    case CL_SOLARIZE: return v < (uint32_t)value ? v : 255u - v;
    case CL_POSTERIZE: return v & ~((1u << (8u - (uint32_t)value)) - 1u) & 255u;
    case CL_INVERT: return 255u - v;
    default: return v;
    }
}
// AUTOCONTRAST: the least and the greatest value present in h (an empty histogram: lo = 256 > hi = 0: the identity) ...
JP_CL_BOTH inline void cl_hist_range(const uint32_t *h, uint32_t &lo, uint32_t &hi) {
    lo = 256u, hi = 0u;
    for (uint32_t i = 0; i < 256u; i++)
        if (h[i]) {
            if (lo == 256u) lo = i;
            hi = i;
        }
}
// ... and entry v; scale: 255.0 / (hi - lo) out of the host's table
JP_CL_BOTH inline uint32_t cl_autocontrast_value(uint32_t lo, uint32_t hi, double scale, uint32_t v) {
    if (hi <= lo) return v;
    const double offset = cl_muld(-(double)lo, scale);
    const int32_t i = (int32_t)cl_addd(cl_muld((double)v, scale), offset);  // (truncated toward zero; |.| <= 255 * 255 * 2)
    return (uint32_t)(i < 0 ? 0 : (i > 255 ? 255 : i));
}
// EQUALIZE: entry v from the histogram h
JP_CL_BOTH inline uint32_t cl_equalize_value(const uint32_t *h, uint32_t v) {
    uint32_t nz = 0, total = 0, last = 0, before = 0;
    for (uint32_t i = 0; i < 256u; i++) {
        const uint32_t c = h[i];
        if (c) nz++, last = c;
        total += c;
        if (i < v) before += c;
    }
    if (nz < 2u) return v;
    const uint32_t step = (total - last) / 255u;
    if (step == 0u) return v;
    const uint32_t q = (step / 2u + before) / step;
    return q > 255u ? 255u : q;  // (behind the last occupied bin)
}

#ifdef JPGPU_CL_DEVICE_BODY
#if defined(JPGPU_HOST_EMULATION)
static inline void cl_lds_add(uint32_t *p, uint32_t v) { *p += v; }  // (the emulation runs the lanes one after the other)
#else
static __device__ __forceinline__ void cl_lds_add(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
#endif

template <uint32_t NT>
struct CBand {
    static __device__ __forceinline__ bool has_hist(uint32_t op) { return op == CL_AUTOCONTRAST || op == CL_EQUALIZE; }
    static __device__ __forceinline__ bool has_table(uint32_t op) { return op != CL_IDENTITY && op != CL_COLOR && op < CL_OPS; }
    static __device__ __forceinline__ uint32_t byte_of(uint32_t d, uint32_t b) { return (d >> (8u * b)) & 255u; }

    // Four pixels in three dwords (bytes R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3): pixel k's channels
    static __device__ __forceinline__ void unpack4(const uint32_t d[3], uint32_t k, uint32_t &r, uint32_t &g, uint32_t &b) {
        const uint64_t lo = (uint64_t)d[0] | ((uint64_t)d[1] << 32);
        const uint64_t hi = (uint64_t)d[1] | ((uint64_t)d[2] << 32);
        const uint32_t p = k < 2u ? (uint32_t)(lo >> (24u * k)) : (uint32_t)(hi >> (24u * k - 32u));
        r = p & 255u, g = (p >> 8) & 255u, b = (p >> 16) & 255u;
    }

    // phase 0: the statistics of the operation to zero
    static __device__ __forceinline__ void zero(uint32_t op, uint32_t tid, ColourLds &l) {
        if (has_hist(op))
            for (uint32_t i = tid; i < 768u; i += NT) l.hist[i] = 0u;
        if (op == CL_CONTRAST && tid == 0u) l.sum = 0u;
    }

    // phase 1: the sum of L (CONTRAST) or the three histograms (AUTOCONTRAST, EQUALIZE) of the current image
    static __device__ __forceinline__ void accumulate(const ColourJob &j, uint32_t op, uint32_t tid, ColourLds &l) {
        const uint32_t npx = j.w * j.h, nb = npx * 3u;
        const JP_GLOBAL uint8_t *pb = (const JP_GLOBAL uint8_t *)j.pix;
        const JP_GLOBAL uint32_t *pd = (const JP_GLOBAL uint32_t *)j.pix;
        if (op == CL_CONTRAST) {
            uint32_t s = 0u;
            for (uint32_t g = tid; g < npx / 4u; g += NT) {
                const uint32_t d[3] = {pd[3u * g], pd[3u * g + 1u], pd[3u * g + 2u]};
#pragma unroll
                for (uint32_t k = 0; k < 4u; k++) {
                    uint32_t r, gg, b;
                    unpack4(d, k, r, gg, b);
                    s += cl_luma(r, gg, b);
                }
            }
            if (tid == 0u)
                for (uint32_t p = npx & ~3u; p < npx; p++) s += cl_luma(pb[3u * p], pb[3u * p + 1u], pb[3u * p + 2u]);
            if (s) cl_lds_add(&l.sum, s);
        } else if (has_hist(op)) {
            for (uint32_t q = tid; q < nb / 4u; q += NT) {
                const uint32_t d = pd[q], c0 = q % 3u;  // (byte 4 q is channel q mod 3)
#pragma unroll
                for (uint32_t b = 0; b < 4u; b++) {
                    const uint32_t c = c0 + b >= 3u ? c0 + b - 3u : c0 + b;
                    cl_lds_add(&l.hist[c * 256u + byte_of(d, b)], 1u);
                }
            }
            if (tid == 0u)
                for (uint32_t x = nb & ~3u; x < nb; x++) cl_lds_add(&l.hist[(x % 3u) * 256u + pb[x]], 1u);
        }
    }

    // phase 2: the table, a lane per entry; scale: the host's table of 255.0 / d
    static __device__ __forceinline__ void table(const ColourJob &j, const ColourOp &o, const JP_GLOBAL double *scale, uint32_t tid, ColourLds &l) {
        if (!has_table(o.op)) return;
        for (uint32_t i = tid; i < 768u; i += NT) {
            const uint32_t c = i >> 8, v = i & 255u;
            uint32_t out;
            if (o.op == CL_AUTOCONTRAST) {
                uint32_t lo, hi;
                cl_hist_range(l.hist + c * 256u, lo, hi);
                out = cl_autocontrast_value(lo, hi, hi > lo ? scale[hi - lo] : 0.0, v);
            } else if (o.op == CL_EQUALIZE) {
                out = cl_equalize_value(l.hist + c * 256u, v);
            } else {
                out = cl_point_value(o.op, o.value, o.op == CL_CONTRAST ? cl_mean(l.sum, j.w * j.h) : 0u, v);
            }
            l.lut[i] = (uint8_t)out;
        }
    }

    // phase 3: the image through the table, or (COLOR) every pixel blended with its L
    static __device__ __forceinline__ void apply(const ColourJob &j, const ColourOp &o, uint32_t tid, const ColourLds &l) {
        const uint32_t npx = j.w * j.h, nb = npx * 3u;
        JP_GLOBAL uint8_t *pb = (JP_GLOBAL uint8_t *)j.pix;
        JP_GLOBAL uint32_t *pd = (JP_GLOBAL uint32_t *)j.pix;
        if (o.op == CL_COLOR) {
            const float f = o.value;
            for (uint32_t g = tid; g < npx / 4u; g += NT) {
                const uint32_t d[3] = {pd[3u * g], pd[3u * g + 1u], pd[3u * g + 2u]};
                uint64_t lo = 0u, hi = 0u;  // (bytes 0..7 and 4..11 of the twelve)
#pragma unroll
                for (uint32_t k = 0; k < 4u; k++) {
                    uint32_t r, gg, b;
                    unpack4(d, k, r, gg, b);
                    const uint32_t y = cl_luma(r, gg, b);
                    const uint64_t p = (uint64_t)(cl_blend(y, r, f) | (cl_blend(y, gg, f) << 8) | (cl_blend(y, b, f) << 16));
                    if (k < 2u) lo |= p << (24u * k);
                    else hi |= p << (24u * k - 32u);
                }
                pd[3u * g] = (uint32_t)lo;
                pd[3u * g + 1u] = (uint32_t)(lo >> 32) | (uint32_t)hi;
                pd[3u * g + 2u] = (uint32_t)(hi >> 32);
            }
            if (tid == 0u)
                for (uint32_t p = npx & ~3u; p < npx; p++) {
                    const uint32_t r = pb[3u * p], g = pb[3u * p + 1u], b = pb[3u * p + 2u], y = cl_luma(r, g, b);
                    pb[3u * p] = (uint8_t)cl_blend(y, r, f), pb[3u * p + 1u] = (uint8_t)cl_blend(y, g, f), pb[3u * p + 2u] = (uint8_t)cl_blend(y, b, f);
                }
            return;
        }
        if (!has_table(o.op)) return;
        for (uint32_t q = tid; q < nb / 4u; q += NT) {
            const uint32_t d = pd[q], c0 = q % 3u;
            uint32_t out = 0u;
#pragma unroll
            for (uint32_t b = 0; b < 4u; b++) {
                const uint32_t c = c0 + b >= 3u ? c0 + b - 3u : c0 + b;
                out |= (uint32_t)l.lut[c * 256u + byte_of(d, b)] << (8u * b);
            }
            pd[q] = out;
        }
        if (tid == 0u)
            for (uint32_t x = nb & ~3u; x < nb; x++) pb[x] = l.lut[(x % 3u) * 256u + pb[x]];
    }

    // Lane tid's share of phase `phase` of operation k of the job.  The caller puts a barrier behind every phase.
    static __device__ __forceinline__ void phase(const ColourJob &j, uint32_t k, uint32_t phase, const JP_GLOBAL double *scale, uint32_t tid, ColourLds &l) {
        const ColourOp o = j.prog.ops[k];
        if (phase == 0u) zero(o.op, tid, l);
        else if (phase == 1u) accumulate(j, o.op, tid, l);
        else if (phase == 2u) table(j, o, scale, tid, l);
        else apply(j, o, tid, l);
    }
};
#endif  // JPGPU_CL_DEVICE_BODY

}  // namespace jpgpu

#if defined(__HIP__) && !defined(JPGPU_HOST_EMULATION)
namespace jpgpu {
// colour.hip: n_images jobs, a workgroup each, on `stream`; d_scale: colour_scale_table on the device; strip_rows: the rows of a
// SHARPNESS strip when not 0 (colour_pixel_band.hpp: cl_strip_rows)
hipError_t launch_colour(const ColourJob *d_jobs, const double *d_scale, uint32_t n_images, uint32_t strip_rows, hipStream_t stream);
}  // namespace jpgpu
#endif
